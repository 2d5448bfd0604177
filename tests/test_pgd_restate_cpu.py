"""The PGD restatement (pgd_restate.py) against what the reference's own loops returned (tests/golden/golden_pgd_v1.npz, written by
tests/golden/make_golden_pgd.py from the two scripts' ``pgd`` and ``AudioAttack.stage_1``), bit for bit -- this pins the reference that
test_gpu_pgd.py holds the kernels and ``audiopure_amd.attacks`` to -- the conditions the fixture's cases were built for, and the
host-side refusals of ``audiopure_amd.attacks.pgd``."""
import os
import re

import numpy as np
import pytest
import torch

import pgd_restate as R
from audiopure_amd import _native as N
from audiopure_amd import attacks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_float32_restatement_equals_the_reference_bit_for_bit(name, form):
    x_adv, found = R.restated(name, form)
    ref = R.golden()[f"{name}/{form}/x_adv"]
    assert x_adv.shape == ref.shape and np.array_equal(bits(x_adv.numpy()), bits(ref))
    if form.startswith("stage1"):
        assert found.tolist() == R.golden()[f"{name}/{form}/success"].tolist()


def test_the_cases_hold_what_they_were_built_for():
    c, g = R.case("b5"), R.golden()
    B, L, n = R.CASES["b5"]
    pred = np.stack([torch.from_numpy(s).max(1)[1].numpy() for s in c["scores"]])
    assert np.array_equal(pred, c["pred"])                       # torch's argmax (lowest index of a tie, a NaN is the maximum)
    hit = pred != c["y"][None]
    assert hit[:, 0].tolist() == [True, False, True, True, True]            # hit, miss, hit: the last hit wins
    assert not hit[:, 1].any()                                              # never hit: the fallback row
    assert hit[:, 2].tolist() == [True] + [False] * n                       # hit at the tie alone; the other index of the tie is y
    assert c["scores"][0, 2, 1] == c["scores"][0, 2, 4] == c["scores"][0, 2].max() and c["y"][2] == 4
    assert np.isnan(c["scores"][1, 3, 2]) and np.nanargmax(c["scores"][1, 3]) == c["y"][3]   # ignoring the NaN would miss the row
    assert hit[:, 3].tolist() == [True, True] + [False] * (n - 1)
    hit_t = pred == c["y_t"][None]
    assert hit_t[:, 0].tolist() == [True, False, True, True, True] and not hit_t[:, 1].any() and hit_t[:, 3].tolist() == [False, True, False, False, False]
    G = c["G"]
    assert np.isnan(G).any() and (G == 0).any() and np.signbit(G[G == 0]).any() and not np.signbit(G[G == 0]).all()
    tiny = np.abs(G[np.isfinite(G) & (G != 0)])
    assert (tiny < np.finfo(np.float32).tiny).any()                         # denormals
    x = c["x"]
    assert (x == 1).any() and (x == -1).any() and ((x < 1) & (x > 1 - R.EPS)).any() and ((x > -1) & (x < -1 + R.EPS)).any()
    # the box clamp is active on both sides, and delta + step leaves the eps ball: the result sits on +-1 / on the ball's surface
    xa = g["b5/convnet/x_adv"]
    assert ((xa == 1) & (x < 1)).any() and ((xa == -1) & (x > -1)).any()
    d = (xa.astype(np.float64) - x)[(np.abs(x) < 0.9)]
    assert np.isclose(np.abs(d).max(), R.EPS, rtol=1e-3) and 3 * R.ALPHA > R.EPS and 3 * R.LR > R.EPS
    assert (np.abs(g["b5/u"] * 2 - 1) * R.EPS + R.ALPHA > R.EPS).any()
    # the KWS script's never-zeroed delta.grad is a different loop, and the fixture shows it
    assert not np.array_equal(bits(g["b5/kws/x_adv"]), bits(xa))
    assert os.path.getsize(R.GOLDEN) < 160 * 1024


def test_float64_restatement_follows_the_float32_one():
    """the float64 run of the same loop (what test_gpu_pgd.py measures the l2 step against) agrees to float32 rounding"""
    c, g = R.case("b5"), R.golden()
    B, L, n = R.CASES["b5"]
    x, y, u = torch.from_numpy(c["x"]), torch.from_numpy(c["y"]), torch.from_numpy(g["b5/u"])
    x64, _ = R.pgd_loop(R.model_of(c, "G_l2"), x, y, R.EPS, R.ALPHA, n, p="l2", u=u, dtype=torch.float64)
    assert x64.dtype == torch.float64 and R.rel(g["b5/convnet_l2/x_adv"], x64.numpy()) < 4 * 2.0 ** -24


def test_pgd_refuses_cpu_tensors_and_an_unknown_norm():
    x, y = torch.zeros(2, 1, 8), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(N.NativeError, match="no CPU path"):
        attacks.pgd(lambda v: v, x, y)
    with pytest.raises(NotImplementedError, match=re.escape("Unsupported norm: l1!")):
        attacks.pgd(lambda v: v, x, y, p="l1")
    assert not attacks.stage_1_served(type("A", (), {"norm": "linf"})(), x, y)


def test_the_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "audiopure.h")).read()
    for name in ("ap_pgd_init", "ap_pgd_step_linf", "ap_pgd_step_l2", "ap_pgd_l2_workspace_bytes", "ap_pgd_chunk"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in N.SIGNATURES, name
    lib = N.lib()
    chunk = lib.ap_pgd_chunk()
    assert chunk == 4096
    assert lib.ap_pgd_l2_workspace_bytes(3, chunk) == 2 * 3 * 8 and lib.ap_pgd_l2_workspace_bytes(3, chunk + 1) == 2 * 3 * 2 * 8
    assert lib.ap_pgd_l2_workspace_bytes(0, 5) == 0


def test_kernel_entry_points_refuse_before_any_launch():
    """every refusal is -22 with the error text set; none of these calls reaches a launch (there is no device here)"""
    lib = N.lib()
    p = 4096                                                     # stand-in non-null addresses, far enough apart
    a = [p * (i + 1) for i in range(8)]
    assert lib.ap_pgd_init(None, None, a[1], a[2], 0.1, 1, 4, None) == -22 and b"null" in lib.ap_last_error()
    assert lib.ap_pgd_init(a[0], None, a[1], a[2], -1.0, 1, 4, None) == -22 and b"eps" in lib.ap_last_error()
    assert lib.ap_pgd_init(a[0], None, a[1], a[1], 0.1, 1, 4, None) == -22 and b"overlap" in lib.ap_last_error()
    assert lib.ap_pgd_init(a[0], None, a[1], a[2], 0.1, 70000, 4, None) == -22 and b"B = 70000" in lib.ap_last_error()
    step = lambda **k: lib.ap_pgd_step_linf(*[k.get(n, d) for n, d in (     # noqa: E731
        ("x", a[0]), ("g", a[1]), ("delta", a[2]), ("x_pert", a[3]), ("x_adv", a[4]), ("found", a[5]), ("pred", a[6]), ("scores", None),
        ("K", 0), ("y", a[7]), ("step", 0.1), ("eps_rows", None), ("eps", 0.1), ("targeted", 0), ("last", 0), ("B", 1), ("n", 4), ("stream", None))])
    assert step(g=None) == -22 and b"null g" in lib.ap_last_error()
    assert step(scores=a[6]) == -22 and b"one of the two" in lib.ap_last_error()
    assert step(pred=None) == -22 and b"one of the two" in lib.ap_last_error()
    assert step(pred=None, scores=a[6], K=5000) == -22 and b"K = 5000" in lib.ap_last_error()
    assert step(x_adv=a[3]) == -22 and b"overlaps" in lib.ap_last_error()
    assert step(eps=float("nan")) == -22 and b"eps" in lib.ap_last_error()
    assert step(n=0) == -22
    rc = lib.ap_pgd_step_l2(a[0], a[1], a[2], a[3], a[4], a[5], a[6], None, 0, a[7], 0.1, None, 0.1, 0, 0, None, 0, 1, 4, None)
    assert rc == -22 and b"workspace" in lib.ap_last_error()


def test_dropin_adds_a_native_stage_1_subclass_and_leaves_audio_attack_alone(tmp_path):
    """``NativeStage1AudioAttack`` overrides ``stage_1`` alone; what the native loop does not serve -- here CPU tensors, and the l2
    norm -- runs the checkout's method (a stand-in checkout whose ``stage_1`` says so)."""
    from test_psy_cpu import STANDIN_WBA, _run
    os.makedirs(tmp_path / "robustness_eval")
    (tmp_path / "robustness_eval" / "_EOT.py").write_text("class EOT:\n    pass\n")
    (tmp_path / "robustness_eval" / "white_box_attack.py").write_text(STANDIN_WBA)
    out = _run("""
        import sys, torch
        import robustness_eval.white_box_attack as wba
        ref = sys.modules["robustness_eval._checkout_white_box_attack"]
        assert issubclass(wba.NativeStage1AudioAttack, wba.AudioAttack) and wba.AudioAttack.stage_1 is ref.AudioAttack.stage_1
        assert {k for k, v in vars(wba.NativeStage1AudioAttack).items() if callable(v)} == {"stage_1"}
        attack = wba.NativeStage1AudioAttack(model=None)
        x, y = torch.zeros(2, 1, 8), torch.zeros(2, dtype=torch.int64)
        for norm in ("linf", "l2"):
            attack.norm = norm
            assert attack.stage_1(x, y) == "stage_1 of the checkout" and attack.generate(x, y) == "stage_1 of the checkout"
        print("OK")
        """, checkout=str(tmp_path))
    assert "OK" in out


def test_stage_1_reads_only_attributes_a_reference_attack_carries():
    """the fixture records the attribute names of the reference's ``AudioAttack`` instances; the native stage 1 reads these of
    them, and the stand-in checkout of the GPU test sets the same"""
    import inspect
    names = set(R.golden()["audio_attack/attributes"].tolist())
    assert set(attacks.STAGE_1_READS) <= names
    read = set(re.findall(r"\battack\.(\w+)", inspect.getsource(attacks.stage_1) + inspect.getsource(attacks.stage_1_served)))
    assert read == set(attacks.STAGE_1_READS), read ^ set(attacks.STAGE_1_READS)
    standin = set(re.findall(r"self\.(\w+)(?:,| =)", R.STANDIN_CHECKOUT)) - {"ran"}
    assert standin <= names and set(attacks.STAGE_1_READS) - {"eot_model"} <= standin
