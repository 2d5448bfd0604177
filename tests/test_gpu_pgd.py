"""The PGD kernels (ap_attack.hip) and ``audiopure_amd.attacks`` on the device against pgd_restate.py, whose float32 form
test_pgd_restate_cpu.py pins bit for bit to the reference's own loops.  ap_pgd_init and ap_pgd_step_linf: equal bits.  ap_pgd_step_l2:
within 4 x the float32 restatement's own error against the float64 one on the same inputs, per tensor as max |d| / max |ref|, computed
here (the kernel adds its norms in fp64, so it is held to the float64 expression, not to float32 torch's bits).  Outputs are
NaN-filled before a call where the call must write them."""
import copy
import functools

import numpy as np
import pytest
import torch

import pgd_restate as R
from audiopure_amd import _native as N
from audiopure_amd import attacks
from audiopure_amd import losses as L

pytestmark = pytest.mark.gpu
ids = lambda c: "-".join(map(str, c))       # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def rows(a, dev, unaligned):
    """a [B, n] float32 array on the device; unaligned: the rows of a buffer sliced at [1:], so no row base is 16-byte aligned when n
    is odd and the first never is"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not unaligned:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


def nan_rows(shape, dev, unaligned):
    return rows(np.full(shape, np.nan, np.float32), dev, unaligned)


def _cpu(k, name, dtype=torch.float32):
    t = torch.from_numpy(k[name])
    return t.to(dtype) if t.is_floating_point() else t


@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "sliced"])
@pytest.mark.parametrize("shape", R.KERNEL_SHAPES, ids=ids)
def test_init_and_linf_step_equal_the_restatement_bit_for_bit(dev, shape, unaligned):
    B, n = shape
    if unaligned and n % 2 == 0:
        n += 1                                                   # an odd row length: every row base at another offset
    k = R.kernel_inputs(B, n)
    lib, st = N.lib(), N.stream()
    x, u, g = (rows(k[a], dev, unaligned) for a in ("x", "u", "g"))
    y, pred, scores = (torch.from_numpy(k[a]).to(dev) for a in ("y", "pred", "scores"))
    eps_rows = torch.from_numpy(k["eps_rows"]).to(dev)
    # the random start, and the zero start
    for noise in (u, None):
        delta, x_pert = nan_rows((B, n), dev, unaligned), nan_rows((B, n), dev, unaligned)
        N.check(lib.ap_pgd_init(N.ptr(x), N.ptr(noise), N.ptr(delta), N.ptr(x_pert), R.EPS, B, n, st), "ap_pgd_init")
        rd, rp = R.init(_cpu(k, "x"), None if noise is None else _cpu(k, "u"), R.EPS)
        assert same_bits(delta, rd) and same_bits(x_pert, rp)
    # one iteration: scalar and per-row eps, both targets, last on and off, the prediction given and taken from the scores
    for targeted in (False, True):
        for per_row in (False, True):
            for last in (False, True):
                for own_argmax in (False, True):
                    delta, x_pert, x_adv = (rows(k[a], dev, unaligned) for a in ("delta", "x_pert", "x_adv"))
                    found = torch.from_numpy(k["found"]).to(dev)
                    step = -R.LR if targeted else R.ALPHA
                    N.check(lib.ap_pgd_step_linf(N.ptr(x), N.ptr(g), N.ptr(delta), N.ptr(x_pert), N.ptr(x_adv), found.data_ptr(),
                                                 None if own_argmax else pred.data_ptr(), N.ptr(scores) if own_argmax else None, R.K,
                                                 y.data_ptr(), step, N.ptr(eps_rows) if per_row else None, 0.0 if per_row else R.EPS,
                                                 int(targeted), int(last), B, n, st), "ap_pgd_step_linf")
                    ref = R.step_linf(_cpu(k, "x"), _cpu(k, "g"), _cpu(k, "delta"), _cpu(k, "x_pert"), _cpu(k, "x_adv"), _cpu(k, "found").bool(),
                                      _cpu(k, "pred"), _cpu(k, "y"), step, _cpu(k, "eps_rows") if per_row else R.EPS, targeted, last)
                    what = (targeted, per_row, last, own_argmax)
                    assert same_bits(delta, ref[0]) and same_bits(x_pert, ref[1]), what
                    assert same_bits(x_adv, ref[2]) and torch.equal(found.cpu().bool(), ref[3]), what
                    if last:                                     # nothing but x_adv is written
                        assert same_bits(delta, _cpu(k, "delta")) and same_bits(x_pert, _cpu(k, "x_pert")), what
    assert not np.isnan(k["delta"]).any() and np.isnan(k["g"]).any() == (n > 1)


@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "sliced"])
@pytest.mark.parametrize("shape", R.KERNEL_SHAPES, ids=ids)
def test_l2_step_follows_float64_within_four_times_float32s_own_error(dev, shape, unaligned):
    B, n = shape
    if unaligned and n % 2 == 0:
        n += 1
    k = R.kernel_inputs(B, n, l2=True)
    lib, st = N.lib(), N.stream()
    x, g = rows(k["x"], dev, unaligned), rows(k["g"], dev, unaligned)
    y, pred = torch.from_numpy(k["y"]).to(dev), torch.from_numpy(k["pred"]).to(dev)
    eps_rows = torch.from_numpy(k["eps_rows"]).to(dev)
    ws = torch.full((lib.ap_pgd_l2_workspace_bytes(B, n) // 8,), float("nan"), dtype=torch.float64, device=dev)
    assert ws.numel() == 2 * B * -(-n // lib.ap_pgd_chunk())
    if B > 1:
        assert not k["g"][1].any()                               # the zero-gradient row
    for per_row in (False, True):
        def restate(dtype):
            return R.step_l2(_cpu(k, "x", dtype), _cpu(k, "g", dtype), _cpu(k, "delta", dtype), _cpu(k, "x_pert", dtype), _cpu(k, "x_adv", dtype),
                             _cpu(k, "found").bool(), _cpu(k, "pred"), _cpu(k, "y"), R.ALPHA, _cpu(k, "eps_rows", dtype) if per_row else R.EPS)
        r64, r32 = restate(torch.float64), restate(torch.float32)
        runs = []
        for _ in range(2):
            delta, x_pert, x_adv = (rows(k[a], dev, unaligned) for a in ("delta", "x_pert", "x_adv"))
            found = torch.from_numpy(k["found"]).to(dev)
            ws.fill_(float("nan"))
            N.check(lib.ap_pgd_step_l2(N.ptr(x), N.ptr(g), N.ptr(delta), N.ptr(x_pert), N.ptr(x_adv), found.data_ptr(), pred.data_ptr(), None, 0,
                                       y.data_ptr(), R.ALPHA, N.ptr(eps_rows) if per_row else None, 0.0 if per_row else R.EPS, 0, 0,
                                       ws.data_ptr(), ws.numel() * 8, B, n, st), "ap_pgd_step_l2")
            runs.append((delta, x_pert, x_adv, found))
        for a, b in zip(*runs):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))        # two runs give equal bits
        delta, x_pert, x_adv, found = runs[0]
        assert not torch.isnan(delta).any() and not torch.isnan(x_pert).any()   # (the zero-norm row: 1 / 0 = inf, min(1, inf) = 1)
        for name, got, i in (("delta", delta, 0), ("x_pert", x_pert, 1)):
            bound = 4 * R.rel(r32[i].numpy(), r64[i].numpy())
            err = R.rel(got.cpu().numpy(), r64[i].numpy())
            print(f"l2 {B}x{n} per_row={per_row} {name}: kernel {err:.3e}, float32 restatement {bound / 4:.3e} (bound {bound:.3e})")
            assert err <= bound, (name, per_row)
        assert same_bits(x_adv, r32[2]) and torch.equal(found.cpu().bool(), r32[3])         # the bookkeeping is exact
        if B > 2:                                                # the row that stays inside the ball: both factors exactly 1
            v = torch.from_numpy(k["delta"][2]) + R.ALPHA * torch.from_numpy(k["g"][2])
            assert float(torch.from_numpy(k["g"][2]).double().norm()) < 1 and float(v.double().norm()) < R.EPS
            assert same_bits(delta[2], R.box(torch.from_numpy(k["x"][2]), v)[0])
    # last: the fallback alone, no workspace read
    delta, x_pert, x_adv = (rows(k[a], dev, unaligned) for a in ("delta", "x_pert", "x_adv"))
    found = torch.from_numpy(k["found"]).to(dev)
    N.check(lib.ap_pgd_step_l2(N.ptr(x), None, N.ptr(delta), N.ptr(x_pert), N.ptr(x_adv), found.data_ptr(), pred.data_ptr(), None, 0, y.data_ptr(),
                               R.ALPHA, None, R.EPS, 0, 1, None, 0, B, n, st), "ap_pgd_step_l2")
    ref = R.step_l2(_cpu(k, "x"), None, _cpu(k, "delta"), _cpu(k, "x_pert"), _cpu(k, "x_adv"), _cpu(k, "found").bool(), _cpu(k, "pred"),
                    _cpu(k, "y"), R.ALPHA, R.EPS, last=True)
    assert same_bits(x_adv, ref[2]) and same_bits(delta, ref[0]) and same_bits(x_pert, ref[1]) and torch.equal(found.cpu().bool(), ref[3])


class _Attack:
    """what ``attacks.stage_1`` reads of an ``AudioAttack``"""

    def __init__(self, model, n, targeted, norm="linf"):
        self.model, self.criterion, self.eps, self.norm = model, torch.nn.CrossEntropyLoss(), R.EPS, norm
        self.learning_rate_1, self.max_iter_1, self._targeted = R.LR, n, targeted
        self.eot_attack_size = self.eot_defense_size = 1
        self.verbose = 0


@pytest.mark.parametrize("name", list(R.CASES))
def test_fixture_cases_with_the_scripted_model_equal_the_reference_bit_for_bit(dev, name):
    c, g = R.case(name), R.golden()
    B, L, n = R.CASES[name]
    x, y, y_t, u = (torch.from_numpy(a).to(dev) for a in (c["x"], c["y"], c["y_t"], g[f"{name}/u"]))
    # RCNN_KWS/train.py's form: transform and criterion passed, delta.grad never zeroed
    m = R.model_of(c)
    got = attacks.pgd(m, x, y, eps=R.EPS, alpha=R.ALPHA, n=n, transform=lambda v: v, criterion=torch.nn.CrossEntropyLoss(), noise=u, accumulate=True)
    assert m.calls == n + 1 and same_bits(got, torch.from_numpy(g[f"{name}/kws/x_adv"]))
    # adv_train_speech_commands.py's form, through the native loss head, and through a criterion called as it is
    for criterion in (None, lambda s, t: torch.nn.functional.cross_entropy(s, t)):
        got, found = attacks.pgd(R.model_of(c), x, y, eps=R.EPS, alpha=R.ALPHA, n=n, p="linf", noise=u, criterion=criterion, return_found=True)
        assert same_bits(got, torch.from_numpy(g[f"{name}/convnet/x_adv"]))
        assert found.cpu().tolist() == R.restated(name, "convnet")[1].tolist()
    # stage 1, targeted and untargeted
    for form, targeted, labels in (("stage1_t", True, y_t), ("stage1_u", False, y)):
        attack = _Attack(R.model_of(c), n, targeted)
        assert attacks.stage_1_served(attack, x, labels)
        x_adv, success = attacks.stage_1(attack, x, labels)
        assert same_bits(x_adv, torch.from_numpy(g[f"{name}/{form}/x_adv"])) and success == g[f"{name}/{form}/success"].tolist()
    # a per-row bound that the kernel would misread is refused on the host
    run = attacks.PgdRun(x, y)
    run.start(None)
    rows_eps = torch.full((B,), R.EPS, device=dev)
    for bad, err in ((rows_eps.double(), ValueError), (rows_eps[:-1] if B > 1 else rows_eps.reshape(1, B), ValueError), (rows_eps.cpu(), N.NativeError)):
        with pytest.raises(err, match="per-row eps"):
            run.step(torch.from_numpy(c["scores"][0]).to(dev), None, R.ALPHA, bad, last=True)
    # l2, 16-bit data and CPU tensors are not served (the drop-in then calls the checkout's method)
    assert not attacks.stage_1_served(_Attack(None, n, True, norm="l2"), x, y)
    assert not attacks.stage_1_served(_Attack(None, n, True), x.to(torch.int16), y)
    assert not attacks.stage_1_served(_Attack(None, n, True), x.cpu(), y.cpu())
    with pytest.raises(N.NativeError):
        attacks.stage_1(_Attack(None, n, True, norm="l2"), x, y)
    # the l2 form follows the reference to float32 rounding: its norms are added in another order, so a proposal d may differ in its
    # last bit, which moves an element only where the rounding of x + d (|x| <= 1: 2^-24 at the most) then falls the other way --
    # once per update at the worst, and once more in the final x + delta
    got = attacks.pgd(R.model_of(c, "G_l2"), x, y, eps=R.EPS, alpha=R.ALPHA, n=n, p="l2", noise=u)
    assert float((got.cpu() - torch.from_numpy(g[f"{name}/convnet_l2/x_adv"])).abs().max()) <= (n + 1) * 2.0 ** -24


DROPIN_CHILD = """
    import sys
    import torch
    sys.path.insert(0, %r)
    import pgd_restate as R
    import robustness_eval.white_box_attack as wba
    assert wba.__file__.replace(chr(92), "/").endswith("dropin/robustness_eval/white_box_attack.py"), wba.__file__
    dev, g = torch.device("cuda:0"), R.golden()
    bits = lambda t: t.detach().cpu().contiguous().view(torch.int32)
    for name, (B, L, n) in R.CASES.items():
        c = R.case(name)
        x, y, y_t = (torch.from_numpy(a).to(dev) for a in (c["x"], c["y"], c["y_t"]))
        for form, targeted, labels in (("stage1_t", True, y_t), ("stage1_u", False, y)):
            for eot in (1, 2):
                model = R.model_of(c)
                attack = wba.NativeStage1AudioAttack(model, masker=None, criterion=torch.nn.CrossEntropyLoss(), eps=R.EPS, norm="linf",
                                                     learning_rate_1=R.LR, max_iter_1=n, max_iter_2=0, eot_attack_size=eot,
                                                     eot_defense_size=eot, verbose=int(eot == 1))
                attack._targeted = not targeted                  # generate() sets it
                if eot > 1:
                    attack.eot_model = R.ScriptedEOT(c)
                x_adv, success = attack.generate(x, labels, targeted=targeted)
                want, ok = torch.from_numpy(g[name + "/" + form + "/x_adv"]), g[name + "/" + form + "/success"].tolist()
                assert x_adv.shape == want.shape and torch.equal(bits(x_adv), bits(want)), (name, form, eot)
                assert success == ok and not attack.ran, (name, form, eot)
                if eot > 1:
                    assert model.calls == 0 and attack.eot_model.asked == [(2, False), (2, True)] * n + [(2, False)]
                else:
                    assert model.calls == n + 1
                    print("FAILED ROWS", name, form, ok.count(False))
        # norm l2 is not served: the checkout's method runs (the stand-in's records that it did), also through generate()
        attack.norm = "l2"
        assert attack.stage_1(x, y) == "stage_1 of the checkout" and attack.generate(x, y) == "stage_1 of the checkout"
        assert attack.ran == ["l2", "l2"]
        # ... and so it does for 16-bit data and CPU tensors under linf
        attack.norm = "linf"
        assert attack.stage_1(x.to(torch.int16), y) == attack.stage_1(x.cpu(), y.cpu()) == "stage_1 of the checkout"
        assert attack.ran == ["l2", "l2", "linf", "linf"]
    print("OK")
"""


def test_dropin_native_stage_1_equals_the_reference_and_hands_l2_to_the_checkout(tmp_path):
    """``robustness_eval.white_box_attack.NativeStage1AudioAttack`` through the drop-in package over a stand-in checkout, in a child
    process (the drop-in finds its checkout on the package path at import): ``generate`` -> ``stage_1`` -> ap_pgd_step_linf on the
    fixture's cases equals the reference's ``x_adv`` and ``success``, targeted and untargeted, with the plain model / criterion calls and
    with both EOT branches; the 'not successful' lines of verbose mode are printed for the rows that failed; with norm 'l2' the
    checkout's ``stage_1`` runs, shown by its recorder."""
    import os
    from test_psy_cpu import _run
    os.makedirs(tmp_path / "robustness_eval")
    (tmp_path / "robustness_eval" / "_EOT.py").write_text("class EOT:\n    pass\n")
    (tmp_path / "robustness_eval" / "white_box_attack.py").write_text(R.STANDIN_CHECKOUT)
    out = _run(DROPIN_CHILD % os.path.dirname(os.path.abspath(__file__)), checkout=str(tmp_path))
    assert "OK" in out
    failed = [int(line.split()[-1]) for line in out.splitlines() if line.startswith("FAILED ROWS")]
    assert len(failed) == 2 * len(R.CASES) and out.count("was not successful") == sum(failed) > 0


# ---------------------------------------------------------------------------------------------------------
# real modules, n = 2
# ---------------------------------------------------------------------------------------------------------
N_ITER = 2


def _wave(B, Ln, seed):
    r = np.random.default_rng(seed)
    t = np.arange(Ln) / 16000.0
    x = 0.4 * np.sin(2 * np.pi * (200.0 + 150.0 * np.arange(B))[:, None] * t) + 0.05 * r.standard_normal((B, Ln))
    return torch.from_numpy(x.astype(np.float32)).reshape(B, 1, Ln), torch.from_numpy(r.random((B, 1, Ln)).astype(np.float32))


def _kws(dev):
    import kws_restate as KR
    from audiopure_amd.audio_models.RCNN_KWS import KWSModel
    from audiopure_amd.transforms.melspec import MelSpecDBHTK
    n_mels, H, Kc = KR.GOLDEN_SHAPE
    m = KWSModel(in_size=n_mels, hidden_size=H, num_classes=Kc)
    m.load_state_dict(KR.kws_weights(n_mels, H, Kc))
    return m.to(dev).train(), MelSpecDBHTK(n_mels), Kc


@functools.lru_cache(maxsize=None)
def _resnet():
    import synth_convnets as S
    return S.synth_init(S.ResNet50(num_classes=10, in_channels=1, reps=(1, 1, 1, 1)), seed=3)


def _convnet(dev, train):
    from audiopure_amd.convnet import NativeConvNet
    from audiopure_amd.transforms.melspec import MelSpecDB
    net = NativeConvNet(copy.deepcopy(_resnet()).to(dev), (1, 32, 32))
    return (net.train() if train else net.eval()), MelSpecDB(32), 10


def _state(model):
    flags = [p.requires_grad for p in model.parameters()]
    grads = [p.grad for p in model.parameters()]
    return flags, grads


@pytest.mark.parametrize("which", ["kws-train", "kws-train-accumulate", "convnet-train", "convnet-eval"])
def test_real_modules_equal_the_restated_loop_and_leave_the_parameters_alone(dev, which):
    accumulate = which == "kws-train-accumulate"                 # the KWS script's own form: the running sum of the gradients, added in place
    if which.startswith("kws-train"):
        (a, mel, Kc), (b, _, _) = _kws(dev), _kws(dev)
        x, u = _wave(3, 4000, 1)
    else:
        (a, mel, Kc), (b, _, _) = _convnet(dev, which == "convnet-train"), _convnet(dev, which == "convnet-train")
        x, u = _wave(4, 16000, 2)
    x, u = x.to(dev), u.to(dev)
    y = (torch.arange(x.shape[0], device=dev) * 3 + 1) % Kc
    list(a.parameters())[0].requires_grad_(False)                # a flag that is off before the call stays off after it
    flags = [p.requires_grad for p in a.parameters()]
    eps = 0.002
    got, found = attacks.pgd(a, x, y, eps=eps, alpha=eps / 5, n=N_ITER, transform=mel, criterion=L.CrossEntropyLoss(), noise=u, return_found=True,
                             accumulate=accumulate)
    assert [p.requires_grad for p in a.parameters()] == flags and all(p.grad is None for p in a.parameters())
    with attacks._frozen(b):                                     # the restated loop on PyTorch operators over the same native modules
        ref, ref_found = R.pgd_loop(b, x, y, eps, eps / 5, N_ITER, transform=mel, criterion=L.CrossEntropyLoss(), u=u, accumulate=accumulate)
    assert same_bits(got, ref) and torch.equal(found, ref_found)
    assert 0 < float((got - x).abs().max()) <= eps + 2.0 ** -24      # (the ball, and one rounding of x + d at |x| < 1)
    if which.startswith("convnet"):
        sa, sb = a.module.state_dict(), b.module.state_dict()
        moved = 0
        for k in sa:
            if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
                assert torch.equal(sa[k], sb[k]), k
                moved += int(not torch.equal(sa[k].cpu(), _resnet().state_dict()[k]))
                if k.endswith("num_batches_tracked"):
                    assert int(sa[k]) == 100 + (N_ITER + 1 if which == "convnet-train" else 0)
        assert (moved > 0) == (which == "convnet-train")         # n + 1 train-mode forwards moved the statistics; eval moved none

    class RaisesInTheSecondIteration(torch.nn.Module):
        def __init__(self, net):
            super().__init__()
            self.net, self.calls = net, 0

        def forward(self, v):
            self.calls += 1
            if self.calls == 2:
                raise RuntimeError("the model raised")
            return self.net(v)

    wrapped = RaisesInTheSecondIteration(a)
    with pytest.raises(RuntimeError, match="the model raised"):
        attacks.pgd(wrapped, x, y, eps=eps, alpha=eps / 5, n=N_ITER, transform=mel, noise=u)
    assert [p.requires_grad for p in a.parameters()] == flags and all(p.grad is None for p in a.parameters())


def test_the_loop_makes_no_host_read(dev):
    """after a warm-up call, a whole ``attacks.pgd`` (KWS in train(), the native loss head) under the sync debug mode "error"; the
    scripts' range assertion, the one host read, is left out by check_range=False"""
    m, mel, Kc = _kws(dev)
    x, u = _wave(3, 4000, 1)
    x, u = x.to(dev), u.to(dev)
    y = (torch.arange(3, device=dev) * 3 + 1) % Kc
    first = attacks.pgd(m, x, y, n=N_ITER, transform=mel, noise=u)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        again = attacks.pgd(m, x, y, n=N_ITER, transform=mel, noise=u, check_range=False)
        drawn = attacks.pgd(m, x, y, n=N_ITER, transform=mel, check_range=False)          # the default draw: torch.rand_like on the device
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert same_bits(first, again) and drawn.shape == x.shape
    with pytest.raises(AssertionError):
        attacks.pgd(m, 2.0 * x + 1.0, y, n=N_ITER, transform=mel, noise=u)
