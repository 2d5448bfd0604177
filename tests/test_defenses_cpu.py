"""Baseline defenses without a GPU: the numpy filter design and resampler taps against the reference's recorded outputs
(tests/golden/golden_defense_v1.npz, tests/golden/make_golden_defense.py) and direct float64 evaluation, the numpy
restatements the GPU tests use against the golden, ``lower_defender``, the scripts' import lines, and the C-ABI."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import defense_restate as R  # noqa: E402
from audiopure_amd.transforms import defense_design as D  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_defense_v1.npz")
DESIGNS = ("lpf_default", "lpf_a", "lpf_b", "bpf_default", "bpf_a")


@pytest.fixture(scope="module")
def G():
    return np.load(GOLDEN)


def _design(G, name):
    wp, ws = G[f"design/{name}/wp"], G[f"design/{name}/ws"]
    if wp.size == 1:
        wp, ws = float(wp[0]), float(ws[0])
    return wp, ws, ("low" if name.startswith("lpf") else "bandpass")


@pytest.mark.parametrize("name", DESIGNS)
def test_design_matches_the_recorded_scipy_design(G, name):
    wp, ws, bt = _design(G, name)
    N, Wn = D.buttord(wp, ws, 3, 40)
    assert N == int(G[f"design/{name}/N"])
    np.testing.assert_allclose(np.atleast_1d(Wn), G[f"design/{name}/Wn"], rtol=1e-13, atol=0)
    b, a = D.butter(N, Wn, bt)
    np.testing.assert_allclose(b, G[f"design/{name}/b"], rtol=1e-10, atol=1e-16)
    np.testing.assert_allclose(a, G[f"design/{name}/a"], rtol=1e-10, atol=1e-13)
    # what the kernels run: the fp32 cast, as frequency_defense.py:89-90 makes it
    assert np.array_equal(b.astype(np.float32), G[f"design/{name}/b"].astype(np.float32))
    assert np.array_equal(a.astype(np.float32), G[f"design/{name}/a"].astype(np.float32))


@pytest.mark.parametrize("name", DESIGNS)
def test_design_matches_scipy_when_installed(G, name):
    signal = pytest.importorskip("scipy.signal")
    wp, ws, bt = _design(G, name)
    N, Wn = D.buttord(wp, ws, 3, 40)
    Ns, Wns = signal.buttord(wp, ws, 3, 40)
    assert N == Ns and np.allclose(Wn, Wns, rtol=1e-13)
    b, a = D.butter(N, Wn, bt)
    bs, as_ = signal.butter(Ns, Wns, btype=bt)
    assert np.allclose(b, bs, rtol=1e-10, atol=1e-16) and np.allclose(a, as_, rtol=1e-10, atol=1e-13)


def test_default_designs_and_the_unstable_refusal():
    N, _, b, a = D.lpf_design()
    assert N == 1 and b.size == a.size == 2 and b.dtype == np.float32
    N, _, b, a = D.bpf_design()
    assert N == 3 and b.size == a.size == 7
    assert 0.94 < D.pole_radius(a) < 0.95
    with pytest.raises(ValueError, match=r"radius 1\.1"):
        D.lpf_design(wp=20, param=40)
    assert D.lpf_design(wp=5, param=2000)[0] == 1 and D.lpf_design(wp=8, param=400)[0] == 2


def test_resampler_taps_against_direct_float64_evaluation():
    kd, ku = D.ds_taps()
    assert kd.shape == (28,) and ku.shape == (2, 15) and kd.dtype == ku.dtype == np.float32

    def tap(t):                               # sinc * Hann^2 at the (rolloff-scaled, clamped) time t, by the formula
        t = min(max(t, -6.0), 6.0)
        s = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
        return s * math.cos(math.pi * t / 12) ** 2

    for j in range(28):                       # 16 k -> 8 k: orig 2, new 1, width ceil(12 / 0.99) = 13
        want = tap((j - 13) / 2 * 0.99) * 0.99 / 2
        assert abs(float(kd[j]) - want) <= 1e-7 * max(abs(want), 1e-3)
    for p in range(2):                        # 8 k -> 16 k: orig 1, new 2, width ceil(6 / 0.99) = 7
        for j in range(15):
            want = tap((-p / 2 + (j - 7)) * 0.99) * 0.99
            assert abs(float(ku[p, j]) - want) <= 1e-7 * max(abs(want), 1e-3)


@pytest.mark.parametrize("order_kind", ["lpf", "bpf", "long"])
def test_chunk_operators_against_direct_float64_evaluation(order_kind):
    a = {"lpf": D.lpf_design()[3], "bpf": D.bpf_design()[3], "long": D.lpf_design(wp=8, param=400)[3]}[order_kind]
    AC, H = D.chunk_operators(a, 128)
    A = D.state_matrix(a)
    n = A.shape[0]
    P = np.eye(n)
    for _ in range(128):
        P = P @ A
    np.testing.assert_allclose(AC, P, rtol=1e-9, atol=1e-11)
    # H[k] is the zero-input response: a unit state in slot i, run through the recurrence with zero input
    for i in range(n):
        s = np.zeros(n)
        s[i] = 1.0
        a64 = np.asarray(a, np.float64) / float(a[0])
        for k in range(128):
            y = s[0]
            assert abs(H[k, i] - y) <= 1e-9 * max(1.0, abs(y))
            s = np.append(s[1:], 0.0) - a64[1:] * y


def test_scan_hand_off_is_exact_in_float64():
    """The three passes of ap_iir_fwd in float64: chunk-wise zero-state filtering + A^C carry + H . S equals the
    sequential filter (so any error on the GPU is fp32 rounding, not a truncated warm-up)."""
    _, _, b, a = D.lpf_design(wp=8, param=400)             # pole 0.998: the tail spans thousands of samples
    rng = np.random.default_rng(0)
    x = rng.normal(0, 0.3, (2, 1000))
    AC, H = D.chunk_operators(a, 128)
    y = np.zeros_like(x)
    S = np.zeros((2, a.size - 1))
    for c0 in range(0, 1000, 128):
        blk = x[:, c0:c0 + 128]
        y0 = R.lfilter(b, a, np.pad(blk, ((0, 0), (0, 128 - blk.shape[1]))))
        y[:, c0:c0 + 128] = (y0 + S @ H.T)[:, :blk.shape[1]]
        e = _end_state(b, a, np.pad(blk, ((0, 0), (0, 128 - blk.shape[1]))))
        S = S @ AC.T + e
    np.testing.assert_allclose(y, R.lfilter(b, a, x), rtol=0, atol=1e-11)


def _end_state(b, a, x):
    b = np.asarray(b, np.float64) / float(a[0])
    a = np.asarray(a, np.float64) / float(a[0])
    n = a.size - 1
    z = np.zeros((x.shape[0], n))
    for t in range(x.shape[1]):
        u = x[:, t]
        yt = b[0] * u + z[:, 0]
        z = np.concatenate([z[:, 1:], np.zeros((x.shape[0], 1))], axis=1) + np.outer(u, b[1:]) - np.outer(yt, a[1:])
    return z


def test_restatements_match_the_golden(G):
    x, g, z = G["x"], G["g"], G["z"]
    np.testing.assert_allclose(R.as_fwd(x), G["AS/y"], atol=1e-6)
    np.testing.assert_allclose(R.as_fwd(g), G["AS/dx"], atol=1e-6)          # AS adjoint = AS
    v, off = R.ms_fwd(x)
    assert np.array_equal(v, G["MS/y"])
    np.testing.assert_allclose(R.ms_bwd(g, off), G["MS/dx"], atol=1e-6)
    assert np.array_equal(R.ms_fwd(G["xq"])[0], G["MSq/y"])
    np.testing.assert_allclose(R.at_fwd(x, z), G["AT/y"], atol=1e-6)
    np.testing.assert_allclose(R.at_bwd(x, z, g), G["AT/dx"], atol=1e-6)
    np.testing.assert_allclose(R.ds_fwd(x), G["DS/y"], atol=1e-6)
    np.testing.assert_allclose(R.ds_matrix(x.shape[1]).T @ g[0], G["DS/dx"][0], atol=1e-6)
    np.testing.assert_allclose(R.ds_fwd(G["xodd"], same_size=False), G["DSodd/y"], atol=1e-6)
    for kind, des in (("LPF", D.lpf_design()), ("BPF", D.bpf_design())):
        b, a = des[2], des[3]
        for tag, xi in (("", x), ("16", G["x16"]), ("mix", G["xmix"])):
            y, _ = R.filt_fwd(xi, b, a)
            scale = max(1.0, float(np.abs(xi).max()))
            np.testing.assert_allclose(y, G[f"{kind}{tag}/y"], atol=1e-6 * scale)
            np.testing.assert_allclose(R.filt_bwd(xi, g, b, a), G[f"{kind}{tag}/dx"], atol=1e-6)
    assert R.clip_range(G["xmix"]) == (-32768.0, 32767.0) and R.clip_range(x) == (-1.0, 1.0)


# ------------------------------------------------------------------------------------------------------- lowering
def _standin(module, name):
    cls = type(name, (), {"__init__": lambda self, t, *a: setattr(self, "defense_type", t), "__module__": module})
    return cls


@pytest.mark.parametrize("name,module,kind", [("TimeDomainDefense", "transforms.time_defense", "MS"),
                                              ("FreqDomainDefense", "transforms.frequency_defense", "BPF"),
                                              ("TimeDomainDefense", "AudioPure.transforms.time_defense", "AS")])
def test_lower_defender_maps_the_reference_classes(name, module, kind):
    from audiopure_amd.lowering import lower_defender
    from audiopure_amd.transforms import defenses
    nat = lower_defender(_standin(module, name)(kind))
    assert type(nat) is getattr(defenses, name) and nat.defense_type == kind
    assert lower_defender(nat) is nat


def test_lower_defender_leaves_everything_else_alone():
    from audiopure_amd.lowering import lower_defender
    other = _standin("mypkg.defenses", "TimeDomainDefense")("MS")          # same name, another module
    assert lower_defender(other) is other
    wrong = _standin("transforms.time_defense", "FreqDomainDefense")("DS")  # right name, the other module
    assert lower_defender(wrong) is wrong
    assert lower_defender(None) is None
    from audiopure_amd.diffusion_models.diffwave_sde import RevDiffWave
    rd = RevDiffWave.__new__(RevDiffWave)
    assert lower_defender(rd) is rd


def test_native_dispatch_names_and_refusals():
    from audiopure_amd.transforms import FreqDomainDefense, TimeDomainDefense
    assert [TimeDomainDefense(t)._get_name() for t in ("AT", "AS", "MS")] == \
        ["Audio_Turbulence", "Average_Smoothing", "Median_Smoothing"]
    assert [FreqDomainDefense(t)._get_name() for t in ("DS", "LPF", "BPF")] == \
        ["Down_Sampling", "Low_Pass_Filter", "Band_Pass_Filter"]
    with pytest.raises(NotImplementedError, match="Unknown defense type: QT!"):
        TimeDomainDefense("QT")(None)
    with pytest.raises(NotImplementedError, match="Unknown defense type: AS!"):
        FreqDomainDefense("AS")._get_name()


def test_cpu_tensors_raise():
    import torch
    from audiopure_amd import _native as N
    from audiopure_amd.transforms import defenses
    for fn in (defenses.AS, defenses.MS, defenses.AT, defenses.DS, defenses.LPF, defenses.BPF):
        with pytest.raises(N.NativeError, match="CPU"):
            fn(torch.zeros(2, 100))


def test_script_imports_give_an_acoustic_system_with_the_native_defender(tmp_path):
    """``from transforms.time_defense import *`` / ``from transforms.frequency_defense import *`` (adaptive_attack_eval.py:
    14-15) from a stand-in checkout whose transforms/__init__ imports librosa and whose frequency_defense imports
    torchaudio, scipy and torch_lfilter (stubbed, as test_dropin_cpu.py stubs them)."""
    import test_dropin_cpu as T
    base = T._standin_checkout(tmp_path)
    tr = os.path.join(base, "transforms")
    os.makedirs(tr, exist_ok=True)
    body = ("class {0}():\n    def __init__(self, defense_type, *args):\n        self.defense_type = defense_type\n"
            "    def __call__(self, x, *args):\n        raise RuntimeError('the reference defender ran')\n")
    with open(os.path.join(tr, "__init__.py"), "w") as f:
        f.write("import librosa\n")
    with open(os.path.join(tr, "time_defense.py"), "w") as f:
        f.write("import torch\n" + body.format("TimeDomainDefense"))
    with open(os.path.join(tr, "frequency_defense.py"), "w") as f:
        f.write("import torchaudio\nfrom scipy import signal\nfrom torch_lfilter import lfilter\n"
                + body.format("FreqDomainDefense"))
    out = T._run(T.SCRIPT_IMPORTS.replace('"statsmodels.stats.proportion"', '"statsmodels.stats.proportion", "torch_lfilter"')
                 + """
    from transforms.time_defense import *
    from transforms.frequency_defense import *
    for d in (TimeDomainDefense('MS'), FreqDomainDefense('BPF')):
        s = AcousticSystem(classifier=Classifier, transform=None, defender=d)
        assert type(s.defender).__module__ == "audiopure_amd.transforms.defenses", type(s.defender)
        assert s.defender.defense_type == d.defense_type
    print("DEFENDERS OK")
    """, checkout=base)
    assert "DEFENDERS OK" in out


# -------------------------------------------------------------------------------------------------------- C-ABI
NEW_SYMBOLS = ("ap_avg_smooth", "ap_median_smooth", "ap_median_smooth_bwd", "ap_at_fwd", "ap_at_bwd", "ap_ds_fwd",
               "ap_ds_bwd", "ap_iir_scratch_elems", "ap_iir_fwd", "ap_iir_bwd")


def test_defense_symbols_are_declared_bound_and_exported():
    from audiopure_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "audiopure.h")).read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\(([^;]*)\);", hdr)
        assert m, name
        nargs = len([p for p in m.group(1).split(",") if p.strip()])
        assert len(N.SIGNATURES[name][1]) == nargs, name
    lib = N.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.ap_iir_scratch_elems(7, 2, 300) == 2 * 300 + 2 * (2 * 3 * 6)   # fp32 y0, then fp64 states
    assert lib.ap_iir_scratch_elems(17, 2, 300) == 0


def test_host_side_refusals_need_no_device():
    from audiopure_amd import _native as N
    lib = N.lib()
    assert lib.ap_avg_smooth(1, 1, 4, 1, 10, None) == -22 and b"odd" in lib.ap_last_error()
    assert lib.ap_median_smooth(1, 1, 1, 65, 1, 10, None) == -22 and b"63" in lib.ap_last_error()
    assert lib.ap_median_smooth(None, 1, 1, 3, 1, 10, None) == -22 and b"NULL" in lib.ap_last_error()
    f = N.farr([1.0] * 17)
    d = (ctypes.c_double * 289)()
    assert lib.ap_iir_fwd(1, 1, 1, 1, f, f, 17, d, 1, 1, 16, 1, 10, None) == -22 and b"16" in lib.ap_last_error()
    assert lib.ap_iir_bwd(1, None, None, 1, f, f, 3, d, 1, None, 16, 1, 10, None) == -22 and b"scratch" in lib.ap_last_error()
    assert lib.ap_ds_fwd(1, 1, f, f, 1, 10, 7, None) == -22 and b"Lout" in lib.ap_last_error()
    assert lib.ap_at_fwd(1, 1, 1, 0.0, 1, 10, None) == -22 and b"snr" in lib.ap_last_error()
    assert lib.ap_avg_smooth(1, 1, 3, 1, 0, None) == -22
