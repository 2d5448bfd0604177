"""ap_psy.hip where its kernels branch: the PSD and the masker threshold on clips built to reach the first and last bin of the
maxima scan, a silent frame in a loud clip, one frame, plateaus, clips of very different loudness in one batch; the hinge loss
and its gradient at hops from 1 to 2048 with the hinge active in a fifth to four fifths of the cells; the refusals.

Both stages of ``ap_psy_threshold`` are read back from ``scratch`` (include/audiopure.h states the layout): the PSD against
tests/psy_restate.py's, and the threshold against the restatement fed THE GPU'S OWN PSD, so that every ``>`` of the masker
sees the same fp32 values on both sides.  tests/test_psy_cpu.py asserts on the CPU that the clips contain what they claim.

One-line defects these cases catch and the recorded clips at hop 512 do not: a maxima scan that starts at k = 2 or stops at
1022 (``end_bins``: the threshold moves by more than 3 dB); ``>=`` for ``>`` in the scan (``impulses``: plateaus); the clip
maximum taken over the batch (``loudness``); a gather that sums a fixed four frames, or whose ``flo`` is off by one only
where frames do not overlap (hops 2048, 700, 64, 1); ``thr_stab`` or ``psd_max_stab`` read without the clip index (B = 2 with
the hinge active in a quarter to two thirds of the cells, against 0.5 % in the earlier random case)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psy_restate as R  # noqa: E402
from audiopure_amd import _native as N  # noqa: E402
from audiopure_amd.robustness_eval import psychoacoustic as P  # noqa: E402

pytestmark = pytest.mark.gpu
NB = 1025


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _threshold(dev, x, hop):
    """ap_psy_threshold through ctypes on x [B, L] with a NaN-filled scratch of the advertised size: every output and both
    stages left in scratch, as numpy."""
    x = torch.from_numpy(np.atleast_2d(x)).to(dev).contiguous()
    B, L = x.shape
    F = 1 + (L - 2048) // hop
    lib = N.lib()
    m = P.PsychoacousticMasker(hop_size=hop)
    n = lib.ap_psy_scratch_elems(2048, hop, B, L)
    assert n >= B * F * (NB + 1)
    scratch = torch.full((n,), float("nan"), device=dev)
    thr = torch.full((B, NB, F), float("nan"), device=dev)
    thr_db = torch.full((B, NB, F), float("nan"), device=dev)
    pm = torch.full((B,), float("nan"), device=dev)
    pm_db = torch.full((B,), float("nan"), device=dev)
    N.check(lib.ap_psy_threshold(N.ptr(x), m.tables(dev).data_ptr(), N.ptr(thr), N.ptr(thr_db), N.ptr(pm), N.ptr(pm_db),
                                 N.ptr(scratch), 2048, hop, B, L, N.stream()), "ap_psy_threshold")
    torch.cuda.synchronize()
    s = scratch.cpu().numpy()
    assert not np.isnan(s[:B * F * (NB + 1)]).any() and np.isnan(s[B * F * (NB + 1):]).all()    # the stated layout, no more
    return dict(thr=thr.cpu().numpy(), thr_db=thr_db.cpu().numpy(), pm=pm.cpu().numpy(), pm_db=pm_db.cpu().numpy(),
                psd=s[:B * F * NB].reshape(B, F, NB), fmax=s[B * F * NB:B * F * (NB + 1)].reshape(B, F), masker=m)


def _check_stage_2(out, b=0):
    """thr_db / thr_stab / psd_max of clip b against the restatement on the PSD the GPU wrote (tolerances: test_gpu_psy.py)."""
    m = out["masker"]
    want, mx = R.threshold_from_psd(out["psd"][b], m.bark, m.absolute_threshold_hearing)
    db, stab = out["thr_db"][b], out["thr"][b]
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(db), fin) and np.all(db[~fin] == want[~fin])
    assert np.abs(db[fin] - want[fin]).max() <= 1e-3
    want_stab, want_pstab = R.stabilised(want, mx)
    assert np.array_equal(stab == 0, want_stab == 0)
    nz = want_stab != 0
    assert np.abs(stab[nz] / want_stab[nz] - 1).max() <= 2e-4
    assert abs(float(out["pm_db"][b]) - float(mx)) <= 1e-5
    assert abs(float(out["pm"][b]) / float(want_pstab) - 1) <= 2e-5
    return want


@pytest.fixture(scope="module")
def clips():
    return R.edge_clips()


@pytest.mark.parametrize("name", ("noise", "one_frame", "hop2048", "hop700", "quiet"))
def test_psd_of_white_noise_within_1e_4_db(dev, clips, name):
    """Stage 1.  Tolerance 1e-4 dB absolute: the two fp64 FFTs differ near 1e-15 of the frame peak; what remains is one fp32
    rounding of each complex64 component (below 1e-6 dB) and the fp32 rounding of a dB value of magnitude <= 200 (ulp 1.5e-5)."""
    x, hop = clips[name]
    out = _threshold(dev, x, hop)
    want = R.psd_db(x, hop)[0].T
    assert out["psd"].shape == (1,) + want.shape and want.min() > want.max() - 120
    err = np.abs(out["psd"][0].astype(np.float64) - want).max()
    print(f"psd {name}: max |d| = {err:.3e} dB")
    assert err <= 1e-4
    assert np.array_equal(out["fmax"][0], out["psd"][0].max(axis=1))
    _check_stage_2(out)


@pytest.mark.parametrize("name", ("silent_middle", "end_bins", "impulses", "constant"))
def test_threshold_on_clips_that_reach_the_scan_edges(dev, clips, name):
    x, hop = clips[name]
    out = _threshold(dev, x, hop)
    m = out["masker"]
    psd = out["psd"][0]
    assert np.array_equal(out["fmax"][0], psd.max(axis=1)) and not np.isnan(psd).any()
    pn, _ = R.normalised(psd)
    maskers = [R.frame_maskers(pn[f], m.bark, m.absolute_threshold_hearing) for f in range(len(pn))]
    want = _check_stage_2(out)
    if name == "silent_middle":                     # exactly-zero frame: -200 in every bin, M = 0, threshold = ATH
        assert np.all(psd[5] == -200.0) and len(maskers[5][0]) == 0 and all(len(maskers[f][0]) > 0 for f in range(5))
        assert np.isneginf(out["thr_db"][0][:3, 5]).all() and np.all(out["thr"][0][:3, 5] == 0)
        ath = m.absolute_threshold_hearing[3:]
        assert np.abs(out["thr_db"][0][3:, 5] - ath).max() <= 1e-3
        assert np.isfinite(out["thr_db"][0][:, :5]).all()
    if name == "end_bins":                          # on the GPU's own PSD too: bins 1 and 1023 are maskers, and they are kept
        for f in range(3):
            first, kept, _ = maskers[f]
            assert first[0] == 1 and first[-1] == 1023 and kept[0] == 1 and kept[-1] == 1023
        # without the masker at bin 1 or at bin 1023 (a scan from k = 2, or one that stops at 1022) the threshold of frame 0
        # would be another one by several dB, against the 1e-3 dB asserted above
        for k, flat, seen in ((1, 0, slice(3, 40)), (1023, 1024, slice(900, 1025))):
            p0 = pn[0].copy()
            p0[k] = p0[flat]
            other = R.frame_threshold(p0, m.bark, m.absolute_threshold_hearing)
            assert np.abs(other[seen] - want[seen, 0]).max() > 3.0
    if name == "impulses":                          # flat rows: silent frames and plateaus, where > and >= differ
        assert np.all(psd[2:4] == -200.0)
        strict = sum(len(R.frame_maskers(pn[f], m.bark, np.full(NB, -np.inf))[0]) for f in (0, 1, 4, 5))
        loose = sum(int((pn[f][1:-1] >= np.maximum(pn[f][:-2], pn[f][2:])).sum()) for f in (0, 1, 4, 5))
        assert strict < loose
    if name == "constant":
        assert np.all(psd[:, 2:] == -200.0) and all(len(mk[0]) == 0 for mk in maskers)


def test_clips_of_very_different_loudness_in_one_batch(dev):
    x = R.loudness_batch()
    out = _threshold(dev, x, 512)
    assert out["pm_db"][0] - out["pm_db"][2] > 10 and out["pm_db"][2] - out["pm_db"][1] > 40
    assert np.all(out["psd"][2, 5] == -200.0)
    for b in range(3):
        _check_stage_2(out, b)
        alone = _threshold(dev, x[b], 512)
        for k in ("thr", "thr_db", "pm", "pm_db", "psd", "fmax"):
            assert np.array_equal(out[k][b], alone[k][0], equal_nan=True), (b, k)


# ---- hinge loss and gradient ----------------------------------------------------------------------------------------
def _loss_grad(dev, delta, thr, pm, hop, guard=64):
    """ap_psy_loss_grad through ctypes: NaN-filled grad, loss and scratch, a guard after grad that must stay NaN."""
    delta = torch.as_tensor(delta).to(dev).contiguous()
    thr = torch.as_tensor(thr).to(dev).contiguous()
    pm = torch.as_tensor(pm).to(dev).contiguous()
    B, L = delta.shape
    assert tuple(thr.shape) == (B, NB, 1 + (L - 2048) // hop) and tuple(pm.shape) == (B,)
    lib = N.lib()
    scratch = torch.full((lib.ap_psy_scratch_elems(2048, hop, B, L),), float("nan"), device=dev)
    grad = torch.full((B * L + guard,), float("nan"), device=dev)
    loss = torch.full((B + 1,), float("nan"), device=dev)
    N.check(lib.ap_psy_loss_grad(N.ptr(delta), N.ptr(thr), N.ptr(pm), N.ptr(grad), N.ptr(loss), N.ptr(scratch), 2048, hop, B,
                                 L, N.stream()), "ap_psy_loss_grad")
    torch.cuda.synchronize()
    assert torch.isnan(grad[B * L:]).all() and torch.isnan(loss[B:]).all()
    return loss[:B].cpu().numpy(), grad[:B * L].view(B, L).cpu().numpy()


@pytest.mark.parametrize("times_sd", (1, 2))
@pytest.mark.parametrize("hop,L", R.LOSS_CASES)
def test_loss_and_gradient_against_fp64_autograd_at_every_hop(dev, hop, L, times_sd):
    """B = 2, thresholds from the native masker on each clip.  The gather's frame range is the only place the hop decides
    which scratch rows a sample sums: hop 2048 (no overlap), hops that do not divide L - 2048, hop 1, one frame, and an L
    that does not fill the last 256-thread block."""
    x, delta = R.loss_case(hop, L, times_sd)
    F = 1 + (L - 2048) // hop
    thr, pm = P.PsychoacousticMasker(hop_size=hop).threshold_and_psd_maximum(torch.from_numpy(x).to(dev))
    thr_h, pm_h = thr.cpu().numpy(), pm.cpu().numpy()
    assert thr_h.shape == (2, NB, F) and pm_h[0] != pm_h[1]
    share = R.active_share(delta, thr_h, pm_h, hop)
    print(f"hop {hop} L {L} x{times_sd}: active share {share}")
    assert np.all(share >= 0.2) and np.all(share <= 0.8)
    loss, grad = _loss_grad(dev, delta, thr, pm, hop)
    want_l, want_g = R.loss_and_grad(delta, thr_h, pm_h, hop)
    print("  loss rel", np.abs(loss / want_l - 1), " grad rel", [np.abs(grad[b] - want_g[b]).max() / np.abs(want_g[b]).max()
                                                                 for b in range(2)])
    assert np.abs(loss / want_l - 1).max() <= 1e-5
    for b in range(2):
        assert np.abs(grad[b] - want_g[b]).max() <= 1e-4 * np.abs(want_g[b]).max()
    end = (F - 1) * hop + 2048                      # samples past the last frame
    assert np.all(grad[:, end:] == 0.0) and np.all(want_g[:, end:] == 0.0)
    assert np.abs(grad[:, end - 8:end]).max() > 0
    # the same bits on a second call, and for clip 1 alone
    loss2, grad2 = _loss_grad(dev, delta, thr, pm, hop)
    assert np.array_equal(loss, loss2) and np.array_equal(grad, grad2)
    loss1, grad1 = _loss_grad(dev, delta[1:], thr[1:], pm[1:], hop)
    assert np.array_equal(loss[1:], loss1) and np.array_equal(grad[1:], grad1)


@pytest.mark.parametrize("hop,L", R.LOSS_CASES)
def test_zero_perturbation_and_zero_threshold(dev, hop, L):
    x, delta = R.loss_case(hop, L, 1)
    F = 1 + (L - 2048) // hop
    thr, pm = P.PsychoacousticMasker(hop_size=hop).threshold_and_psd_maximum(torch.from_numpy(x).to(dev))
    # all-zero delta: loss exactly 0, gradient exactly 0, no NaN (the reference's sqrt backward gives NaN there)
    loss, grad = _loss_grad(dev, np.zeros_like(delta), thr, pm, hop)
    assert np.all(loss == 0.0) and np.all(grad == 0.0)
    # a threshold of 0 everywhere: every non-zero bin is active, so the loss is the mean of P
    zero = torch.zeros_like(thr)
    loss, grad = _loss_grad(dev, delta, zero, pm, hop)
    pm_h = pm.cpu().numpy()
    Pw = R.power(delta, pm_h, hop)
    assert (Pw > 0).all() and Pw.shape == (2, NB, F)
    assert np.abs(loss / Pw.mean(axis=(1, 2)) - 1).max() <= 1e-5
    _, want_g = R.loss_and_grad(delta, np.zeros((2, NB, F)), pm_h, hop)
    for b in range(2):
        assert np.abs(grad[b] - want_g[b]).max() <= 1e-4 * np.abs(want_g[b]).max()


# ---- refusals -------------------------------------------------------------------------------------------------------
SENTINEL = -77.25


def test_refusals_return_22_and_leave_the_outputs_alone(dev):
    lib = N.lib()
    B, L, hop = 2, 2048 + 512, 512
    F = 2
    m = P.PsychoacousticMasker()
    x = torch.zeros(B, L, device=dev)
    tab = m.tables(dev)
    outs = dict(thr=torch.full((B, NB, F), SENTINEL, device=dev), thr_db=torch.full((B, NB, F), SENTINEL, device=dev),
                pm=torch.full((B,), SENTINEL, device=dev), pm_db=torch.full((B,), SENTINEL, device=dev),
                grad=torch.full((B, L), SENTINEL, device=dev), loss=torch.full((B,), SENTINEL, device=dev),
                scratch=torch.full((lib.ap_psy_scratch_elems(2048, hop, B, L),), SENTINEL, device=dev))

    def thr_args(**kw):
        a = dict(x=N.ptr(x), tab=tab.data_ptr(), thr=N.ptr(outs["thr"]), thr_db=N.ptr(outs["thr_db"]), pm=N.ptr(outs["pm"]),
                 pm_db=N.ptr(outs["pm_db"]), scratch=N.ptr(outs["scratch"]), window=2048, hop=hop, B=B, L=L)
        a.update(kw)
        return [a[k] for k in ("x", "tab", "thr", "thr_db", "pm", "pm_db", "scratch", "window", "hop", "B", "L")] + [N.stream()]

    def loss_args(**kw):
        a = dict(delta=N.ptr(x), thr=N.ptr(outs["thr"]), pm=N.ptr(outs["pm"]), grad=N.ptr(outs["grad"]),
                 loss=N.ptr(outs["loss"]), scratch=N.ptr(outs["scratch"]), window=2048, hop=hop, B=B, L=L)
        a.update(kw)
        return [a[k] for k in ("delta", "thr", "pm", "grad", "loss", "scratch", "window", "hop", "B", "L")] + [N.stream()]

    shapes = (dict(hop=0), dict(hop=2049), dict(L=2047), dict(window=1024), dict(B=0))
    for kw in shapes + tuple({k: None} for k in ("x", "tab", "thr", "pm", "scratch")):
        assert lib.ap_psy_threshold(*thr_args(**kw)) == -22, kw
        assert lib.ap_last_error()
    for kw in shapes + tuple({k: None} for k in ("delta", "thr", "pm", "grad", "loss", "scratch")):
        assert lib.ap_psy_loss_grad(*loss_args(**kw)) == -22, kw
        assert lib.ap_last_error()
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == SENTINEL).all()), k
    assert lib.ap_psy_scratch_elems(1024, hop, B, L) == 0 and lib.ap_psy_scratch_elems(2048, 0, B, L) == 0
    assert lib.ap_psy_scratch_elems(2048, hop, 0, L) == 0 and lib.ap_psy_scratch_elems(2048, hop, B, 2047) == 0
    # the optional outputs really are optional: NULL thr_db / psd_max_db is accepted and changes nothing else
    assert lib.ap_psy_threshold(*thr_args(thr_db=None, pm_db=None)) == 0
    torch.cuda.synchronize()
    assert bool((outs["thr_db"] == SENTINEL).all()) and bool((outs["pm_db"] == SENTINEL).all())
    assert not bool((outs["thr"] == SENTINEL).any()) and not bool((outs["pm"] == SENTINEL).any())
