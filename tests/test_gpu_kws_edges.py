"""The KWS route's kernels (ap_kws.hip: KWSModel forward and backward, HTK mel-dB forward and its two-pass backward) against
the float64 references of kws_restate.py, at the frame counts, widths, batch sizes and input levels where the kernels and
their launchers branch.  Every kernel writes into a NaN-filled buffer (the backward's scratch included), so an element it
leaves out, or reads before writing, fails the comparison; every refusal tested here is returned by the host code before any
launch.  The bounds are 8 x the float32 error of the restatement on these very cases, or the bound test_gpu_kws.py already
holds where that is tighter (kws_restate.py); the case tables and the conditions on the inputs are asserted by
test_kws_restate_cpu.py."""
import ctypes as C
import functools

import pytest
import torch

import kws_restate as R
from audiopure_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def nan_like(shape, dev):
    return torch.full(shape, float("nan"), device=dev, dtype=torch.float32)


# ---- classifier ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(shape):
    from audiopure_amd.audio_models.RCNN_KWS import KWSModel
    n_mels, H, Kc = shape
    m = KWSModel(in_size=n_mels, hidden_size=H, num_classes=Kc)
    m.load_state_dict(R.kws_weights(*shape))
    return m.to(torch.device("cuda:0")).eval()


def _fwd(m, xd, out):
    """xd [B,n_mels,T] -> out [B,K]"""
    return N.lib().ap_kws_fwd(m._handle(), N.ptr(xd), N.ptr(out), xd.shape[0], xd.shape[2], N.stream())


def _bwd(m, xd, vd, dx):
    """into dx [B,n_mels,T]; the scratch is NaN-filled as well: the kernel must write each save before it reads it"""
    B, _, T = xd.shape
    n = N.lib().ap_kws_bwd_scratch_elems(m._handle(), B, T)
    assert n > 0
    return N.lib().ap_kws_bwd(m._handle(), N.ptr(xd), N.ptr(vd), N.ptr(dx), N.ptr(nan_like((n,), xd.device)), B, T, N.stream())


def _check_kws_gradient(case, dx):
    """dx [B,n_mels,T] on the device against float64 autograd: per clip to KWS_GRAD_BOUND of the clip's largest entry, and
    exactly 0 in every column the model does not read (with one class: everywhere)."""
    n_mels, H, Kc, T, B = case
    _, ref = R.kws_reference(*case)
    got = dx.cpu().double()
    if Kc == 1:
        assert bool((got == 0.0).all())
        return
    err = R.per_clip_rel_err(got, ref)
    print(f"kws gradient {case}: per-clip max |d| / max |ref| up to {float(err.max()):.2e} (bound {R.KWS_GRAD_BOUND:.1e})")
    assert bool(torch.isfinite(got).all()) and float(err.max()) <= R.KWS_GRAD_BOUND, err.tolist()
    assert bool((got[:, :, ~R.kws_read_columns(T)] == 0.0).all())


@pytest.mark.parametrize("case", R.KWS_CASES, ids=lambda c: "-".join(map(str, c)))
def test_kws_forward_and_input_gradient_match_float64(dev, case):
    """T = 5, 6: one GRU step, softmax over one step, an unread last column; 19, 20 / 21: the second step appears; 37: the
    third; 672 (436, 440, 1940): the last clip the forward's LDS holds.  (20, 128, 64) fills the backward's static arrays,
    (60, 96, 12) has three pointwise groups, (32, 8, 1) one class.  One workgroup per clip: a row is its clip's alone."""
    n_mels, H, Kc, T, B = case
    m = _model(case[:3])
    ref, _ = R.kws_reference(*case)
    xd, vd = R.kws_mel(n_mels, T, B)[:, 0].contiguous().to(dev), R.kws_cotangent(n_mels, T, B, Kc).to(dev)
    out = nan_like((B, Kc), dev)
    N.check(_fwd(m, xd, out), "ap_kws_fwd")
    err = float((out.cpu().double() - ref).abs().max())
    print(f"kws forward {case}: max |d logp| = {err:.2e} (bound {R.KWS_LOGP_BOUND:.1e})")
    assert err <= (0.0 if Kc == 1 else R.KWS_LOGP_BOUND)                       # (NaN fails)
    again, rows = nan_like((B, Kc), dev), nan_like((B, Kc), dev)
    N.check(_fwd(m, xd, again), "ap_kws_fwd")
    for i in range(B):
        N.check(_fwd(m, xd[i:i + 1], rows[i:i + 1]), "ap_kws_fwd")
    assert torch.equal(again, out) and torch.equal(rows, out)

    dx = nan_like((B, n_mels, T), dev)
    N.check(_bwd(m, xd, vd, dx), "ap_kws_bwd")
    _check_kws_gradient(case, dx)
    again, rows = nan_like((B, n_mels, T), dev), nan_like((B, n_mels, T), dev)
    N.check(_bwd(m, xd, vd, again), "ap_kws_bwd")
    for i in range(B):
        N.check(_bwd(m, xd[i:i + 1], vd[i:i + 1], rows[i:i + 1]), "ap_kws_bwd")
    assert torch.equal(again, dx) and torch.equal(rows, dx)


@pytest.mark.parametrize("case", R.KWS_BWD_ONLY_CASES, ids=lambda c: "-".join(map(str, c)))
def test_kws_backward_runs_past_the_forwards_lds_limit(dev, case):
    """ap_kws_bwd keeps its state in global scratch; through the module the forward refuses first."""
    n_mels, H, Kc, T, B = case
    m = _model(case[:3])
    x = R.kws_mel(n_mels, T, B)
    xd, vd = x[:, 0].contiguous().to(dev), R.kws_cotangent(n_mels, T, B, Kc).to(dev)
    dx = nan_like((B, n_mels, T), dev)
    N.check(_bwd(m, xd, vd, dx), "ap_kws_bwd")
    _check_kws_gradient(case, dx)
    with pytest.raises(N.NativeError, match=f"{T} mel frames need {R.kws_fwd_lds_bytes(n_mels, H, Kc, T)} bytes of LDS"):
        m(x.to(dev).requires_grad_(True))


def test_kws_module_surface(dev):
    """[B,1,n_mels,T] and [B,n_mels,T], a strided view and its contiguous copy, with and without a gradient: the same bits,
    which are the C entry points' bits; no clips give an empty result."""
    case = R.GOLDEN_SHAPE + (81, 8)
    n_mels, H, Kc, T, B = case
    m = _model(case[:3])
    x4, vd = R.kws_mel(n_mels, T, B).to(dev), R.kws_cotangent(n_mels, T, B, Kc).to(dev)
    x3 = x4[:, 0].contiguous()
    out, dx = nan_like((B, Kc), dev), nan_like((B, n_mels, T), dev)
    N.check(_fwd(m, x3, out), "ap_kws_fwd")
    N.check(_bwd(m, x3, vd, dx), "ap_kws_bwd")
    wide = torch.zeros((B, n_mels, 2 * T), device=dev)
    wide[:, :, ::2] = x3
    assert not wide[:, :, ::2].is_contiguous()
    with torch.no_grad():
        for xin in (x4, x3, wide[:, :, ::2], wide[:, None, :, ::2]):
            assert torch.equal(m(xin), out)
    for xin in (x4, x3):
        xg = xin.clone().requires_grad_(True)
        lp = m(xg)
        (g,) = torch.autograd.grad(lp, xg, vd)
        assert torch.equal(lp.detach(), out) and g.shape == xin.shape and torch.equal(g.reshape(dx.shape), dx)
    wg = wide.clone().requires_grad_(True)
    lp = m(wg[:, :, ::2])
    (g,) = torch.autograd.grad(lp, wg, vd)
    assert torch.equal(lp.detach(), out) and torch.equal(g[:, :, ::2], dx) and bool((g[:, :, 1::2] == 0.0).all())
    for grad in (False, True):
        empty = m(torch.empty((0, 1, n_mels, T), device=dev, requires_grad=grad))
        assert empty.shape == (0, Kc) and empty.dtype == torch.float32


# ---- HTK mel-dB front-end -------------------------------------------------------------------------------------------------
def _htk_fwd(xd, out, n_mels):
    """xd [B,L] -> out [B,n_mels,1 + L // 200]"""
    return N.lib().ap_melspec_db_htk(N.ptr(xd), N.ptr(out), n_mels, xd.shape[0], xd.shape[1], N.stream())


def _htk_bwd(xd, vd, dx, n_mels):
    B, L = xd.shape
    scratch = nan_like((B * (1 + L // 200) * 400,), xd.device)
    return N.lib().ap_melspec_db_htk_bwd(N.ptr(xd), N.ptr(vd), N.ptr(dx), N.ptr(scratch), n_mels, B, L, N.stream())


def _check_htk(dev, x, n_mels, tag):
    """Forward and backward of x [B,L] into NaN-filled buffers against float64: dB to HTK_DB_BOUND, the gradient per sample to
    HTK_GRAD_BOUND of the largest reference gradient within +-400 samples (where that is 0, exactly); two launches give equal
    bits and a clip's rows do not depend on the clips launched with it.  Returns (dB, dx, reference mel power)."""
    from audiopure_amd.transforms import MelSpecDBHTK
    B, L = x.shape
    frames = 1 + L // 200
    v = R.htk_cotangent(tag, B, n_mels, L)
    ref_db, mel, ref_g = R.htk_reference(x, n_mels, v)
    xd, vd = x.to(dev), v.to(dev)
    out, dx = nan_like((B, n_mels, frames), dev), nan_like((B, L), dev)
    N.check(_htk_fwd(xd, out, n_mels), "ap_melspec_db_htk")
    N.check(_htk_bwd(xd, vd, dx, n_mels), "ap_melspec_db_htk_bwd")
    err = float((out.cpu().double() - ref_db).abs().max())
    d, scale = (dx.cpu().double() - ref_g).abs(), R.htk_local_scale(ref_g)
    worst = float((d / scale.clamp(min=1e-300))[scale > 0].max()) if bool((scale > 0).any()) else 0.0
    print(f"htk mel {tag} n_mels={n_mels} B={B}: max |d dB| = {err:.2e} (bound {R.HTK_DB_BOUND:.1e}), "
          f"max |d grad| / local max |ref| = {worst:.2e} (bound {R.HTK_GRAD_BOUND:.1e})")
    assert err <= R.HTK_DB_BOUND                                               # (NaN fails)
    assert bool(torch.isfinite(dx).all()) and float((d - R.HTK_GRAD_BOUND * scale).max()) <= 0.0, worst
    out2, dx2 = nan_like(tuple(out.shape), dev), nan_like(tuple(dx.shape), dev)
    N.check(_htk_fwd(xd, out2, n_mels), "ap_melspec_db_htk")
    N.check(_htk_bwd(xd, vd, dx2, n_mels), "ap_melspec_db_htk_bwd")
    assert torch.equal(out2, out) and torch.equal(dx2, dx)
    out1, dx1 = nan_like(tuple(out.shape), dev), nan_like(tuple(dx.shape), dev)
    for i in range(B):
        N.check(_htk_fwd(xd[i:i + 1], out1[i:i + 1], n_mels), "ap_melspec_db_htk")
        N.check(_htk_bwd(xd[i:i + 1], vd[i:i + 1], dx1[i:i + 1], n_mels), "ap_melspec_db_htk_bwd")
    assert torch.equal(out1, out) and torch.equal(dx1, dx)
    # the module: the same kernels on [B,1,L], with and without a gradient
    mod = MelSpecDBHTK(n_mels)
    with torch.no_grad():
        assert torch.equal(mod(xd[:, None]), out[:, None])
    xg = xd[:, None].clone().requires_grad_(True)
    y = mod(xg)
    (g,) = torch.autograd.grad(y, xg, vd[:, None])
    assert torch.equal(y.detach(), out[:, None]) and torch.equal(g[:, 0], dx)
    return out.cpu(), dx.cpu(), mel


@pytest.mark.parametrize("L,n_mels,B", R.HTK_CASES)
def test_htk_mel_forward_and_gradient_match_float64(dev, L, n_mels, B):
    """201: the smallest clip, both reflections on the same samples; 202, 399: the reflections overlap inside a frame; 400,
    600 / 401, 601 / 399, 599: the frame count steps; 1 and 64 filters: the fewest and the most the kernel holds."""
    _check_htk(dev, R.htk_noise(B, L), n_mels, L)


@pytest.mark.parametrize("n_mels", R.HTK_MELS)
def test_htk_mel_on_loud_quiet_and_silent_stretches(dev, n_mels):
    """A frame that reads zeros only (reflections included) is under the 1e-10 clamp: exactly -100 dB in every filter, and an
    exactly zero gradient on every sample only such frames read -- the whole of the all-zero clip.  The gradient scales as
    1 / power, 1e6 times larger in the quiet stretch than in the loud one, which only the local scale looks at."""
    x = R.htk_stretch_clips()
    out, dx, mel = _check_htk(dev, x, n_mels, "s")
    silent = R.htk_silent_frames(mel)
    assert int(silent.sum()) == 6 + 2 + 13
    assert bool((out.transpose(1, 2)[silent] == -100.0).all())
    zero = R.htk_silent_samples(mel, x.shape[1])
    assert zero.sum(dim=1).tolist() == [801, 201, 2400]
    assert bool((dx[zero] == 0.0).all()) and bool((dx[~zero] != 0.0).any())


# ---- refusals: host checks that precede every launch -------------------------------------------------------------------------
def _refused(rc, text):
    assert rc == -22
    with pytest.raises(N.NativeError, match=text):
        N.check(rc, "call")


def test_kws_launch_refusals_leave_the_outputs_alone(dev):
    m = _model(R.GOLDEN_SHAPE)
    for T, text in ((4, "4 mel frames are too few for the separable conv"), (673, "673 mel frames need 163864 bytes of LDS")):
        xd, out = R.kws_mel(40, T, 2)[:, 0].contiguous().to(dev), nan_like((2, 4), dev)
        _refused(_fwd(m, xd, out), "ap_kws_fwd: " + text)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
    assert N.lib().ap_kws_bwd_scratch_elems(m._handle(), 2, 4) == 0
    assert N.lib().ap_kws_bwd_scratch_elems(m._handle(), 2, 5) > 0
    xd, vd = R.kws_mel(40, 4, 2)[:, 0].contiguous().to(dev), R.kws_cotangent(40, 4, 2, 4).to(dev)
    dx, scratch = nan_like((2, 40, 4), dev), nan_like((4096,), dev)
    _refused(N.lib().ap_kws_bwd(m._handle(), N.ptr(xd), N.ptr(vd), N.ptr(dx), N.ptr(scratch), 2, 4, N.stream()),
             "ap_kws_bwd: 4 mel frames are too few for the separable conv")
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(scratch).all())


@pytest.mark.parametrize("n_mels,H,Kc", [(64, 64, 4), (45, 64, 4), (65, 64, 4), (0, 64, 4), (40, 129, 4), (60, 64, 4), (40, 64, 65)])
def test_kws_create_refuses_shapes_it_does_not_hold(dev, n_mels, H, Kc):
    """n_mels 64 and 45 are not divisible by their n_mels // 20 groups, hidden 64 not by the 3 groups of 60 mels; 65 / 129 / 65
    are past the kernels' static limits."""
    blob, h = torch.zeros(max(1, N.lib().ap_kws_blob_elems(n_mels, H, Kc)), device=dev), C.c_void_p()
    _refused(N.lib().ap_kws_create(n_mels, H, Kc, N.ptr(blob), blob.numel(), N.stream(), C.byref(h)),
             r"ap_kws_create: unsupported shape \(n_mels <= 64, hidden <= 128, num_classes <= 64\)")
    assert h.value is None


def test_kws_create_refuses_a_short_blob(dev):
    n = N.lib().ap_kws_blob_elems(*R.GOLDEN_SHAPE)
    assert n == sum(v.numel() for v in R.kws_weights(*R.GOLDEN_SHAPE).values())
    blob, h = torch.zeros(n, device=dev), C.c_void_p()
    _refused(N.lib().ap_kws_create(*R.GOLDEN_SHAPE, N.ptr(blob), n - 1, N.stream(), C.byref(h)),
             f"ap_kws_create: blob has {n - 1} elements, expected {n}")
    assert h.value is None


@pytest.mark.parametrize("L,n_mels,text", [(200, 40, "bad argument"), (1000, 0, r"n_mels 0 outside \[1, 64\]"),
                                           (1000, 65, r"n_mels 65 outside \[1, 64\]")])
def test_htk_mel_refusals_leave_the_outputs_alone(dev, L, n_mels, text):
    xd = R.htk_noise(2, L).to(dev)
    frames = 1 + L // 200
    out, dx = nan_like((2, max(n_mels, 1), frames), dev), nan_like((2, L), dev)
    vd, scratch = torch.ones((2, max(n_mels, 1), frames), device=dev), nan_like((2 * frames * 400,), dev)
    _refused(_htk_fwd(xd, out, n_mels), "ap_melspec_db_htk: " + text)
    _refused(N.lib().ap_melspec_db_htk_bwd(N.ptr(xd), N.ptr(vd), N.ptr(dx), N.ptr(scratch), n_mels, 2, L, N.stream()),
             "ap_melspec_db_htk_bwd: " + text)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(dx).all()) and bool(torch.isnan(scratch).all())
