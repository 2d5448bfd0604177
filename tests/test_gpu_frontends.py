"""M5 (ap_frontend.hip) and the Slaney mel-dB front-end (ap_mel.hip) against the float64 restatements of
frontend_restate.py, at the lengths, widths and input levels where the kernels and their launchers branch.  Every kernel
writes into a NaN-filled buffer, so an element it leaves out fails the comparison; every refusal tested here is returned by
the host code before any launch.  The conditions on the inputs are asserted by test_frontend_restate_cpu.py."""
import functools

import numpy as np
import pytest
import torch

import frontend_restate as R
from audiopure_amd import _native as N

pytestmark = pytest.mark.gpu

M5_ATOL = 2e-5                       # log-probabilities, the bound of test_m5_matches_oracle
# decided clips: 8 x the error of float32 CPU autograd of the restatement against float64 on the same clips (measured:
# 3.3e-7 at most over the seven cases, per clip, max |d| / max |ref|); the factor covers the kernel's other summation order
# (80- and 192-term FMA chains, BatchNorm folded into the weights)
M5_GRAD_DECIDED = 8 * 3.3e-7
MEL_ATOL = 5e-3                      # dB, the bound of test_melspec_matches_oracle
MEL_GRAD_LOCAL = 2e-4                # of the largest reference gradient within +-2048 samples


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def nan_like(shape, dev):
    return torch.full(shape, float("nan"), device=dev, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _m5_module(nc, no):
    from audiopure_amd.audio_models.M5.M5Net import M5
    m5 = M5(n_input=1, n_output=no, n_channel=nc)
    m5.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in R.m5_weights(no, nc).items()})
    return m5.to(torch.device("cuda:0")).eval()


def _m5_fwd(m5, xd, out):
    return N.lib().ap_m5_fwd(m5._handle(), N.ptr(xd), N.ptr(out), xd.shape[0], xd.shape[2], N.stream())


def _m5_bwd(m5, xd, vd, dx):
    return N.lib().ap_m5_bwd(m5._handle(), N.ptr(xd), N.ptr(vd), N.ptr(dx), xd.shape[0], xd.shape[2], N.stream())


@pytest.mark.parametrize("L,nc,no", R.M5_FWD_CASES)
def test_m5_forward_matches_float64(dev, L, nc, no):
    """6848: Q4 = 1; 16016 / 16037: conv-1 windows dropped by the pooling, unread tail; 32000 / 48000 (and 16400 at 64
    channels): the clip is read from global memory instead of LDS; 16000 at 64 channels: 152 832 B, staged."""
    m5, x = _m5_module(nc, no), R.m5_clips(8, L)
    ref, _ = R.m5_forward(R.m5_weights(no, nc), x.double())
    xd, out = x.to(dev), nan_like((8, no), dev)
    N.check(_m5_fwd(m5, xd, out), "ap_m5_fwd")
    err = float((out.cpu().double() - ref).abs().max())
    print(f"m5 forward L={L} nc={nc} n_out={no}: max |d logp| = {err:.2e}")
    assert err <= M5_ATOL                                                    # (NaN fails)
    for i in range(8):                                                       # one workgroup per clip: a row is its clip's alone
        one = nan_like((1, no), dev)
        N.check(_m5_fwd(m5, xd[i:i + 1].contiguous(), one), "ap_m5_fwd")
        assert torch.equal(one[0], out[i]), i


@pytest.mark.parametrize("B", [1, 300])
def test_m5_forward_at_one_clip_and_at_more_clips_than_compute_units(dev, B):
    m5, x = _m5_module(32, 10), R.m5_clips(B, 8000)
    ref, _ = R.m5_forward(R.m5_weights(10, 32), x.double())
    out = nan_like((B, 10), dev)
    N.check(_m5_fwd(m5, x.to(dev), out), "ap_m5_fwd")
    assert float((out.cpu().double() - ref).abs().max()) <= M5_ATOL


@pytest.mark.parametrize("L,nc,text", [(6847, 32, "too short for four conv/pool stages"), (64000, 32, "needs 179456 bytes of LDS"),
                                       (79, 32, "shorter than the first kernel 80")])
def test_m5_forward_refusals_leave_the_output_alone(dev, L, nc, text):
    m5 = _m5_module(nc, 10)
    xd, out = R.m5_clips(2, L).to(dev), nan_like((2, 10), dev)
    with pytest.raises(N.NativeError, match=text):
        N.check(_m5_fwd(m5, xd, out), "ap_m5_fwd")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@functools.lru_cache(maxsize=None)
def _m5_grad_reference(L, nc):
    no = 64 if nc == 64 else 10
    x, v = R.m5_clips(8, L), R.m5_cotangent(8, no)
    xr = x.double().requires_grad_(True)
    lp, pre = R.m5_forward(R.m5_weights(no, nc), xr)
    (g,) = torch.autograd.grad(lp, xr, v.double())
    return no, x, v, g, R.m5_decided(pre, R.M5_TAU)


@pytest.mark.parametrize("L,nc", R.M5_GRAD_CASES)
def test_m5_input_gradient_matches_float64_autograd(dev, L, nc):
    """Clips whose pooling and ReLU selections are decided (frontend_restate.m5_decided, tau = 7e-6: 6, 6, 6, 6, 6, 4 and 4 of
    8) must agree with float64 autograd to 2.6e-6 of the clip's largest entry; the others keep the earlier bound, under which
    a selection may flip at isolated samples."""
    no, x, v, ref, decided = _m5_grad_reference(L, nc)
    assert int(decided.sum()) >= R.M5_MIN_DECIDED
    m5 = _m5_module(nc, no)
    xd, vd, dx = x.to(dev), v.to(dev), nan_like(tuple(x.shape), dev)
    N.check(_m5_bwd(m5, xd, vd, dx), "ap_m5_bwd")
    got = dx.cpu().double()
    errs = R.m5_gradient_errors(got, ref)
    print(f"m5 gradient L={L} nc={nc}: decided {decided.tolist()} per-clip max|d|/max|ref| {[f'{e:.1e}' for e in errs[0]]}")
    R.assert_m5_gradient(got, ref, decided, M5_GRAD_DECIDED)
    if L == 16037:
        assert bool((dx[..., 16000:] == 0.0).all())                          # nothing that survives the pooling reads the tail
    # the module's autograd route: the same kernel, and a forward value that is the no-grad forward's
    xg = xd.clone().requires_grad_(True)
    lp = m5(xg)
    (g,) = torch.autograd.grad(lp, xg, vd)
    with torch.no_grad():
        assert torch.equal(lp.detach(), m5(xd))
    assert torch.equal(g, dx)


@pytest.mark.parametrize("L,nc,nbytes", [(48000, 32, 168608), (24000, 64, 167744)])
def test_m5_backward_refuses_what_its_lds_cannot_hold(dev, L, nc, nbytes):
    """The forward serves both lengths (134 784 and 134 144 B); the backward keeps a selection byte per activation on top."""
    no = 64 if nc == 64 else 10
    m5 = _m5_module(nc, no)
    xd, vd, dx = R.m5_clips(2, L).to(dev), R.m5_cotangent(2, no).to(dev), nan_like((2, 1, L), dev)
    with pytest.raises(N.NativeError, match=f"m5 backward: clip length {L} needs {nbytes} bytes of LDS"):
        N.check(_m5_bwd(m5, xd, vd, dx), "ap_m5_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all())
    out = nan_like((2, no), dev)
    N.check(_m5_fwd(m5, xd, out), "ap_m5_fwd")
    assert bool(torch.isfinite(out).all())


# ---- mel-dB --------------------------------------------------------------------------------------------------------------
def _mel_fwd(xd, out, n_mels, mode):
    return N.lib().ap_melspec_db(N.ptr(xd), N.ptr(out), n_mels, mode, xd.shape[0], xd.shape[-1], N.stream())


def _check_mel_forward(dev, x, tag):
    from audiopure_amd.transforms import MelSpecDB, ToMelSpectrogramDB
    B, L = x.shape[0], x.shape[-1]
    xd = x.to(dev).reshape(B, L)
    worst = 0.0
    for n_mels in R.MEL_FWD_MELS:
        for mode in (0, 1):
            ref = R.mel_db(x.double(), n_mels, mode)
            assert ref.shape == (B, 1, n_mels, 1 + L // 512)
            out = nan_like((B, n_mels, 1 + L // 512), dev)
            N.check(_mel_fwd(xd, out, n_mels, mode), "ap_melspec_db")
            err = float((out.cpu().double() - ref[:, 0]).abs().max())
            worst = max(worst, err if err == err else float("inf"))
            assert err <= MEL_ATOL, (tag, n_mels, mode, err)
            via_module = (MelSpecDB if mode == 0 else ToMelSpectrogramDB)(n_mels)(x.to(dev))
            assert via_module.shape == (B, 1, n_mels, 1 + L // 512) and torch.equal(via_module[:, 0], out)
    print(f"mel forward {tag}: max |d dB| = {worst:.2e}")


@pytest.mark.parametrize("L", R.MEL_FWD_L)
def test_mel_forward_matches_float64_at_every_frame_count_edge(dev, L):
    """L < 2048 (a frame longer than the clip), L % 512 in {0, 1, 511} (the last frame appears / holds one sample), and
    n_mels 32, 40, 64, 128 (the widest built) in both modes."""
    _check_mel_forward(dev, R.mel_noise(3, L), f"L={L}")


def test_mel_forward_on_loud_quiet_and_silent_stretches(dev):
    """Mode 1's -80 dB floor is reached from the very quiet stretch (above the 1e-10 clamp) and from the zeros (under it);
    mode 0 holds -100 exactly on the zeros."""
    x = R.mel_stretch_clips(R.MEL_FWD_STRETCHES)
    _check_mel_forward(dev, x, "stretches")
    out = nan_like((3, 32, 33), dev)
    N.check(_mel_fwd(x.to(dev).reshape(3, -1), out, 32, 1), "ap_melspec_db")
    ref = R.mel_db(x.double(), 32, 1)[:, 0]
    got = out.cpu()
    assert float(got.max()) == 0.0 and float(got.min()) == -80.0
    share, ref_share = float((got == -80.0).float().mean()), float((ref == -80.0).float().mean())
    assert abs(share - ref_share) < 0.01 and 0.3 < share < 0.6               # measured 0.44 on the reference


def test_mel_refusals_and_the_forward_only_mode(dev):
    from audiopure_amd.transforms import MelSpecDB, ToMelSpectrogramDB
    xd, out = R.mel_noise(2, 2048).to(dev), nan_like((2, 129, 5), dev)
    assert _mel_fwd(xd.reshape(2, -1), out, 129, 0) == -22
    assert _mel_fwd(xd.reshape(2, -1), out, 32, 2) == -22
    dx, scratch = nan_like((2, 2048), dev), nan_like((2, 5, 2048), dev)
    assert N.lib().ap_melspec_db_bwd(N.ptr(xd), N.ptr(out), N.ptr(dx), N.ptr(scratch), 129, 2, 2048, N.stream()) == -22
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(dx).all()) and bool(torch.isnan(scratch).all())
    with pytest.raises(NotImplementedError):
        ToMelSpectrogramDB(32)(xd.clone().requires_grad_(True))
    assert MelSpecDB(40)(xd).shape == (2, 1, 40, 5)


def _check_mel_gradient(dev, x, tag):
    B, L = x.shape[0], x.shape[-1]
    frames = 1 + L // 512
    xd = x.to(dev).reshape(B, L)
    for n_mels in R.MEL_GRAD_MELS:
        v = R.mel_cotangent(tag, B, n_mels, L)
        xr = x.double().requires_grad_(True)
        mel = R.mel_power(xr, n_mels)
        assert R.mel_clamp_is_far(mel.detach())
        (ref,) = torch.autograd.grad(R.mel_db(xr, n_mels), xr, v.double())
        dx, scratch = nan_like((B, L), dev), nan_like((B, frames, 2048), dev)
        vd = v.to(dev).reshape(B, n_mels, frames).contiguous()
        N.check(N.lib().ap_melspec_db_bwd(N.ptr(xd), N.ptr(vd), N.ptr(dx), N.ptr(scratch), n_mels, B, L, N.stream()),
                "ap_melspec_db_bwd")
        got = dx.cpu().double().reshape(B, 1, L)
        scale = R.local_scale(ref)
        excess = (got - ref).abs() - MEL_GRAD_LOCAL * scale
        worst = float(((got - ref).abs() / scale.clamp(min=1e-300)).max())
        print(f"mel gradient {tag} n_mels={n_mels}: max |d| / local max |ref| = {worst:.2e}")
        assert bool(torch.isfinite(got).all()) and float(excess.max()) <= 0.0, (tag, n_mels, worst)
        silent = R.mel_silent_samples(mel.detach(), L)
        assert bool((dx.cpu()[silent] == 0.0).all())
        yield silent


@pytest.mark.parametrize("L", R.MEL_GRAD_L)
def test_mel_input_gradient_matches_float64_autograd(dev, L):
    """Per sample against the largest reference gradient within +-2048 samples; L = 1, 513, 2049 put the gather's first /
    last covering frame at the clip's two ends."""
    for silent in _check_mel_gradient(dev, R.mel_noise(2, L), f"L={L}"):
        assert not bool(silent.any())


def test_mel_input_gradient_on_loud_quiet_and_silent_stretches(dev):
    """The gradient scales as 1 / power: 1e5 times larger in the quiet stretch than in the loud one, which a bound relative
    to the global maximum would never look at.  Where every covering frame is silent the clamp is active: dx is exactly 0."""
    for silent in _check_mel_gradient(dev, R.mel_stretch_clips(R.MEL_GRAD_STRETCHES), "s"):
        assert silent.sum(dim=1).tolist() == [6656, 5120]
