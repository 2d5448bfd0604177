"""The UNet's primitive kernels (ap_convnet.hip, ap_unet_bwd.hip) against float64 references (frontend_restate.py), at the
shapes where they branch: attention on its scalar and 16-byte paths, past 256 positions, at 64 channels off and on the MFMA
shapes and at the LDS limit; GroupNorm backward at seven shapes and three activations; the small elementwise kernels, which
had no direct test.  Every kernel writes into a NaN-filled buffer; every refusal is returned before any launch."""
import numpy as np
import pytest
import torch

import frontend_restate as R
from audiopure_amd import _native as N
from conftest import rel_err

pytestmark = pytest.mark.gpu

ATT_FWD_TOL, ATT_BWD_TOL, GN_BWD_TOL = 3e-6, 1e-5, 1e-5       # the bounds of test_gpu_unet.py (max |d| / max |ref|)
# peaked rows (qkv x 4): float32 torch on the CPU is itself (forward, gradient) this far from float64; the tolerance of such
# a case is max(the bound above, 4 x this)
ATT_F32_ERR = {(64, 128, 2): (6.7e-6, 3.9e-6), (32, 100, 1): (2.7e-6, 1.2e-6), (64, 256, 3): (7.0e-6, 3.9e-6)}
# float32 numpy cos / sin against float64 on the same (float32) arguments, by dim; the tolerance is 4 x this
TEMB_NUMPY_F32_ERR = {2: 3.0e-8, 128: 5.0e-8}
ULPS = 2.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def nan_like(shape, dev):
    return torch.full(shape, float("nan"), device=dev, dtype=torch.float32)


def _att_tols(ch, T, heads, peaked):
    if not peaked:
        return ATT_FWD_TOL, ATT_BWD_TOL
    f, b = ATT_F32_ERR[(ch, T, heads)]
    return max(ATT_FWD_TOL, 4 * f), max(ATT_BWD_TOL, 4 * b)


@pytest.mark.parametrize("ch,T,heads,peaked", R.ATT_CASES)
def test_attention_forward_and_backward_match_float64(dev, ch, T, heads, peaked):
    lib = N.lib()
    B, C = R.ATT_B, heads * ch
    qkv, do = R.att_inputs(ch, T, heads, peaked)
    q64 = qkv.double().requires_grad_(True)
    ref = R.qkv_attention(q64, heads)
    (gref,) = torch.autograd.grad(ref, q64, do.double())
    ftol, btol = _att_tols(ch, T, heads, peaked)
    qd, out = qkv.to(dev), nan_like((B, C, T), dev)
    N.check(lib.ap_attention_qkv(N.ptr(qd), N.ptr(out), B, C, T, heads, N.stream()), "ap_attention_qkv")
    ferr = rel_err(out.cpu().numpy(), ref.detach().numpy())
    # the backward takes `out` from the forward kernel, as the UNet's tape does
    dod, dq, stats = do.to(dev), nan_like((B, 3 * C, T), dev), nan_like((B * heads * T * 3,), dev)
    N.check(lib.ap_attention_qkv_bwd(N.ptr(qd), N.ptr(out), N.ptr(dod), N.ptr(dq), N.ptr(stats), B, C, T, heads, N.stream()),
            "ap_attention_qkv_bwd")
    berr = rel_err(dq.cpu().numpy(), gref.numpy())
    print(f"attention ch={ch} T={T} heads={heads} peaked={peaked}: forward {ferr:.2e} (tol {ftol:.1e}) backward {berr:.2e} (tol {btol:.1e})")
    assert ferr <= ftol and berr <= btol                                     # (NaN fails)
    assert bool(torch.isfinite(stats).all())


@pytest.mark.parametrize("C,T,heads,text", [(64, 321, 1, "164352 bytes"), (48, 16, 2, "channels per head 24 not built"),
                                            (64, 16, 3, "bad argument")])
def test_attention_refusals_leave_the_outputs_alone(dev, C, T, heads, text):
    lib = N.lib()
    qd, dod = torch.zeros((1, 3 * C, T), device=dev), torch.zeros((1, C, T), device=dev)
    out, dq, stats = nan_like((1, C, T), dev), nan_like((1, 3 * C, T), dev), nan_like((heads * T * 3,), dev)
    assert lib.ap_attention_qkv(N.ptr(qd), N.ptr(out), 1, C, T, heads, N.stream()) == -22
    assert text in lib.ap_last_error().decode()
    assert lib.ap_attention_qkv_bwd(N.ptr(qd), N.ptr(dod), N.ptr(dod), N.ptr(dq), N.ptr(stats), 1, C, T, heads, N.stream()) == -22
    assert text in lib.ap_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(dq).all()) and bool(torch.isnan(stats).all())


@pytest.mark.parametrize("case", R.GN_BWD_CASES)
def test_groupnorm_backward_matches_float64_autograd(dev, case):
    B, C, H, W, G, act, use_ss = case
    x, g, b, ss, dy = R.gn_inputs(B, C, H, W)
    xr = x.double().requires_grad_(True)
    y, y1 = R.groupnorm_film_act(xr, g.double(), b.double(), ss.double() if use_ss else None, G, act)
    (ref,) = torch.autograd.grad(y, xr, dy.double())
    xd, gd, bd, sd_, dyd = x.to(dev), g.to(dev), b.to(dev), ss.to(dev), dy.to(dev)
    dx = nan_like(tuple(x.shape), dev)
    N.check(N.lib().ap_groupnorm_bwd(N.ptr(xd), N.ptr(gd), N.ptr(bd), N.ptr(sd_) if use_ss else None, N.ptr(dyd), N.ptr(dx), B, C,
                                     H * W, G, 1e-5, act, N.stream()), "ap_groupnorm_bwd")
    got = dx.cpu().double()
    assert bool(torch.isfinite(got).all())
    keep = torch.ones(B, G, dtype=torch.bool)
    if act == 1:                                                             # a slab with an element at the ReLU's kink is not compared
        keep = R.groupnorm_decided(y1, G, R.GN_TAU)
        assert float((~keep).float().mean()) <= R.GN_MAX_SKIPPED
    m = keep[:, :, None].expand(B, G, (C // G) * H * W).reshape(x.shape)
    err = rel_err((got * m).numpy(), (ref * m).numpy())
    print(f"groupnorm backward {case}: {err:.2e}, {int((~keep).sum())} slabs skipped")
    assert err <= GN_BWD_TOL
    # the forward at the same shape, through the same restatement
    yd = nan_like(tuple(x.shape), dev)
    N.check(N.lib().ap_groupnorm_nchw(N.ptr(xd), N.ptr(gd), N.ptr(bd), N.ptr(sd_) if use_ss else None, N.ptr(yd), B, C, H * W, G, 1e-5,
                                      act, N.stream()), "ap_groupnorm_nchw")
    assert rel_err(yd.cpu().numpy(), y.detach().numpy()) <= 3e-6


@pytest.mark.parametrize("dim", [2, 128])
@pytest.mark.parametrize("n", R.SMALL_N)
def test_timestep_embedding_matches_float64_of_the_float32_argument(dev, n, dim):
    t, freqs = R.temb_inputs(n, dim)
    ref4, _ = R.temb_reference(np.asarray(R.TEMB_T, dtype=np.float32), freqs)    # t cycles through these four
    ref = ref4[np.arange(n) % 4]
    out = nan_like((n, dim), dev)
    td, fd = torch.from_numpy(t).to(dev), torch.from_numpy(freqs).to(dev)
    N.check(N.lib().ap_timestep_embedding(N.ptr(td), N.ptr(fd), N.ptr(out), n, dim, N.stream()), "ap_timestep_embedding")
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    print(f"timestep embedding n={n} dim={dim}: {err:.2e} (tol {4 * TEMB_NUMPY_F32_ERR[dim]:.1e})")
    assert err <= 4 * TEMB_NUMPY_F32_ERR[dim]


@pytest.mark.parametrize("with_z", [False, True])
@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("n", R.SMALL_N)
def test_psample_update_is_float32_exact(dev, n, clip, with_z):
    """Within 2 ulp of the result of float32 numpy in the kernel's operation order.  The compiler may fuse a product into
    the addition that follows it, and such a fused step differs from the two-rounding one by up to half an ulp of the
    PRODUCT -- hundreds of ulps of a result that cancels -- so the distance is taken to the nearest of the values the
    contractions C++ allows can give (frontend_restate.psample_forms; the first is the uncontracted one)."""
    x, eps, z = R.small_inputs(n)
    c = R.PSAMPLE_COEF
    forms = R.psample_forms(x, eps, z if with_z else None, clip=clip, **c)
    xd, ed, zd = (torch.from_numpy(a).to(dev) for a in (x, eps, z))
    out = nan_like((n,), dev)
    N.check(N.lib().ap_psample_update(N.ptr(xd), N.ptr(ed), N.ptr(zd) if with_z else None, N.ptr(out), c["r1"], c["r2"], c["c1"],
                                      c["c2"], c["sigma"], clip, n, N.stream()), "ap_psample_update")
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    plain, near = float(R.ulp_distance_to_nearest(got, forms[:1]).max()), float(R.ulp_distance_to_nearest(got, forms).max())
    print(f"psample n={n} clip={clip} z={with_z}: {near:.2f} ulp from the nearest form, {plain:.1f} from the uncontracted one")
    assert near <= ULPS


@pytest.mark.parametrize("with_y", [False, True])
@pytest.mark.parametrize("n", R.SMALL_N)
def test_axpbyc_is_float32_exact(dev, n, with_y):
    x, y, _ = R.small_inputs(n)
    a, b, c = 0.3, -1.7, 0.25
    forms = R.axpbyc_forms(x, y if with_y else None, a, b, c)
    xd, yd, out = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), nan_like((n,), dev)
    N.check(N.lib().ap_axpbyc(N.ptr(xd), N.ptr(yd) if with_y else None, N.ptr(out), a, b, c, n, N.stream()), "ap_axpbyc")
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    assert float(R.ulp_distance_to_nearest(got, forms).max()) <= ULPS
    if not with_y:                                                           # b must not matter without y
        out2 = nan_like((n,), dev)
        N.check(N.lib().ap_axpbyc(N.ptr(xd), None, N.ptr(out2), a, 123.0, c, n, N.stream()), "ap_axpbyc")
        assert torch.equal(out, out2)


@pytest.mark.parametrize("BC,H,W", [(6, 5, 7), (1, 1, 1)])
def test_upsample_nearest2x_is_exact(dev, BC, H, W):
    from audiopure_amd import synth
    x = torch.from_numpy(synth.uniform("upx", (BC, H, W), 1)).to(dev)
    y = nan_like((BC, 2 * H, 2 * W), dev)
    N.check(N.lib().ap_upsample_nearest2x(N.ptr(x), N.ptr(y), BC, H, W, N.stream()), "ap_upsample_nearest2x")
    assert torch.equal(y, x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))
