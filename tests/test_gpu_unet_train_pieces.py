"""The kernels of ap_unet_train.hip through the C-ABI, where they branch: ap_groupnorm_train_bwd against float64 autograd of the same
expression (bounds: 4 x float32 torch's error on the same case, recorded below and re-measured on the CPU by
test_unet_train_cpu.py), ap_dropout bit for bit against the numpy restatement, ap_silu_bwd and ap_qsample_rows
against float64, and ap_conv2d_wgrad on integer data, exact, at the geometries the UNet adds to test_gpu_conv2d_wgrad_edges.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_train_restate as R  # noqa: E402
from audiopure_amd import _native as N  # noqa: E402

NAN = float("nan")
EPS = 1e-5

# ---- ap_groupnorm_train_bwd: name -> (B, C, groups, HW, act, scale_shift?) -- HW in {4, 16, 25, 1024} (below a wave, a quarter block,
# odd, four turns of the block), channels per group in {1, 2, 3, 12}, B in {1, 3}, act 0 and 2, with and without the FiLM
GN_CASES = {
    "hw4_cpg1": (1, 32, 32, 4, 2, True),
    "hw16_cpg2": (3, 64, 32, 16, 2, True),
    "hw25_cpg3": (3, 96, 32, 25, 0, False),
    "hw1024_cpg12": (1, 384, 32, 1024, 2, True),
    "hw1024_cpg2_plain": (3, 64, 32, 1024, 2, False),
    "hw25_cpg12_linear": (1, 24, 2, 25, 0, True),
    "hw16_cpg3_plain": (3, 12, 4, 16, 2, False),
    "hw4_cpg12_linear": (3, 24, 2, 4, 0, True),
}
# float32 torch (autograd of the same expression on the CPU) against float64, per case the largest of the four outputs' max |d| / max
# |ref|; the bound of a case is 4 x its figure.  Measured by `gn_measure_f32`, re-measured by test_unet_train_cpu.py.
GN_F32_ERR = {
    "hw4_cpg1": 2.30e-07, "hw16_cpg2": 2.07e-07, "hw25_cpg3": 1.36e-07, "hw1024_cpg12": 3.95e-07, "hw1024_cpg2_plain": 2.60e-07,
    "hw25_cpg12_linear": 8.73e-08, "hw16_cpg3_plain": 1.76e-07, "hw4_cpg12_linear": 1.05e-07,
}
SILU_BWD_F32_ERR = 5.65e-07         # float32 torch's SiLU backward over [-20, 20] against float64, max |d| / max |ref|


@functools.lru_cache(maxsize=None)
def gn_inputs(name):
    """float32 x, gamma (channel 0 negative, the last channel exactly 0), beta, scale_shift or None, dy.  Shared: do not modify."""
    B, C, groups, HW, act, film = GN_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(B, C, HW, generator=g) * 1.5 + 0.3
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    gamma[0] = -gamma[0].abs() - 0.1
    gamma[C - 1] = 0.0
    ss = 0.5 * torch.randn(B, 2 * C, generator=g) if film else None
    dy = torch.randn(B, C, HW, generator=g)
    return x, gamma, beta, ss, dy


def gn_autograd(name, dtype):
    """(dx, dgamma, dbeta, dss or None) of sum(dy * act(group_norm(x) (1 + sc) + sh)) by autograd in `dtype`"""
    B, C, groups, HW, act, film = GN_CASES[name]
    x, gamma, beta, ss, dy = (None if t is None else t.to(dtype).clone().requires_grad_(True) for t in gn_inputs(name))
    y = F.group_norm(x, groups, gamma, beta, EPS)
    if film:
        y = y * (1 + ss[:, :C, None]) + ss[:, C:, None]
    if act == 2:
        y = y * torch.sigmoid(y)
    (y * dy.detach()).sum().backward()
    return x.grad, gamma.grad, beta.grad, (ss.grad if film else None)


def worst(got, ref):
    return max(R.rel(a, b) for a, b in zip(got, ref) if b is not None and a is not None)


def gn_measure_f32(name):
    return worst(gn_autograd(name, torch.float32), gn_autograd(name, torch.float64))


def silu_inputs():
    x = torch.linspace(-20.0, 20.0, 4001)
    dy = torch.randn(4001, generator=torch.Generator().manual_seed(4))
    return x, dy


def silu_bwd_autograd(dtype):
    x, dy = silu_inputs()
    x = x.to(dtype).requires_grad_(True)
    (x * torch.sigmoid(x) * dy.to(dtype)).sum().backward()
    return x.grad


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def gn_call(dev, name, x=None, skip=()):
    """-> (dx, dgamma, dbeta, dss) from ap_groupnorm_train_bwd; outputs and workspace start NaN-filled; `skip`: outputs passed NULL"""
    lib = N.lib()
    B, C, groups, HW, act, film = GN_CASES[name]
    x0, gamma, beta, ss, dy = (None if t is None else t.to(dev) for t in gn_inputs(name))
    x = x0 if x is None else x
    need = lib.ap_groupnorm_train_workspace_bytes(B, C)
    assert need == B * C * 8
    ws = torch.full((need // 4,), NAN, device=dev)
    outs = {"dx": torch.full_like(x0, NAN), "dgamma": torch.full((C,), NAN, device=dev), "dbeta": torch.full((C,), NAN, device=dev),
            "dss": torch.full((B, 2 * C), NAN, device=dev) if film else None}
    for k in skip:
        outs[k] = None
    N.check(lib.ap_groupnorm_train_bwd(N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(ss), N.ptr(dy), N.ptr(outs["dx"]), N.ptr(outs["dgamma"]),
                                       N.ptr(outs["dbeta"]), N.ptr(outs["dss"]), ws.data_ptr(), need, B, C, HW, groups, EPS, act,
                                       N.stream()), "ap_groupnorm_train_bwd")
    torch.cuda.synchronize()
    return tuple(outs[k] for k in ("dx", "dgamma", "dbeta", "dss"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GN_CASES))
def test_groupnorm_train_bwd_against_float64(dev, name):
    got = gn_call(dev, name)
    ref = gn_autograd(name, torch.float64)
    assert all(bool(torch.isfinite(t).all()) for t in got if t is not None)
    errs = [R.rel(a, b) for a, b in zip(got, ref) if b is not None]
    print(f"{name}: dx, dgamma, dbeta, dss: {['%.2e' % e for e in errs]}  bound {4 * GN_F32_ERR[name]:.2e}")
    assert (got[3] is None) == (ref[3] is None)
    assert max(errs) <= 4 * GN_F32_ERR[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hw16_cpg2", "hw1024_cpg12", "hw25_cpg3"])
def test_groupnorm_train_bwd_unaligned_and_null_outputs(dev, name):
    """x at a 4-byte (not 16-byte) aligned address gives the same bits; each output may be NULL and the others keep their bits."""
    full = gn_call(dev, name)
    x = gn_inputs(name)[0]
    buf = torch.empty(x.numel() + 5, device=dev)
    shift = next(s for s in range(1, 5) if (buf.data_ptr() + 4 * s) % 16 != 0)
    xu = buf[shift:shift + x.numel()].view(x.shape)
    xu.copy_(x)
    assert xu.data_ptr() % 16 != 0 and xu.is_contiguous()
    for a, b in zip(gn_call(dev, name, x=xu), full):
        assert (a is None and b is None) or torch.equal(a, b)
    keys = ("dx", "dgamma", "dbeta", "dss")
    for i, k in enumerate(keys):
        if full[i] is None:
            continue
        got = gn_call(dev, name, skip=(k,))
        assert got[i] is None
        for j in range(4):
            if j != i:
                assert (got[j] is None and full[j] is None) or torch.equal(got[j], full[j]), (k, keys[j])
    got = gn_call(dev, name, skip=("dgamma", "dbeta"))                    # the form a frozen GroupNorm takes: no workspace use
    assert torch.equal(got[0], full[0])


@pytest.mark.gpu
def test_groupnorm_train_bwd_refusals(dev):
    lib = N.lib()
    t = torch.zeros(64, device=dev)
    args = lambda **kw: [N.ptr(kw.get(k, t)) for k in ("x", "gamma", "beta", "ss", "dy", "dx", "dgamma", "dbeta", "dss")]
    assert lib.ap_groupnorm_train_bwd(*args(ss=None), t.data_ptr(), 256, 1, 4, 4, 2, EPS, 2, N.stream()) == -22      # dss without FiLM
    assert b"dss" in lib.ap_last_error()
    assert lib.ap_groupnorm_train_bwd(*args(), t.data_ptr(), 16, 1, 4, 4, 2, EPS, 2, N.stream()) == -22               # workspace too small
    assert lib.ap_groupnorm_train_bwd(*args(), t.data_ptr(), 256, 1, 4, 4, 3, EPS, 2, N.stream()) == -22              # C % groups
    assert lib.ap_groupnorm_train_bwd(*args(dx=None, dgamma=None, dbeta=None, dss=None), t.data_ptr(), 256, 1, 4, 4, 2, EPS, 2,
                                      N.stream()) == -22
    assert lib.ap_groupnorm_train_workspace_bytes(0, 4) == 0


def dropout_call(dev, x, p, seed, draw, offset):
    y = torch.full_like(x, NAN)
    N.check(N.lib().ap_dropout(N.ptr(x), N.ptr(y), x.shape[0], x.shape[1], p, seed, draw, offset, N.stream()), "ap_dropout")
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 64, 4096 + 3])
@pytest.mark.parametrize("p", [0.0, 0.3, 0.9])
def test_dropout_is_the_numpy_restatement_bit_for_bit(dev, n, p):
    seed, draw, offset, B = 0xFEDCBA9876543210, 3, (1 << 32) + 5, 4           # both words of the seed and of the sample index in use
    x = torch.randn(B, n, generator=torch.Generator().manual_seed(n))
    if p == 0.0:
        x[0, 0], x[1, 1], x[2, 2] = -0.0, 1e-40, NAN                           # p = 0 copies BITS
    want = x.numpy() * R.dropout_mask(seed, draw, offset, B, n, p)
    got = dropout_call(dev, x.to(dev), p, seed, draw, offset)
    if p == 0.0:
        assert np.array_equal(got.cpu().numpy().view(np.int32), x.numpy().view(np.int32))
    else:
        assert np.array_equal(got.cpu().numpy(), want)
        # rows 2-3 of the B = 4 call are a B = 2 call at sample_offset + 2; the backward is the same mask on dy
        sub = dropout_call(dev, x[2:].to(dev).contiguous(), p, seed, draw, offset + 2)
        assert np.array_equal(sub.cpu().numpy().view(np.int32), got[2:].cpu().numpy().view(np.int32))
        dy = torch.ones(B, n)
        assert np.array_equal(dropout_call(dev, dy.to(dev), p, seed, draw, offset).cpu().numpy(), R.dropout_mask(seed, draw, offset, B, n, p))
        assert not torch.equal(dropout_call(dev, dy.to(dev), p, seed, draw + 1, offset), dropout_call(dev, dy.to(dev), p, seed, draw, offset))


@pytest.mark.gpu
def test_dropout_refuses_p_outside_the_half_open_interval(dev):
    x = torch.ones(2, 8, device=dev)
    y = torch.full_like(x, 7.0)
    for p in (1.0, -0.1, NAN, 1.5):
        assert N.lib().ap_dropout(N.ptr(x), N.ptr(y), 2, 8, p, 1, 0, 0, N.stream()) == -22
        assert b"ap_dropout" in N.lib().ap_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                              # refused before any launch


@pytest.mark.gpu
def test_silu_bwd_and_qsample_rows_against_float64(dev):
    lib = N.lib()
    x, dy = silu_inputs()
    xd, dyd, dx = x.to(dev), dy.to(dev), torch.full_like(x, NAN).to(dev)    # (named: a temporary's block is reused by the next one)
    N.check(lib.ap_silu_bwd(N.ptr(xd), N.ptr(dyd), N.ptr(dx), x.numel(), N.stream()), "ap_silu_bwd")
    e = R.rel(dx, silu_bwd_autograd(torch.float64))
    print(f"ap_silu_bwd: {e:.2e}  bound {4 * SILU_BWD_F32_ERR:.2e}")
    assert e <= 4 * SILU_BWD_F32_ERR
    g = torch.Generator().manual_seed(9)
    B, n = 3, 1024 + 7
    x0, z = torch.randn(B, n, generator=g), torch.randn(B, n, generator=g)
    sa, sb = R.tables()
    a = torch.from_numpy(sa[[0, 37, 199]].astype(np.float32))
    b = torch.from_numpy(sb[[0, 37, 199]].astype(np.float32))
    out = torch.full((B, n), NAN, device=dev)
    x0d, zd, ad, bd = x0.to(dev), z.to(dev), a.to(dev), b.to(dev)
    N.check(lib.ap_qsample_rows(N.ptr(x0d), N.ptr(zd), N.ptr(ad), N.ptr(bd), N.ptr(out), B, n, N.stream()), "ap_qsample_rows")
    ax, bz = a.double()[:, None] * x0.double(), b.double()[:, None] * z.double()
    assert bool(((out.cpu().double() - (ax + bz)).abs() <= 2.0 ** -23 * (ax.abs() + bz.abs())).all())
    assert lib.ap_qsample_rows(N.ptr(out), N.ptr(out), None, N.ptr(out), N.ptr(out), B, n, N.stream()) == -22
    assert lib.ap_silu_bwd(N.ptr(dx), N.ptr(dx), None, 4, N.stream()) == -22


# ---- ap_conv2d_wgrad at the geometries this net adds: (B, Cin, H, W, Cout, k, stride, pad, groups, x_cstride, x_coff) ---------------
WGRAD_CASES = {
    "downsample_8x8": (3, 64, 8, 8, 64, 3, 2, 1, 1, 64, 0),                # Downsample.op: 3 x 3 stride 2 pad 1, 8 x 8 -> 4 x 4
    "out_conv_cout_1": (2, 32, 8, 8, 1, 3, 1, 1, 1, 32, 0),                # out.2: one row
    "stem_cin_1_cout_128": (2, 1, 16, 16, 128, 3, 1, 1, 1, 1, 0),          # input_blocks.0.0 of the shipped net: 9 columns, a full row tile
    "qkv_conv1d_t64": (2, 64, 8, 8, 192, 1, 1, 0, 1, 64, 0),               # AttentionBlock.qkv: Cout = 3 C over T = 64
    "linear_b3_704_rows": (3, 128, 1, 1, 704, 1, 1, 0, 1, 128, 0),         # the concatenated emb_layers rows, contracted over B = 3 alone
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_conv2d_wgrad_exact_at_the_unets_geometries(dev, name):
    import test_gpu_conv2d_wgrad_edges as E
    from audiopure_amd import synth
    c = WGRAD_CASES[name]
    B, Cin, H, W, Cout, k, s, pad, g, cs, co = c
    OH, OW = E.geometry(c)
    x = torch.from_numpy(synth.uniform("utw/x/" + name, (B, cs, H, W), 0, -2.49, 2.49)).round()
    dy = torch.from_numpy(synth.uniform("utw/dy/" + name, (B, Cout, OH, OW), 0, -1.49, 1.49)).round()
    ref = E.reference(x, dy, c)
    assert float(ref.abs().max()) > 0
    got = E.wgrad(dev, x.to(dev), dy.to(dev), c)
    assert torch.equal(got.cpu().double(), ref)
