"""ap_gate_bwd and ap_relu_outer_bwd (ap_backward.hip) called by name: until now they ran only inside whole-net gradients, at
pre-activations that never saturate.  ap_gate_bwd against float64 autograd of tanh(a_t) sigmoid(a_s) under a bound derived from
its arithmetic; ap_relu_outer_bwd, one fp32 product behind a sign test, exactly."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiopure_amd import synth  # noqa: E402
from audiopure_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
GATE_SHAPES = [(2, 3, 77), (2, 64, 130)]                          # 462 elements: no multiple of the 256-thread workgroup; 65 of them
PLANTS_T = (0.0, 15.0, -15.0, 16.0, -16.0, 40.0, -40.0)
PLANTS_S = (0.0, 88.5, -88.5, 100.0, -100.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def U(key, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform(key, shape, 3, lo, hi))


def gate_inputs(B, C_, L):
    """a [B][2C][L] uniform in [-3, 3) with every (a_t, a_s) pair of the planted values somewhere, dg uniform in [-1, 1)"""
    a, dg = U(f"gba{C_}.{L}", (B, 2 * C_, L), -3.0, 3.0).clone(), U(f"gbd{C_}.{L}", (B, C_, L))
    i = 0
    for vt in PLANTS_T + (None,):
        for vs in PLANTS_S + (None,):
            b, c, t = i % B, (5 * i) % C_, (17 * i + 3) % L
            if vt is not None:
                a[b, c, t] = vt
            if vs is not None:
                a[b, C_ + c, t] = vs
            i += 1
    return a, dg


def gate_bwd(dev, a, dg):
    B, C2, L = a.shape
    ad, dgd = a.to(dev), dg.to(dev)
    da = torch.full(a.shape, NAN, device=dev)
    N.check(N.lib().ap_gate_bwd(N.ptr(ad), N.ptr(dgd), N.ptr(da), B, C2 // 2, L, N.stream()), "ap_gate_bwd")
    return da.cpu()


@pytest.mark.parametrize("B,C_,L", GATE_SHAPES)
def test_gate_bwd_matches_float64_autograd(dev, B, C_, L):
    """|da - da_ref| <= 16 * 2^-24 |dg| per element, absolute.  expf is good to 1 ulp and the build has no fast-math; E = expf(2 a_t)
    carries 2^-24 E, E - 1 is exact near 0, so th = (E - 1) / (E + 1) carries about 3.4 * 2^-24 absolute, 1 - th^2 about twice that,
    sg = 1 / (1 + expf(-a_s)) a few ulp relative, and the products three more roundings -- all times factors <= 1.  The kernel's
    clamp of a_t at +-15 moves the true derivative by less than 4e-13.  Measured on an MI355X: see DESIGN.md."""
    a, dg = gate_inputs(B, C_, L)
    a64 = a.double().requires_grad_(True)
    g = torch.tanh(a64[:, :C_]) * torch.sigmoid(a64[:, C_:])
    (ref,) = torch.autograd.grad(g, a64, dg.double())
    assert torch.isfinite(ref).all()
    da = gate_bwd(dev, a, dg)
    assert torch.isfinite(da).all()
    unit = 2.0 ** -24 * torch.cat([dg, dg], 1).double().abs()
    err = (da.double() - ref).abs()
    worst = float((err / unit.clamp_min(1e-300)).max())
    at = int((err / unit.clamp_min(1e-300)).argmax())
    print(f"worst |da - da_ref| = {worst:.2f} x 2^-24 |dg| (bound 16), at a = {float(a.reshape(-1)[at]):.4f}")
    assert (err <= 16 * unit).all()


def test_gate_bwd_halves_are_where_the_forward_reads_them(dev):
    """dg zero but in channel 2: da is zero but in rows 2 (the tanh half) and C + 2 (the sigmoid half), and those two differ as
    d/da_t and d/da_s do."""
    B, C_, L = 2, 3, 77
    a, dg = gate_inputs(B, C_, L)
    dg = torch.zeros_like(dg)
    dg[:, 2] = U("gbone", (B, L), 0.5, 1.0)
    da = gate_bwd(dev, a, dg)
    rows = [2, C_ + 2]
    others = [r for r in range(2 * C_) if r not in rows]
    assert torch.count_nonzero(da[:, others]).item() == 0
    a64 = a.double()
    th, sg = torch.tanh(a64[:, 2]), torch.sigmoid(a64[:, C_ + 2])
    unit = 16 * 2.0 ** -24 * dg[:, 2].double()
    assert ((da[:, 2].double() - dg[:, 2].double() * sg * (1 - th * th)).abs() <= unit).all()
    assert ((da[:, C_ + 2].double() - dg[:, 2].double() * th * sg * (1 - sg)).abs() <= unit).all()
    assert float((da[:, 2] - da[:, C_ + 2]).abs().max()) > 0.1   # the halves are not each other


@pytest.mark.parametrize("B,S,L", [(2, 5, 77), (1, 64, 300)])
def test_relu_outer_bwd_is_the_masked_product_exactly(dev, B, S, L):
    """dr = r > 0 ? w2[c] deps[b][t] : 0 from a NaN-filled dr; r holds +0.0, -0.0 and negatives (all masked)."""
    r, w2, deps = U(f"ror{S}.{L}", (B, S, L)).clone(), U(f"row{S}", (S,)), U(f"rod{L}", (B, 1, L))
    flat = r.view(-1)
    flat[0::7] = 0.0
    flat[1::7] = -0.0
    assert (r < 0).any() and (r > 0).any() and bool(torch.signbit(r[r == 0]).any()) and not bool(torch.signbit(r[r == 0]).all())
    ref = torch.where(r > 0, w2.view(1, S, 1) * deps, torch.zeros(()))
    rd, wd, dd = r.to(dev), w2.to(dev), deps.to(dev).contiguous()
    dr = torch.full((B, S, L), NAN, device=dev)
    N.check(N.lib().ap_relu_outer_bwd(N.ptr(rd), N.ptr(wd), N.ptr(dd), N.ptr(dr), B, S, L, N.stream()), "ap_relu_outer_bwd")
    dr = dr.cpu()
    assert not torch.isnan(dr).any()
    assert torch.equal(dr, ref)
    assert torch.count_nonzero(dr[r <= 0]).item() == 0 and torch.count_nonzero(dr).item() > dr.numel() // 4


def test_backward_pieces_refuse_null_and_empty(dev):
    lib = N.lib()
    t = torch.full((2 * 6 * 77,), NAN, device=dev)
    p, st = N.ptr(t), N.stream()
    for args in ((None, p, p, 2, 3, 77), (p, None, p, 2, 3, 77), (p, p, None, 2, 3, 77), (p, p, p, 0, 3, 77), (p, p, p, 2, 0, 77), (p, p, p, 2, 3, 0)):
        assert lib.ap_gate_bwd(*args, st) == -22
    assert b"ap_gate_bwd" in lib.ap_last_error()
    for args in ((None, p, p, p, 2, 3, 77), (p, None, p, p, 2, 3, 77), (p, p, None, p, 2, 3, 77), (p, p, p, None, 2, 3, 77), (p, p, p, p, 0, 3, 77),
                 (p, p, p, p, 2, 0, 77), (p, p, p, p, 2, 3, 0)):
        assert lib.ap_relu_outer_bwd(*args, st) == -22
    assert b"ap_relu_outer_bwd" in lib.ap_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(t).all()                                   # nothing was launched
