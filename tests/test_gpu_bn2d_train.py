"""ap_bn2d_train_fwd / ap_bn2d_train_bwd through the C-ABI against float64 (torch functionals and autograd), where the kernels branch:
two values per channel, HW = 1, one channel and more than two wave-widths of channels, a channel slice, the fused ReLU with a
negative gamma and a gamma of exactly 0, two momenta, a channel of constant input.  Every buffer a kernel writes starts NaN-filled;
the workspace has exactly the size the query returned.  Bounds: measured on these cases, case by case (F32_ERR below), per
tensor as max |d| / max |ref|."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
from audiopure_amd import synth  # noqa: E402
from audiopure_amd import _native as N  # noqa: E402
import convnet_train_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAN, EPS = float("nan"), 1e-5

# name: (B, C, H W, x_cstride, x_coff, relu, momentum)
CASES = {
    "two_values": (2, 3, 1, 3, 0, 0, 0.1),                # n = 2: the unbiased variance is twice the biased one
    "hw1_b4": (4, 5, 1, 5, 0, 1, 0.1),
    "one_channel": (3, 1, 35, 1, 0, 0, 0.1),
    "c130": (2, 130, 9, 130, 0, 1, 0.1),                  # the finalising kernels' third block of 64 channels, two of them live
    "slice": (3, 6, 16, 12, 3, 1, 0.1),                   # channels [3, 9) of 12
    "relu_gammas": (4, 8, 64, 8, 0, 1, 0.1),              # gamma[0] < 0, gamma[1] == 0
    "cumulative": (4, 8, 64, 8, 0, 0, 0.25),              # momentum=None at num_batches_tracked = 3: 1 / 4
    "constant_channel": (4, 4, 25, 4, 0, 0, 0.1),         # channel 2 constant: variance 0, rstd = 1 / sqrt(eps), finite gradients
    "several_slices": (5, 2, 1000, 2, 0, 1, 0.1),         # n = 5000: every one of the 64 slices has work, slices straddle images
}


def inputs(name):
    B, C, HW, cs, co, relu, mom = CASES[name]
    x = torch.from_numpy(synth.uniform("bn2d/x/" + name, (B, cs, HW), 0, -2.0, 3.0))
    gamma = torch.from_numpy(synth.uniform("bn2d/g/" + name, (C,), 0, 0.5, 1.5))
    beta = torch.from_numpy(synth.uniform("bn2d/b/" + name, (C,), 0, -0.5, 0.5))
    rm = torch.from_numpy(synth.uniform("bn2d/rm/" + name, (C,), 0, -0.2, 0.2))
    rv = torch.from_numpy(synth.uniform("bn2d/rv/" + name, (C,), 0, 0.5, 1.5))
    dy = torch.from_numpy(synth.uniform("bn2d/dy/" + name, (B, C, HW), 0, -1.0, 1.0))
    if name == "relu_gammas":
        gamma[0], gamma[1], beta[1] = -1.25, 0.0, 0.3         # (beta > 0: the ReLU lets the constant channel through)
    if name == "constant_channel":
        x[:, 2] = 0.75
    return x, gamma, beta, rm, rv, dy


def reference(name):
    B, C, HW, cs, co, relu, mom = CASES[name]
    x, gamma, beta, rm, rv, dy = (t.double() for t in inputs(name))
    xs = x[:, co:co + C].clone().requires_grad_(True)
    g, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    n = B * HW
    mu = xs.mean((0, 2))
    var = ((xs - mu[None, :, None]) ** 2).mean((0, 2))
    rstd = 1.0 / torch.sqrt(var + EPS)
    y = (xs - mu[None, :, None]) * rstd[None, :, None] * g[None, :, None] + b[None, :, None]
    if relu:
        y = torch.relu(y)
    y.backward(dy)
    return dict(y=y.detach(), stat=torch.stack([mu, rstd]).detach(), rm=(1 - mom) * rm + mom * mu.detach(),
                rv=(1 - mom) * rv + mom * var.detach() * n / (n - 1), dx=xs.grad, dgamma=g.grad, dbeta=b.grad)


# Bounds measured on THESE cases, case by case (the networks' bounds contain whole networks' error growth and would let a wrong
# formula pass here): 4 x the error of float32 torch (F.batch_norm in training mode, ReLU, autograd, on the CPU) against the float64
# reference above, per tensor as max |d| / max |ref|, the largest of the forward tensors (y, stat, running statistics) and of the
# backward tensors (dx, dgamma, dbeta) -- `measure_f32`, re-measured by test_convnet_train_cpu.py.  Two figures stand out and are
# properties of the case, not of an implementation: with n = 2 values per channel xhat is +-1 and dx is what the eps in
# 1 / sqrt(var + eps) leaves of an exact cancellation (max |dx| is 1e-5 of max |dy|), so float32 inputs alone move it by 7e-3; and
# float32 torch does not get a variance of exactly 0 for the constant channel.
F32_ERR = {"two_values": (1.1e-7, 7.2e-3), "hw1_b4": (7.6e-8, 5.4e-7), "one_channel": (8.0e-8, 1.4e-7), "c130": (9.0e-8, 1.3e-7),
           "slice": (9.4e-8, 1.8e-7), "relu_gammas": (9.5e-8, 1.4e-7), "cumulative": (8.1e-8, 1.6e-7),
           "constant_channel": (2.5e-6, 1.2e-7), "several_slices": (7.7e-8, 5.5e-7)}
FWD_KEYS, GRAD_KEYS = ("y", "stat", "rm", "rv"), ("dx", "dgamma", "dbeta")


def measure_f32(name):
    """float32 torch on the case -> (forward error, backward error) against `reference`"""
    import torch.nn.functional as F
    B, C, HW, cs, co, relu, mom = CASES[name]
    x, gamma, beta, rm, rv, dy = inputs(name)
    ref = reference(name)
    xs = x[:, co:co + C].clone().requires_grad_(True)
    g, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.batch_norm(xs, rm, rv, g, b, True, mom, EPS)
    if relu:
        y = torch.relu(y)
    y.backward(dy)
    mu = xs.detach().mean((0, 2))
    rstd = 1.0 / torch.sqrt(xs.detach().var((0, 2), unbiased=False) + EPS)
    got = dict(y=y.detach(), stat=torch.stack([mu, rstd]), rm=rm, rv=rv, dx=xs.grad, dgamma=g.grad, dbeta=b.grad)
    return max(R.rel(got[k], ref[k]) for k in FWD_KEYS), max(R.rel(got[k], ref[k]) for k in GRAD_KEYS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", list(CASES))
def test_forward_running_statistics_and_backward_match_float64(dev, name):
    lib = N.lib()
    B, C, HW, cs, co, relu, mom = CASES[name]
    x, gamma, beta, rm, rv, dy = (t.to(dev) for t in inputs(name))
    ref = reference(name)
    need = lib.ap_bn2d_train_workspace_bytes(C)
    assert need > 0 and need % 8 == 0
    ws = torch.full((need // 8,), NAN, device=dev, dtype=torch.float64)
    y, stat = torch.full((B, C, HW), NAN, device=dev), torch.full((2, C), NAN, device=dev)
    N.check(lib.ap_bn2d_train_fwd(N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(rm), N.ptr(rv), N.ptr(y), N.ptr(stat), ws.data_ptr(), need, B, C,
                                  HW, cs, co, EPS, mom, relu, N.stream()), "ap_bn2d_train_fwd")
    dx, dg, db = torch.full((B, C, HW), NAN, device=dev), torch.full((C,), NAN, device=dev), torch.full((C,), NAN, device=dev)
    ws2 = torch.full((need // 8,), NAN, device=dev, dtype=torch.float64)
    N.check(lib.ap_bn2d_train_bwd(N.ptr(x), N.ptr(y), N.ptr(dy), N.ptr(gamma), N.ptr(stat), N.ptr(dx), N.ptr(dg), N.ptr(db), ws2.data_ptr(),
                                  need, B, C, HW, cs, co, relu, N.stream()), "ap_bn2d_train_bwd")
    got = dict(y=y, stat=stat, rm=rm, rv=rv, dx=dx, dgamma=dg, dbeta=db)
    fwd_bound, grad_bound = (4 * e for e in F32_ERR[name])
    for k, bound in [(k, fwd_bound) for k in FWD_KEYS] + [(k, grad_bound) for k in GRAD_KEYS]:
        assert torch.isfinite(got[k]).all(), k
        err = R.rel(got[k], ref[k])
        print(f"{name} {k}: max |d| / max |ref| = {err:.2e} (bound {bound:.2e})")
        assert err <= bound, k
    if relu:                                                      # the mask is y > 0 of the value AFTER the affine: identical decisions
        assert torch.equal(y.cpu() > 0, ref["y"] > 0)
    if name == "relu_gammas":
        assert torch.equal(y[:, 1].cpu(), torch.relu(beta[1].cpu()).expand(B, HW)) and float(dg[1]) != 0.0
        assert float(dx[:, 1].abs().max()) == 0.0               # gamma = 0: no gradient reaches x, d gamma still does
    if name == "constant_channel":
        assert abs(float(stat[1, 2]) - EPS ** -0.5) <= fwd_bound * EPS ** -0.5
    # the optional outputs: the sums alone, nothing else written
    dg2 = torch.full((C,), NAN, device=dev)
    N.check(lib.ap_bn2d_train_bwd(N.ptr(x), N.ptr(y), N.ptr(dy), N.ptr(gamma), N.ptr(stat), None, N.ptr(dg2), None, ws2.data_ptr(), need, B, C,
                                  HW, cs, co, relu, N.stream()), "ap_bn2d_train_bwd")
    assert torch.equal(dg2, dg)


def test_two_runs_give_equal_bits(dev):
    lib = N.lib()
    name = "several_slices"
    B, C, HW, cs, co, relu, mom = CASES[name]
    outs = []
    for _ in range(2):
        x, gamma, beta, rm, rv, dy = (t.to(dev) for t in inputs(name))
        need = lib.ap_bn2d_train_workspace_bytes(C)
        ws = torch.full((need // 8,), NAN, device=dev, dtype=torch.float64)
        y, stat, dx = torch.full((B, C, HW), NAN, device=dev), torch.full((2, C), NAN, device=dev), torch.full((B, C, HW), NAN, device=dev)
        dg, db = torch.full((C,), NAN, device=dev), torch.full((C,), NAN, device=dev)
        N.check(lib.ap_bn2d_train_fwd(N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(rm), N.ptr(rv), N.ptr(y), N.ptr(stat), ws.data_ptr(), need, B,
                                      C, HW, cs, co, EPS, mom, relu, N.stream()), "ap_bn2d_train_fwd")
        N.check(lib.ap_bn2d_train_bwd(N.ptr(x), N.ptr(y), N.ptr(dy), N.ptr(gamma), N.ptr(stat), N.ptr(dx), N.ptr(dg), N.ptr(db), ws.data_ptr(),
                                      need, B, C, HW, cs, co, relu, N.stream()), "ap_bn2d_train_bwd")
        outs.append((y, stat, rm, rv, dx, dg, db))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_refused_before_any_launch(dev):
    lib = N.lib()
    C = 4
    x, g, b, rm, rv = (torch.ones(C, device=dev) for _ in range(5))
    y, stat = torch.full((C,), NAN, device=dev), torch.full((2, C), NAN, device=dev)
    need = lib.ap_bn2d_train_workspace_bytes(C)
    ws = torch.full((need // 8,), NAN, device=dev, dtype=torch.float64)

    def fwd(B=1, HW=1, cs=C, co=0, wb=need, mom=0.1):
        return lib.ap_bn2d_train_fwd(N.ptr(x), N.ptr(g), N.ptr(b), N.ptr(rm), N.ptr(rv), N.ptr(y), N.ptr(stat), ws.data_ptr(), wb, B, C, HW, cs,
                                     co, EPS, mom, 0, N.stream())

    assert fwd() == -22 and b"more than 1" in lib.ap_last_error()             # n = 1: torch raises there too
    assert fwd(B=2, co=1) == -22 and fwd(B=2, wb=need - 8) == -22 and fwd(B=2, mom=1.5) == -22
    assert lib.ap_bn2d_train_bwd(N.ptr(x), N.ptr(y), N.ptr(x), N.ptr(g), N.ptr(stat), N.ptr(y), None, None, ws.data_ptr(), need, 1, C, 1, C, 0, 0,
                                 N.stream()) == -22
    assert lib.ap_bn2d_train_workspace_bytes(0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(stat).all() and torch.isnan(ws).all()
    assert torch.equal(rm, torch.ones_like(rm)) and torch.equal(rv, torch.ones_like(rv))
