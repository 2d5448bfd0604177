"""The native training step on the GPU: the weight-gradient kernels through the C-ABI, every parameter gradient of
``training_loss`` and three SGD steps -- each against a float64 reference (einsum / autograd through the float64 oracle),
never against the code under test."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
from audiopure_amd import synth  # noqa: E402
from audiopure_amd import _native as N  # noqa: E402
import train_restate as T  # noqa: E402
from wgrad_restate import corr_reference  # noqa: E402  (the float64 einsum: shared with test_gpu_wgrad_edges.py)
from test_train_cpu import check_against_golden  # noqa: E402

pytestmark = pytest.mark.gpu

PLAIN, FILM, GATE = 0, 1, 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def U(key, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform(key, shape, 3, lo, hi))


def _net(cfg, dev, seed=0):
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.WaveNet import WaveNet_Speech_Commands
    sd = synth.wavenet_state_dict(cfg, seed)
    net = WaveNet_Speech_Commands(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.to(dev), sd


# ---- 1. ap_wgrad_corr -----------------------------------------------------------------------------------------
CORR_CASES = [(64, 32, 3, 1, 1, 37, PLAIN), (512, 256, 3, 4, 2, 640, FILM), (32, 32, 3, 8, 2, 129, FILM),
              (512, 256, 3, 2048, 2, 300, FILM), (256, 256, 1, 1, 3, 777, GATE)]


@pytest.mark.parametrize("M,Nn,taps,dil,B,L,mode", CORR_CASES)
def test_wgrad_corr_matches_float64_einsum(dev, M, Nn, taps, dil, B, L, mode):
    """Tolerance 1e-4 of max|G_ref| (test_gpu_grad.py's bar for the input gradient; the sums run to B L ~ 2000 terms).  FiLM values
    are large next to Q, so an implementation that adds them to the zero padding misses by far more."""
    lib = N.lib()
    key = f"wg{M}.{Nn}.{taps}.{dil}.{L}"
    P = U(key + "P", (B, M, L))
    Q = U(key + "Q", (B, 2 * Nn if mode == GATE else Nn, L), -2.0, 2.0)
    film = U(key + "f", (Nn,), 1.0, 3.0) if mode == FILM else None
    scale = math.sqrt(0.5)
    ref = scale * corr_reference(P, Q, film, taps, dil, mode)
    Pd, Qd, fd = P.to(dev), Q.to(dev), (film.to(dev) if film is not None else None)
    ws = torch.empty(lib.ap_wgrad_workspace_bytes(B, M, Nn, L, taps), device=dev, dtype=torch.uint8)
    assert ws.numel() > 0

    def run(G, accumulate):
        N.check(lib.ap_wgrad_corr(N.ptr(Pd), N.ptr(Qd), N.ptr(fd), N.ptr(G), ws.data_ptr(), ws.numel(), B, M, Nn, L, taps, dil, mode,
                                  scale, accumulate, N.stream()), "ap_wgrad_corr")
        return G

    G1 = run(torch.full((M, Nn, taps), float("nan"), device=dev), 0)
    G2 = run(torch.empty((M, Nn, taps), device=dev), 0)
    torch.cuda.synchronize()
    assert torch.equal(G1, G2)                                    # two runs: the same bits
    tol = 1e-4 * float(ref.abs().max())
    err = float((G1.cpu().double() - ref).abs().max())
    print(f"max|G - G_ref| = {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    for k in range(taps):
        if abs((k - taps // 2) * dil) >= L:                       # a tap no sample meets: exact zeros
            assert float(ref[:, :, k].abs().max()) == 0.0 and torch.count_nonzero(G1[:, :, k]).item() == 0
    prior = U(key + "G0", (M, Nn, taps)) * float(ref.abs().max())
    G3 = run(prior.to(dev).clone(), 1)
    assert float((G3.cpu().double() - (prior.double() + ref)).abs().max()) <= tol
    assert torch.equal(G3, prior.to(dev) + G1)                    # G + Delta, Delta being what accumulate = 0 writes


def test_wgrad_corr_refuses_bad_arguments(dev):
    lib = N.lib()
    t = torch.zeros(64 * 64 * 40, device=dev)
    ws = torch.empty(1 << 20, device=dev, dtype=torch.uint8)
    call = lambda M, Nn, taps, wsb: lib.ap_wgrad_corr(N.ptr(t), N.ptr(t), None, N.ptr(t), ws.data_ptr(), wsb, 1, M, Nn, 40, taps, 1, PLAIN, 1.0,
                                                      0, N.stream())
    assert call(48, 32, 3, ws.numel()) == -22 and call(32, 32, 2, ws.numel()) == -22
    assert call(32, 32, 3, 16) == -22                             # workspace too small: refused, nothing launched
    assert lib.ap_wgrad_corr(N.ptr(t), N.ptr(t), None, N.ptr(t), ws.data_ptr(), ws.numel(), 1, 32, 32, 40, 3, 1, FILM, 1.0, 0, N.stream()) == -22


# ---- 2. the small kernels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", ["one", "tensor", "broadcast", "broadcast+mask", "mask"])
def test_rowsum_matches_float64_autograd(dev, weighting):
    """Each weighting as the gradient it serves, by float64 autograd: a bias (w = 1), a per-row scale of a second tensor, of a
    broadcast row, and the init conv's weight / bias behind its ReLU (WaveNet.py:147,168).  Bound: thread i adds ceil(n / 256)
    terms in turn, then eight tree levels, plus the product's and the scale's roundings: (ceil(n / 256) + 10) 2^-24 sum|terms|."""
    _rowsum_case(dev, weighting, 3, 5, 777)


@pytest.mark.parametrize("B,M,L", [(1, 1, 1), (2, 3, 255), (1, 2, 257)])
@pytest.mark.parametrize("weighting", ["one", "broadcast+mask"])
def test_rowsum_at_the_edges_of_its_strided_loop(dev, weighting, B, M, L):
    """One element (255 threads add nothing), one short of and one past the 256-thread stride; the same bound formula.  The mask
    holds +0.0 and -0.0, which `> 0` both drops."""
    _rowsum_case(dev, weighting, B, M, L, zeros_in_mask=True)


def _rowsum_case(dev, weighting, B, M, L, zeros_in_mask=False):
    lib = N.lib()
    k = "" if (B, M, L) == (3, 5, 777) else f".{B}.{M}.{L}"
    A, W, Wb = U("rsA" + k, (B, M, L)), U("rsW" + k, (B, M, L)), U("rsWb" + k, (B, 1, L))
    w0, b0 = U("rsw0" + k, (M,)), U("rsb0" + k, (M,), -0.3, 0.3)
    p = torch.ones(M, dtype=torch.float64, requires_grad=True)
    A64 = A.double()
    h0 = torch.relu(w0.view(1, M, 1) * Wb + b0.view(1, M, 1))                   # fp32, as ap_init_conv forms it
    if zeros_in_mask and h0.numel() >= 3:
        h0.view(-1)[1::5] = 0.0
        h0.view(-1)[2::5] = -0.0
        assert bool(torch.signbit(h0[h0 == 0]).any()) and not bool(torch.signbit(h0[h0 == 0]).all())
    if weighting == "one":
        f, args = (A64 * (W.double() + p.view(1, M, 1))).sum(), (None, None, 0)
    elif weighting == "tensor":
        f, args = (A64 * W.double() * p.view(1, M, 1)).sum(), (W, None, 0)
    elif weighting == "broadcast":
        f, args = (A64 * Wb.double() * p.view(1, M, 1)).sum(), (Wb, None, 1)
    elif weighting == "broadcast+mask":                                        # d/dw0 of sum A relu(w0 x + b0), at the fp32 mask
        f, args = (A64 * (h0 > 0) * (p.view(1, M, 1) * Wb.double())).sum(), (Wb, h0, 1)
    else:
        f, args = (A64 * (h0 > 0) * p.view(1, M, 1)).sum(), (None, h0, 0)
    (ref,) = torch.autograd.grad(f, p)
    terms = A64.abs() * (1 if args[0] is None else args[0].double().abs()) * (1 if args[1] is None else (args[1] > 0))
    scale = 0.75
    bound = (math.ceil(B * L / 256) + 10) * 2.0 ** -24 * scale * terms.sum(dim=(0, 2))
    Wd, Rd = (None if a is None else a.to(dev).contiguous() for a in args[:2])
    out, Ad = torch.full((M,), float("nan"), device=dev), A.to(dev)
    N.check(lib.ap_rowsum(N.ptr(Ad), N.ptr(Wd), N.ptr(Rd), N.ptr(out), B, M, L, args[2], scale, 0, N.stream()), "ap_rowsum")
    first = out.clone()
    N.check(lib.ap_rowsum(N.ptr(Ad), N.ptr(Wd), N.ptr(Rd), N.ptr(out), B, M, L, args[2], scale, 1, N.stream()), "ap_rowsum")
    err = (first.cpu().double() - scale * ref).abs()
    print("err", err.tolist(), "bound", bound.tolist())
    assert (err <= bound).all()
    assert torch.equal(out, first + first)                        # accumulate = 1 adds the same sum again


def test_rowsum_f64_matches_float64_sum(dev):
    """The plain sum handed out as fp64 (the FiLM cotangents): fp32 inputs summed in fp64 -- at most n roundings of 2^-53 relative to
    sum|terms|; accumulate = 1 adds the same sum again."""
    lib = N.lib()
    B, M, L = 3, 5, 777
    A = U("rs64A", (B, M, L))
    ref = A.double().sum(dim=(0, 2))
    Ad, out = A.to(dev), torch.full((M,), float("nan"), device=dev, dtype=torch.float64)
    N.check(lib.ap_rowsum_f64(N.ptr(Ad), out.data_ptr(), B, M, L, 0, N.stream()), "ap_rowsum_f64")
    first = out.clone()
    N.check(lib.ap_rowsum_f64(N.ptr(Ad), out.data_ptr(), B, M, L, 1, N.stream()), "ap_rowsum_f64")
    bound = B * L * 2.0 ** -53 * A.double().abs().sum(dim=(0, 2))
    assert ((first.cpu() - ref).abs() <= bound).all()
    assert torch.equal(out, first + first)
    assert lib.ap_rowsum_f64(N.ptr(Ad), None, B, M, L, 0, N.stream()) == -22


@pytest.mark.parametrize("rows,cols", [(64, 96), (33, 1), (7, 768), (256, 256)])
def test_weight_norm_bwd_matches_float64_autograd(dev, rows, cols):
    """dg, dv of W = g v / ||v|| by the per-tensor rule (floor from the larger of the two); rows of one element: finite, dv = 0."""
    lib = N.lib()
    v, g, dW = U(f"wnv{rows}.{cols}", (rows, cols)), U(f"wng{rows}", (rows, 1), 0.5, 1.5), U(f"wnd{rows}.{cols}", (rows, cols))
    v64, g64 = v.double().requires_grad_(True), g.double().requires_grad_(True)
    W = v64 * (g64 / v64.norm(dim=1, keepdim=True))
    dg_ref, dv_ref = torch.autograd.grad(W, (g64, v64), dW.double())
    dg, dv = torch.full((rows, 1), float("nan"), device=dev), torch.full((rows, cols), float("nan"), device=dev)
    dWd, vd, gd = dW.to(dev), v.to(dev), g.to(dev)                # (held: three temporaries would share one freed block)
    N.check(lib.ap_weight_norm_bwd(N.ptr(dWd), N.ptr(vd), N.ptr(gd), N.ptr(dg), N.ptr(dv), rows, cols, N.stream()), "ap_weight_norm_bwd")
    G = max(float(dg_ref.abs().max()), float(dv_ref.abs().max()))
    T.check_tensor("dg", dg.cpu(), dg_ref, G)
    T.check_tensor("dv", dv.cpu(), dv_ref, G)
    if cols == 1:
        assert float(dv_ref.abs().max()) < 1e-12 and torch.count_nonzero(dv).item() == 0


@pytest.mark.parametrize("rows,cols", [(5, 300), (4, 2)])
def test_weight_norm_bwd_of_an_all_zero_row_is_zero_not_nan(dev, rows, cols):
    """Row 1 of v is all zero: it has no direction, and the kernel gives dg = 0 and dv = 0 exactly there (autograd gives NaN).  The
    other rows against float64 autograd under the per-tensor rule; more than one 256-thread stride of columns, and two columns."""
    lib = N.lib()
    v, g, dW = U(f"wnzv{rows}.{cols}", (rows, cols)).clone(), U(f"wnzg{rows}", (rows, 1), 0.5, 1.5), U(f"wnzd{rows}.{cols}", (rows, cols))
    v[1] = 0.0
    keep = [r for r in range(rows) if r != 1]
    v64, g64 = v[keep].double().requires_grad_(True), g[keep].double().requires_grad_(True)
    W = v64 * (g64 / v64.norm(dim=1, keepdim=True))
    dg_ref, dv_ref = torch.autograd.grad(W, (g64, v64), dW[keep].double())
    dg, dv = torch.full((rows, 1), float("nan"), device=dev), torch.full((rows, cols), float("nan"), device=dev)
    dWd, vd, gd = dW.to(dev), v.to(dev), g.to(dev)
    N.check(lib.ap_weight_norm_bwd(N.ptr(dWd), N.ptr(vd), N.ptr(gd), N.ptr(dg), N.ptr(dv), rows, cols, N.stream()), "ap_weight_norm_bwd")
    dg, dv = dg.cpu(), dv.cpu()
    assert torch.isfinite(dg).all() and torch.isfinite(dv).all()
    assert float(dg[1].abs().max()) == 0.0 and torch.count_nonzero(dv[1]).item() == 0
    G = max(float(dg_ref.abs().max()), float(dv_ref.abs().max()))
    T.check_tensor("dg", dg[keep], dg_ref, G)
    T.check_tensor("dv", dv[keep], dv_ref, G)


def test_embed_bwd_matches_float64_autograd(dev):
    """Embed dims 128 / 512 / 512: fc_t of every layer, then swish(fc_t2(swish(fc_t1(.)))), from a random dpart."""
    cfg = synth.mini_wavenet_config(64, 3, 12)
    assert (cfg["diffusion_step_embed_dim_in"], cfg["diffusion_step_embed_dim_mid"], cfg["diffusion_step_embed_dim_out"]) == (128, 512, 512)
    net, sd = _net(cfg, dev, seed=2)
    eng = net.engine()
    lib, NL, C_, E = eng.lib, 3, 64, 512
    step = 37.0
    dpart = U("edp", (NL, C_))
    # float64 reference
    lv = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd.items() if ".fc_t" in k}
    from oracle import diffwave_oracle as O
    sw = lambda t: t * torch.sigmoid(t)
    e0 = O.step_embedding(torch.full((1, 1), step, dtype=torch.float64), 128)
    emb = sw(torch.nn.functional.linear(e0, lv["residual_layer.fc_t1.weight"], lv["residual_layer.fc_t1.bias"]))
    emb = sw(torch.nn.functional.linear(emb, lv["residual_layer.fc_t2.weight"], lv["residual_layer.fc_t2.bias"]))
    f = sum((torch.nn.functional.linear(emb, lv[f"residual_layer.residual_blocks.{n}.fc_t.weight"],
                                        lv[f"residual_layer.residual_blocks.{n}.fc_t.bias"]).view(-1) * dpart[n].double()).sum() for n in range(NL))
    names = list(lv)
    ref = dict(zip(names, torch.autograd.grad(f, [lv[k] for k in names])))
    # native
    part = torch.empty(NL * C_ + E, device=dev)
    N.check(lib.ap_embed(eng.ctx, step, N.ptr(part), N.stream()), "ap_embed")
    z = lambda *s: torch.zeros(s, device=dev)
    fct_w, fct_b, w1, b1, w2, b2 = z(NL, C_, E), z(NL, C_), z(512, 128), z(512), z(512, 512), z(512)
    scratch, dpd = torch.empty(lib.ap_embed_bwd_scratch_elems(eng.ctx), device=dev), dpart.double().to(dev)
    for _ in range(2):                                            # accumulate = 1 twice onto zeros: twice the gradient
        N.check(lib.ap_embed_bwd(eng.ctx, step, dpd.data_ptr(), N.ptr(part[NL * C_:]), N.ptr(fct_w), N.ptr(fct_b), N.ptr(w1), N.ptr(b1),
                                 N.ptr(w2), N.ptr(b2), N.ptr(scratch), 1, N.stream()), "ap_embed_bwd")
    before = [t.clone() for t in (fct_w, fct_b, w1, b1, w2, b2)]    # a refusal (scratch off an 8-byte boundary) launches nothing
    assert lib.ap_embed_bwd(eng.ctx, step, dpd.data_ptr(), N.ptr(part[NL * C_:]), N.ptr(fct_w), N.ptr(fct_b), N.ptr(w1), N.ptr(b1), N.ptr(w2),
                            N.ptr(b2), scratch.data_ptr() + 4, 1, N.stream()) == -22
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (fct_w, fct_b, w1, b1, w2, b2)))
    got = {"residual_layer.fc_t1.weight": w1, "residual_layer.fc_t1.bias": b1, "residual_layer.fc_t2.weight": w2, "residual_layer.fc_t2.bias": b2}
    for n in range(NL):
        got[f"residual_layer.residual_blocks.{n}.fc_t.weight"] = fct_w[n]
        got[f"residual_layer.residual_blocks.{n}.fc_t.bias"] = fct_b[n]
    G = max(float(v.abs().max()) for v in ref.values())
    for k in names:
        T.check_tensor(k, got[k].cpu() / 2, ref[k], G)


def test_embed_bwd_without_accumulate_overwrites(dev):
    """accumulate = 0 into NaN-filled outputs gives the bits that the first accumulate = 1 call gives onto zeros."""
    cfg = synth.mini_wavenet_config(64, 3, 12)
    net, _ = _net(cfg, dev, seed=2)
    eng = net.engine()
    lib, NL, C_, E = eng.lib, 3, 64, 512
    step = 37.0
    part = torch.empty(NL * C_ + E, device=dev)
    N.check(lib.ap_embed(eng.ctx, step, N.ptr(part), N.stream()), "ap_embed")
    scratch, dpd = torch.empty(lib.ap_embed_bwd_scratch_elems(eng.ctx), device=dev), U("edp", (NL, C_)).double().to(dev)
    shapes = [(NL, C_, E), (NL, C_), (512, 128), (512,), (512, 512), (512,)]

    def run(fill, accumulate):
        outs = [torch.full(s, fill, device=dev) for s in shapes]
        N.check(lib.ap_embed_bwd(eng.ctx, step, dpd.data_ptr(), N.ptr(part[NL * C_:]), *(N.ptr(t) for t in outs), N.ptr(scratch), accumulate,
                                 N.stream()), "ap_embed_bwd")
        return outs

    added, written = run(0.0, 1), run(float("nan"), 0)
    for a, w in zip(added, written):
        assert torch.isfinite(w).all() and float(w.abs().max()) > 0
        assert torch.equal(a, w)


# ---- 3. - 5. training_loss ------------------------------------------------------------------------------------
def native_step(net, x, z, steps, dev):
    """(loss, {name: .grad}) of one native training step."""
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams, training_loss
    dh = calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG)
    net.zero_grad(set_to_none=True)
    loss = training_loss(net, torch.nn.MSELoss(), x.to(dev), dh, noise_source=(torch.tensor(steps), z.to(dev)))
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()}


_REF = {}


def reference_step(cfg, sd, x, z, steps, key):
    if key not in _REF:                                           # computed once, shared, never modified
        _REF[key] = T.oracle_grads(sd, cfg, x, z, steps, torch.float64)
    return _REF[key]


TRAIN_CASES = [(32, 3, 300, 3, [3, 3, 150]), (64, 13, 700, 2, [0, 0]), (256, 3, 640, 2, [17, 5])]


@pytest.mark.parametrize("C_,NL,L,B,steps", TRAIN_CASES)
def test_training_loss_gradients_match_float64_oracle(dev, monkeypatch, C_, NL, L, B, steps):
    """Every parameter gradient: two step groups on the 32-channel net, which runs zero-padded in the 64-channel kernels and so with
    kept pre-gate activations and the composed backward (C = 32); the same path at its own width with dilations 1024 and 2048 >= L
    (C = 64); the fused ap_resblock_bwd with dy_scratch (C = 256).  The composed backward WITHOUT kept pre-gate activations is
    test_training_loss_gradients_without_kept_pre_gate (C = 128).  Once with the default budget and once with every clip its own
    sub-batch."""
    from audiopure_amd.diffusion_models import _grad as Gm
    cfg = synth.mini_wavenet_config(C_, NL, 12)
    net, sd = _net(cfg, dev, seed=4)
    x = torch.from_numpy(synth.waveforms(B, L, seed=31))
    z = torch.from_numpy(synth.noise(0, B, L, seed=31))
    loss_ref, ref = reference_step(cfg, sd, x, z, steps, (C_, NL, L))
    loss, g = native_step(net, x, z, steps, dev)
    print(f"loss {loss:.7f} ref {loss_ref:.7f}")
    assert abs(loss - loss_ref) <= 2e-5 * abs(loss_ref)
    last = f"residual_layer.residual_blocks.{NL - 1}.res_conv."
    assert {k for k, v in g.items() if v is None} == {last + "bias", last + "weight_g", last + "weight_v"} == {k for k, v in ref.items() if v is None}
    G = T.largest(ref)
    for k, r in ref.items():
        if r is not None:
            T.check_tensor(k, g[k].cpu(), r, G)
    # every clip its own sub-batch: the save of ONE clip fits, that of two does not
    eg = Gm._eps_grad_of(net)
    one = eg.saved_bytes(x[:1].to(dev), True)
    monkeypatch.setattr(Gm, "SAVE_BUDGET_BYTES", one)
    plan = Gm.plan_sub_batches(steps, lambda k: eg.saved_bytes(x[:k].to(dev), True), one)
    assert all(len(idx) == 1 for _, idx in plan) and len(plan) == B
    loss1, g1 = native_step(net, x, z, steps, dev)
    singles = all(len(idx) == 1 for _, idx in Gm.step_groups(steps))
    for k, r in ref.items():
        if r is None:
            assert g1[k] is None
        elif singles:
            assert torch.equal(g1[k], g[k]), k                    # the same evaluations in the same order: the same bits
        else:
            print(f"{k}: per-clip vs batch {float((g1[k] - g[k]).abs().max()) / (float(g[k].abs().max()) + 1e-30):.2e} of max|g|")
            assert float((g1[k] - g[k]).abs().max()) <= 1e-6 * float(g[k].abs().max()) + 1e-30, k
            T.check_tensor(k + " (per clip)", g1[k].cpu(), r, G)


def test_training_loss_gradients_without_kept_pre_gate(dev):
    """C = 128: the library's block serves this width, but no save keeps pre-gate activations there (_link_plan: 64 and 256 only), so
    EpsGrad.backward recomputes y = DilConv(u) + b per layer and hands THAT to the gate-mode contractions.  Two step groups, one of
    two clips; every gradient against the float64 oracle under the per-tensor rule."""
    from audiopure_amd.diffusion_models import _grad as Gm
    C_, NL, L, B, steps = 128, 3, 300, 3, [3, 3, 150]
    cfg = synth.mini_wavenet_config(C_, NL, 12)
    net, sd = _net(cfg, dev, seed=4)
    x = torch.from_numpy(synth.waveforms(B, L, seed=31))
    z = torch.from_numpy(synth.noise(0, B, L, seed=31))
    eg = Gm._eps_grad_of(net)
    _, saved = eg.forward_save(x.to(dev), 3.0)
    assert saved.pre_gate is None and saved.gate_factors is None  # the path this test is about
    del saved
    loss_ref, ref = reference_step(cfg, sd, x, z, steps, (C_, NL, L))
    loss, g = native_step(net, x, z, steps, dev)
    print(f"loss {loss:.7f} ref {loss_ref:.7f}")
    assert abs(loss - loss_ref) <= 2e-5 * abs(loss_ref)
    assert {k for k, v in g.items() if v is None} == {k for k, v in ref.items() if v is None}
    G = T.largest(ref)
    for k, r in ref.items():
        if r is not None:
            T.check_tensor(k, g[k].cpu(), r, G)


def test_training_loss_under_no_grad_is_the_plain_forward(dev):
    """Evaluating the loss without autograd keeps nothing and agrees with the differentiable evaluation (2e-5 relative: the loss bar)."""
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams, training_loss
    cfg = synth.mini_wavenet_config(64, 3, 12)
    net, _ = _net(cfg, dev, seed=4)
    dh = calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG)
    x = torch.from_numpy(synth.waveforms(3, 300, seed=31)).to(dev)
    src = (torch.tensor([3, 3, 150]), torch.from_numpy(synth.noise(0, 3, 300, seed=31)).to(dev))
    a = training_loss(net, torch.nn.MSELoss(), x, dh, noise_source=src)
    with torch.no_grad():
        b = training_loss(net, torch.nn.MSELoss(), x, dh, noise_source=src)
    assert a.requires_grad and not b.requires_grad and b.grad_fn is None
    assert abs(a.item() - b.item()) <= 2e-5 * abs(a.item())


def test_narrow_net_forward_and_input_gradient_match_oracle(dev):
    """The 32-channel net through the 64-channel kernels, outside training: net.forward with per-clip steps, net.eps, and the input
    gradient, against the oracle at test_gpu_grad.py's bars (eps 2e-5, gradient 1e-4 of max)."""
    from oracle import diffwave_oracle as O
    cfg = synth.mini_wavenet_config(32, 3, 12)
    net, sd = _net(cfg, dev, seed=5)
    w = O.fold_state_dict(sd)
    B, L = 3, 300
    x = torch.from_numpy(synth.waveforms(B, L, seed=11))
    steps = torch.tensor([[3.0], [3.0], [150.0]])
    rel = lambda a, b: float((a - b).abs().max() / (b.abs().max() + 1e-30))
    with torch.no_grad():
        ref = O.eps_net(w, cfg, x, steps)
        assert rel(net((x.to(dev), steps.to(dev))).cpu(), ref) < 2e-5
        assert rel(net.eps(x[:2].to(dev), 3.0).cpu(), ref[:2]) < 2e-5
    v = U("nnv", (B, 1, L))
    xr = x.clone().requires_grad_(True)
    (g_ref,) = torch.autograd.grad(O.eps_net(w, cfg, xr, torch.full((B, 1), 9.0)), xr, v)
    xd = x.to(dev).requires_grad_(True)
    (g,) = torch.autograd.grad(net.eps(xd, 9.0), xd, v.to(dev))
    assert rel(g.cpu(), g_ref) < 1e-4


def test_training_loss_matches_the_reference_golden(dev):
    """Loss and gradients against the REFERENCE's own training_loss + autograd (tests/golden/make_golden_train.py)."""
    gt = np.load(os.path.join(ROOT, "tests", "golden", "golden_train_v1.npz"))
    cfg = synth.mini_wavenet_config(32, 3, 12)
    net, _ = _net(cfg, dev, seed=0)
    loss, g = native_step(net, torch.from_numpy(gt["x"]), torch.from_numpy(gt["z"]), gt["steps"].tolist(), dev)
    check_against_golden(gt, loss, g)


def test_three_sgd_steps_follow_the_float64_oracle(dev):
    """lr = 0.05, no momentum, a fixed batch of the first net above.  Per tensor theta_3 - theta_0 agrees to 3e-4 of max|delta_ref|
    (floor as for the gradients: three summed gradients, each held to 1e-4), the native loss falls, and the re-fold after
    optimizer.step() is picked up (else steps 2 and 3 would repeat step 1's gradient)."""
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams, training_loss
    C_, NL, L, B, steps = TRAIN_CASES[0]
    cfg = synth.mini_wavenet_config(C_, NL, 12)
    net, sd = _net(cfg, dev, seed=4)
    x = torch.from_numpy(synth.waveforms(B, L, seed=31))
    z = torch.from_numpy(synth.noise(0, B, L, seed=31))
    lr = 0.05
    leaves = T.leaves_of(sd, torch.float64)
    for _ in range(3):
        loss = T.oracle_loss(leaves, cfg, x, z, steps, torch.float64)
        names = list(leaves)
        gs = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
        leaves = {k: (v.detach() - lr * g if g is not None else v.detach()).requires_grad_(True) for k, v, g in zip(names, leaves.values(), gs)}
    dh = calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG)
    src = (torch.tensor(steps), z.to(dev))
    theta0 = {k: p.detach().clone() for k, p in net.named_parameters()}
    opt = torch.optim.SGD(net.parameters(), lr=lr)
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss = training_loss(net, torch.nn.MSELoss(), x.to(dev), dh, noise_source=src)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        losses.append(training_loss(net, torch.nn.MSELoss(), x.to(dev), dh, noise_source=src).item())
    print("native losses", losses)
    assert losses[3] < losses[0]
    delta_ref = {k: leaves[k].detach() - torch.from_numpy(np.asarray(sd[k])).double() for k in leaves}
    D = max(float(d.abs().max()) for d in delta_ref.values())
    for k, p in net.named_parameters():
        T.check_tensor(k, (p.detach() - theta0[k]).cpu(), delta_ref[k], D, rel=3e-4)


# ---- 6. refusals ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32s", "bf16", "bf16s"])
def test_training_loss_refuses_the_other_precision_modes_before_any_launch(dev, mode):
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams, training_loss
    cfg = synth.mini_wavenet_config(256, 3, 12)
    net, _ = _net(cfg, dev)
    net.set_precision(mode)
    dh = calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG)
    x = torch.from_numpy(synth.waveforms(2, 256, seed=1)).to(dev)
    with pytest.raises(N.NativeError, match=repr(mode)):
        training_loss(net, torch.nn.MSELoss(), x, dh)
    assert net._engine is None                                    # no context was even built: nothing was launched
    assert all(p.grad is None for p in net.parameters())


def test_backward_without_param_grads_returns_the_same_bits(dev):
    """param_grads=None is the call as it always was; with a ParamGrads the input gradient is still those bits."""
    from audiopure_amd.diffusion_models._grad import EpsGrad, ParamGrads
    for C_ in (64, 256):
        cfg = synth.mini_wavenet_config(C_, 3, 12)
        net, _ = _net(cfg, dev, seed=5)
        x = torch.from_numpy(synth.waveforms(2, 640, seed=11)).to(dev)
        v = U("pgv", (2, 1, 640)).to(dev)
        eg = EpsGrad(net)
        _, saved = eg.forward_save(x, 9.0)
        a = eg.backward(saved, v)
        b = eg.backward(saved, v, None)
        c = eg.backward(saved, v, param_grads=ParamGrads(net).at(x, 9.0))
        assert torch.equal(a, b) and torch.equal(a, c)
