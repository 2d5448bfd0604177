"""Input gradient of the purification chain.

The reference's white-box adaptive attack back-propagates a loss through the defender
(``robustness_eval/white_box_attack.py:392,437-439``; the scripts build ``RevDiffWave`` whose
``torchsde.sdeint_adjoint`` re-integrates backwards, ``diffusion_models/diffwave_sde.py:200-204``).
Every sampler here is a chain of links ``x <- ca x + cb eps(x, t) + cs z`` (``ap_step``), so the gradient is

    dL/dx_t = ca dL/dx_{t-1} + cb J_eps(x_t, t)^T dL/dx_{t-1}

with the states x_t check-pointed in the forward pass.  A link's 37 layer inputs are kept for the backward pass while the
chain fits a memory budget (``SAVE_BUDGET_BYTES``; 288 GB of HBM hold a PGD batch comfortably) and recomputed otherwise
(the adjoint's memory/compute trade).

``J_eps^T v`` runs on the HIP library.  Which forward sweep a link runs, what it keeps and which backward reads that is
decided in one place, ``_link_plan`` (the table of kernels per arithmetic mode is its docstring).  Gradients with respect
to the network's parameters are not formed (the attack differentiates with respect to the audio only; parameters
are frozen at evaluation, ``adaptive_attack_eval.py:98-101``).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from .. import _native as N

_RS = 0.707106781186547524
_F1D = 0x200                      # AP_CONV_1D


class _LinkPlan(NamedTuple):
    """One link's saving forward, as ``_link_plan`` decides it."""
    sweep: str                    # "block": ap_resblock_fwd[_save] per layer; "gate": ap_resblock_fwd_gate[_save] on fp32 tensors
    #                               + ap_skip_gemm per group; "u": ap_resblock_fwd_u_save on u images + ap_skip_gemm per group
    keeps: Optional[str]          # besides layer inputs: "pre_gate", "gate_factors" or None
    backward: str                 # what serves the save while the flags stay: "f32", "bf16_saved", "bf16" (see _backward_form) or "composed"
    slots: int                    # residual-stream slots: NL + 1 (every layer's input), 3 (h_0 + a ping-pong pair) or 1 (h_0; the u pair is the sweep's own)
    group: int                    # layers per skip GEMM (0 in the "block" sweep)
    dims: tuple                   # (B, C, S, L, NL, embed_dim_out, gate factor bytes per layer)

    def io(self, n: int):
        """(slot layer n reads, slot it writes its h' / u_out to); "u" sweep: slots of its pair of u images."""
        if self.keeps != "gate_factors":
            return n, n + 1
        return (n & 1, (n + 1) & 1) if self.sweep == "u" else (0 if n == 0 else 1 + ((n - 1) & 1), 1 + (n & 1))


def _backward_form(precision, pre_gate: bool, gate_factors: bool, fused_bf16, bwd_f32_available, bwd_bf16_available) -> str:
    """Which per-layer backward serves a save holding these things (res = skip = 256 channels wherever *_available says yes):
    "f32"        ap_resblock_bwd from kept pre-gate activations: the gate's derivative behind W2^T [dh'; dskip], then the transposed
                 dilated conv in F(2,3) form with the residual path in its epilogue -- the forward block's flops, no glue;
    "bf16_saved" ap_resblock_bwd_bf16_saved from kept gate derivative factors (bf16 and bf16-storage modes): no recomputation;
    "bf16"       ap_resblock_bwd_bf16 from the layer inputs, the dilated conv recomputed inside its first kernel;
    "composed"   every other shape / mode: the recomputed dilated conv (unless pre-gate activations were kept), W2^T [dh'; dskip] and
                 the transposed dilated conv as ap_conv2d_fwd calls in AP_CONV_1D mode, ap_gate_bwd between them."""
    if gate_factors:
        return "bf16_saved"
    if pre_gate:
        return "f32" if precision == N.AP_PREC_F32 and bwd_f32_available else "composed"
    return "bf16" if fused_bf16 and precision == N.AP_PREC_BF16 and bwd_bf16_available else "composed"


def _link_plan(precision, C, S, NL, embed_dim_out, B, L, acts, keep_gate_factors, fused_bf16, group, bwd_f32_available,
               bwd_bf16_available, factor_bytes) -> _LinkPlan:
    """The one decision per link, from plain values (``group``: NativeEngine.deferred_skip_group(); the two ``*_available`` and
    ``factor_bytes``: the library's answers for this (B, L)):
      fp32, C in (64, 256), acts   "block" sweep with ap_resblock_fwd_save, keeps the pre-gate activations (3x the memory; the
                                   backward skips the dilated conv's recomputation)
      bf16, factors kept (default) "gate" sweep with ap_resblock_fwd_gate_save, keeps the gate's derivative factors (16.4 MB per
                                   clip-second and layer) and of the layer inputs only the first
      bf16 otherwise               "gate" sweep (group > 0: the form ap_eps_fwd runs, same eps bit for bit) or "block" sweep
      bf16 storage                 "u" sweep, always with factors: no lean form (no fp32 layer inputs exist to recompute from), so
                                   acts=False gives the full form; a shape without that backward is an error
      everything else              "block" sweep with ap_resblock_fwd, layer inputs only."""
    bf16_modes = (N.AP_PREC_BF16, N.AP_PREC_BF16_STORE)
    group = int(group) if precision in bf16_modes else 0
    if precision == N.AP_PREC_BF16_STORE:
        if group <= 0 or not bwd_bf16_available:
            raise N.NativeError("set_precision('bf16s'): no backward for this shape (res = skip = 256 channels, the deferred-skip form)")
        sweep, keeps, slots = "u", "gate_factors", 1
    elif acts and fused_bf16 and keep_gate_factors and group > 0 and bwd_bf16_available:
        sweep, keeps, slots = "gate", "gate_factors", 3
    else:
        sweep, slots = "gate" if group > 0 else "block", NL + 1
        keeps = "pre_gate" if acts and precision == N.AP_PREC_F32 and C in (64, 256) else None
    form = _backward_form(precision, keeps == "pre_gate", keeps == "gate_factors", fused_bf16, bwd_f32_available, bwd_bf16_available)
    return _LinkPlan(sweep, keeps, form, slots, group, (B, C, S, L, NL, embed_dim_out, int(factor_bytes)))


def _link_buffers(plan: _LinkPlan):
    """(the buffers a link keeps as [(field of _Saved, shape, dtype)], the gate-image buffer the sweep needs as (shape, dtype) or
    None): what forward_save allocates and saved_bytes sums.  The gate images live in ONE buffer per EpsGrad, reused by every
    link (295 MB per clip-second at group = 36)."""
    B, C, S, L, NL, E, fbytes = plan.dims
    keep = [("hs", (plan.slots, B, C, L), torch.float32), ("skip", (B, S, L), torch.float32), ("part", (NL * C + E,), torch.float32)]
    if plan.keeps == "pre_gate":
        keep.append(("pre_gate", (NL, B, 2 * C, L), torch.float32))
    if plan.keeps == "gate_factors":
        keep.append(("gate_factors", (NL, fbytes), torch.uint8))       # (an opaque image per layer)
    gimg = ((min(plan.group, NL) * B * L * C,), torch.bfloat16) if plan.group > 0 else None
    return keep, gimg


def _nbytes(shape, dtype) -> int:
    return math.prod(shape) * dtype.itemsize


class _Saved(NamedTuple):
    """What forward_save keeps for backward."""
    hs: torch.Tensor                                   # [slots][B][C][L] layer inputs (hs[0] = h_0 always)
    skip: torch.Tensor                                 # [B][S][L] skip sum
    part: torch.Tensor                                 # FiLM vectors of every layer, then the step embedding
    pre_gate: Optional[torch.Tensor] = None            # [NL][B][2C][L]
    gate_factors: Optional[torch.Tensor] = None        # [NL][ap_gate_factor_bytes(B, L)] uint8

    def lean(self) -> "_Saved":
        """The same evaluation without the pre-gate activations (its backward recomputes the dilated conv)."""
        return self._replace(pre_gate=None)


class EpsGrad:
    """Backward weights of one WaveNet_Speech_Commands plus eps forward-with-save / backward."""

    def __init__(self, net):
        self.net = net
        self._key = None
        self._gimg = None               # bf16 mode: the group's gate images of forward_save, one buffer reused by every link
        self.keep_gate_factors = True   # bf16 mode: keep the gate's derivative factors in the forward pass (False: recompute the dilated conv in the backward)
        self.fused_bf16 = True          # tools/check_bwd_bf16.py turns it off to time / compare the composed fp32 backward in bf16 mode

    # ---- weights ---------------------------------------------------------------------------------------
    def _prepare(self):
        net = self.net
        eng = net.engine()
        key = (eng.serial, eng.loaded_key, net._precision)   # (serial, not id(): a precision switch builds a new engine, possibly at the old one's address)
        if self._key == key:
            return eng
        lib, dev = eng.lib, next(net.parameters()).device
        C_, S_, NL = eng.cfg.res_channels, eng.cfg.skip_channels, eng.cfg.num_res_layers
        cyc = eng.cfg.dilation_cycle
        if net._precision == N.AP_PREC_BF16_STORE and not (C_ == 256 and S_ == 256):
            raise N.NativeError("set_precision('bf16s') (AP_PREC_BF16_STORE) needs res = skip = 256 channels")
        if C_ == 256 and S_ == 256 and net._precision in (N.AP_PREC_F32, N.AP_PREC_BF16, N.AP_PREC_BF16_STORE):
            # the fused backward kernels' own weight images: built here, once per load, outside any stream capture (the launch
            # functions allocate nothing: include/audiopure.h, ap_ctx_prepare_backward)
            N.check(lib.ap_ctx_prepare_backward(eng.ctx, N.stream()), "ap_ctx_prepare_backward")

        def folded(which, layer, n):
            t = torch.empty(n, device=dev, dtype=torch.float32)
            N.check(lib.ap_ctx_get_folded(eng.ctx, which, layer, N.ptr(t), n, N.stream()), "ap_ctx_get_folded")
            return t

        def pack(w4):                                           # [Cout][Cin][kh][kw] -> packed images
            w4 = w4.contiguous()
            co, ci, kh, kw = w4.shape
            out = torch.empty(lib.ap_conv2d_packed_elems(co, ci, kh, kw, 1), device=dev, dtype=torch.float32)
            N.check(lib.ap_conv2d_pack(N.ptr(w4), None, N.ptr(out), co, ci, kh, kw, 1, N.stream()), "ap_conv2d_pack")
            return out

        self.layers = []
        blocks = net.residual_layer.residual_blocks
        for n in range(NL):
            w1 = folded(0, n, 2 * C_ * C_ * 3).reshape(2 * C_, C_, 1, 3)
            w2 = torch.cat([folded(1, n, C_ * C_).reshape(C_, C_), folded(2, n, S_ * C_).reshape(S_, C_)], 0)   # [(C+S)][C]
            self.layers.append(dict(
                d=2 ** (n % cyc),
                a=pack(w1),                                                           # u -> pre-gate a   (C -> 2C, k=3, dil d)
                g=pack(w2.t().reshape(C_, C_ + S_, 1, 1)),                            # [RS dh'; dskip] -> dg  (C+S -> C, 1x1)
                u=pack(w1.flip(3).permute(1, 0, 2, 3)),                               # da -> du   (2C -> C, k=3 flipped, dil d)
                b1=blocks[n].dilated_conv_layer.conv.bias.detach().float().contiguous()))
        s = float(torch.tensor(math.sqrt(1.0 / NL), dtype=torch.float32))             # WaveNet.py:135
        wf1 = folded(3, 0, S_ * S_).reshape(S_, S_) * s
        self.wf1 = pack(wf1.reshape(S_, S_, 1, 1))                                    # skip_sum -> r (scale folded in)
        self.wf1_t = pack(wf1.t().reshape(S_, S_, 1, 1))                              # dr -> dskip
        self.bf1 = net.final_conv[0].conv.bias.detach().float().contiguous()
        self.wf2 = net.final_conv[2].conv.weight.detach().float().reshape(-1).contiguous()
        self.w0 = folded(4, 0, C_)
        self.ones = torch.ones(C_, device=dev)
        self.C, self.S, self.NL = C_, S_, NL
        torch.cuda.synchronize(dev)
        self._key = key
        return eng

    def _conv(self, lib, x, packed, bias, res, out, B, Cin, L, Cout, kw, pad, dil, flags=0):
        if self.net._precision in (N.AP_PREC_F32_SPLIT, N.AP_PREC_BF16, N.AP_PREC_BF16_STORE):   # follow the network's arithmetic mode: the split GEMM (fp32-class
            flags |= 0x100                                       # results from the bf16 matrix pipe, AP_CONV_SPLIT) where the forward ran on that pipe too
        fl = flags | _F1D | ((dil << 16) if dil > 1 else 0)
        N.use_conv_workspace(x.device)                           # short clips meet the split-K condition: this device's buffer
        N.check(lib.ap_conv2d_fwd(N.ptr(x), N.ptr(packed), N.ptr(bias), N.ptr(res), N.ptr(out), B, Cin, 1, L, Cout, 1, kw, 1,
                                  pad, 1, fl, Cin, 0, N.stream()), "ap_conv2d_fwd")

    def _plan(self, eng, B, L, acts) -> _LinkPlan:
        lib, cfg = eng.lib, eng.cfg
        return _link_plan(self.net._precision, self.C, self.S, self.NL, cfg.embed_dim_out, B, L, acts, self.keep_gate_factors,
                          self.fused_bf16, eng.deferred_skip_group(), lib.ap_resblock_bwd_available(eng.ctx, B, L),
                          lib.ap_resblock_bwd_bf16_available(eng.ctx, B, L), lib.ap_gate_factor_bytes(B, L))

    def _ensure_gimg(self, gimg, dev, allocate=True) -> int:
        """Make the gate-image buffer hold ``gimg`` (of _link_buffers); the bytes newly allocated -- ``allocate=False``: the bytes
        it would allocate.  The buffer only grows and is reused by every link, so a chain is charged for it once."""
        if gimg is None or (self._gimg is not None and self._gimg.numel() >= gimg[0][0] and self._gimg.device == dev):
            return 0
        if allocate:
            self._gimg = None
            self._gimg = torch.empty(gimg[0], device=dev, dtype=gimg[1])
        return _nbytes(*gimg)

    def saved_bytes(self, x: torch.Tensor, acts: bool = True, split: bool = False):
        """Bytes ``forward_save(x, ., acts)`` keeps, computed without allocating (the sum of _link_buffers), plus the gate-image buffer
        while this object does not hold one of that size yet.  ``split``: the pair (bytes the link keeps, bytes of that one-off
        buffer) instead of their sum."""
        eng = self._prepare()
        keep, gimg = _link_buffers(self._plan(eng, x.shape[0], x.shape[2], acts))
        link, once = sum(_nbytes(shape, dtype) for _, shape, dtype in keep), self._ensure_gimg(gimg, x.device, allocate=False)
        return (link, once) if split else link + once

    def eps_only(self, x: torch.Tensor, step: float):
        """The plain fused forward (``ap_eps_fwd``): what the chain's forward pass calls -- nothing is kept."""
        with torch.no_grad():
            return self.net.eps(x.detach(), step)

    # ---- one eps evaluation, keeping what its backward needs ---------------------------------------------------
    def forward_save(self, x: torch.Tensor, step: float, acts: bool = True):
        """One eps evaluation that keeps what its backward needs: (eps, _Saved).  ``acts=False``: the lean form, layer inputs
        only, where the mode has one (_link_plan)."""
        eng = self._prepare()
        lib, ctx, dev, st = eng.lib, eng.ctx, x.device, N.stream()
        B, _, L = x.shape
        C_, NL = self.C, self.NL
        plan = self._plan(eng, B, L, acts)
        keep, gimg = _link_buffers(plan)
        saved = _Saved(**{name: torch.empty(shape, device=dev, dtype=dtype) for name, shape, dtype in keep})
        hs, skip, part, pre, fac = saved
        N.check(lib.ap_embed(ctx, float(step), N.ptr(part), st), "ap_embed")
        N.check(lib.ap_init_conv(ctx, N.ptr(x), N.ptr(hs[0]), B, L, st), "ap_init_conv")
        film = lambda n: N.ptr(part[n * C_:(n + 1) * C_])
        # the deferred-skip sweeps do not compute the last layer's h' / u_out (nobody reads it: hs[NL] stays unwritten and backward()
        # starts from dh = 0)
        if plan.sweep == "u":
            # the sweep ap_eps_fwd runs with bf16 storage (same eps bit for bit), every block also keeping its gate's derivative factors;
            # the rounding of the stored residual passes the gradient straight through, so the backward is the bf16 mode's
            u = torch.empty((2, B * C_ * L), device=dev, dtype=torch.bfloat16)   # the residual stream's ping-pong pair of u images
            N.check(lib.ap_init_conv_u(ctx, N.ptr(x), N.ptr(part[:C_]), u[0].data_ptr(), B, L, st), "ap_init_conv_u")

            def layer(n, g):
                last = n + 1 == NL
                src, dst = plan.io(n)
                N.check(lib.ap_resblock_fwd_u_save(ctx, n, u[src].data_ptr(), None if last else film(n + 1),
                                                   None if last else u[dst].data_ptr(), g, fac[n].data_ptr(), B, L, st),
                        "ap_resblock_fwd_u_save")
        elif plan.sweep == "gate":
            def layer(n, g):
                src, dst = plan.io(n)
                h_in, h_out = N.ptr(hs[src]), N.ptr(hs[dst]) if n + 1 < NL else None
                if fac is not None:
                    N.check(lib.ap_resblock_fwd_gate_save(ctx, n, h_in, film(n), h_out, g, fac[n].data_ptr(), B, L, st), "ap_resblock_fwd_gate_save")
                else:
                    N.check(lib.ap_resblock_fwd_gate(ctx, n, h_in, film(n), h_out, g, B, L, st), "ap_resblock_fwd_gate")
        else:
            def layer(n, g):
                if pre is not None:
                    N.check(lib.ap_resblock_fwd_save(ctx, n, N.ptr(hs[n]), film(n), N.ptr(hs[n + 1]), N.ptr(skip), N.ptr(pre[n]),
                                                     1 if n else 0, B, L, st), "ap_resblock_fwd_save")
                else:
                    N.check(lib.ap_resblock_fwd(ctx, n, N.ptr(hs[n]), film(n), N.ptr(hs[n + 1]), N.ptr(skip), 1 if n else 0, B, L, st),
                            "ap_resblock_fwd")
        if gimg is None:                                         # the fused block adds its own skip term
            for n in range(NL):
                layer(n, None)
        else:                                                    # one skip GEMM per group of G layers, grouped as ap_eps_fwd groups them
            self._ensure_gimg(gimg, dev)
            G = min(plan.group, NL)
            images = self._gimg[:gimg[0][0]].view(G, B, L, C_)
            for n0 in range(0, NL, G):
                nl = min(G, NL - n0)
                for n in range(n0, n0 + nl):
                    layer(n, images[n - n0].data_ptr())
                N.check(lib.ap_skip_gemm(ctx, n0, nl, images.data_ptr(), N.ptr(skip), 1 if n0 else 0, B, L, st), "ap_skip_gemm")
        eps = torch.empty((B, 1, L), device=dev)
        N.check(lib.ap_final_affine(ctx, N.ptr(skip), None, N.ptr(eps), None, 0.0, 0.0, 0.0, None, 0, 0, 0, B, L, st), "ap_final_affine")
        return eps, saved

    def backward(self, saved, d_eps: torch.Tensor) -> torch.Tensor:
        """J_eps(x, t)^T d_eps for the evaluation ``saved`` came from; the per-layer form follows what the save holds and the flags
        as they are now (_backward_form)."""
        eng = self._prepare()
        lib, ctx = eng.lib, eng.ctx
        hs, skip, part, pre, fac = saved
        NL, C_, S_ = self.NL, self.C, self.S
        B, L, dev = hs.shape[1], hs.shape[3], hs.device
        d_eps = d_eps.detach().float().contiguous()
        st = N.stream()
        # final_conv: r = W_f1 (skip s) + b_f1; eps = w_f2 . relu(r) + b_f2
        r = torch.empty((B, S_, L), device=dev)
        self._conv(lib, skip, self.wf1, self.bf1, None, r, B, S_, L, S_, 1, 0, 1)
        dr = torch.empty_like(r)
        N.check(lib.ap_relu_outer_bwd(N.ptr(r), N.ptr(self.wf2), N.ptr(d_eps), N.ptr(dr), B, S_, L, st), "ap_relu_outer_bwd")
        dskip = r                                                 # reuse
        self._conv(lib, dr, self.wf1_t, None, None, dskip, B, S_, L, S_, 1, 0, 1)
        dh = torch.zeros((B, C_, L), device=dev)                  # the last block's h' output is not used (WaveNet.py:133)
        form = _backward_form(self.net._precision, pre is not None, fac is not None, self.fused_bf16,
                              lib.ap_resblock_bwd_available(ctx, B, L), lib.ap_resblock_bwd_bf16_available(ctx, B, L))
        if form != "composed":                                    # two fused launches per layer, dh / dh2 ping-pong
            dy = torch.empty((B, 2 * C_, L), device=dev) if form == "f32" else torch.empty((B, L, 2 * C_), device=dev, dtype=torch.bfloat16)
            dh2 = torch.empty_like(dh)
            if form == "f32":
                def layer(n, dh, dh2):
                    N.check(lib.ap_resblock_bwd(ctx, n, N.ptr(dh), N.ptr(dskip), N.ptr(pre[n]), N.ptr(dy), N.ptr(dh2), B, L, st), "ap_resblock_bwd")
            elif form == "bf16_saved":                            # dg = W2^T [dh'; dskip], dy = factor . dg, then the transposed dilated conv
                dsk = torch.empty((B, L, S_), device=dev, dtype=torch.bfloat16)  # dskip once as the bf16 image every layer's kernel stages
                N.check(lib.ap_bwd_bf16_rows_image(N.ptr(dskip), dsk.data_ptr(), B, S_, L, st), "ap_bwd_bf16_rows_image")

                def layer(n, dh, dh2):
                    N.check(lib.ap_resblock_bwd_bf16_saved(ctx, n, fac[n].data_ptr(), N.ptr(dh), dsk.data_ptr(), 1, dy.data_ptr(), N.ptr(dh2),
                                                           B, L, st), "ap_resblock_bwd_bf16_saved")
            else:                                                 # from the layer INPUTS the forward pass wrote anyway
                def layer(n, dh, dh2):
                    N.check(lib.ap_resblock_bwd_bf16(ctx, n, N.ptr(hs[n]), N.ptr(part[n * C_:(n + 1) * C_]), N.ptr(dh), N.ptr(dskip),
                                                     dy.data_ptr(), N.ptr(dh2), B, L, st), "ap_resblock_bwd_bf16")
            for n in range(NL - 1, -1, -1):
                layer(n, dh, dh2)
                dh, dh2 = dh2, dh
        else:
            z = torch.empty((B, C_ + S_, L), device=dev)         # [RS dh' ; dskip], dskip is the same for every block
            N.check(lib.ap_copy_channels(N.ptr(dskip), N.ptr(z), B, S_, L, S_, 0, C_ + S_, C_, st), "ap_copy_channels")
            t1 = torch.empty_like(dh)
            dg = torch.empty_like(dh)
            u = torch.empty_like(dh) if pre is None else None
            a = torch.empty((B, 2 * C_, L), device=dev) if pre is None else None
            da = torch.empty((B, 2 * C_, L), device=dev)
            nel = dh.numel()
            for n in range(NL - 1, -1, -1):
                lay = self.layers[n]
                d = lay["d"]
                N.check(lib.ap_axpbyc(N.ptr(dh), None, N.ptr(t1), _RS, 0.0, 0.0, nel, st), "ap_axpbyc")
                N.check(lib.ap_copy_channels(N.ptr(t1), N.ptr(z), B, C_, L, C_, 0, C_ + S_, 0, st), "ap_copy_channels")
                self._conv(lib, z, lay["g"], None, None, dg, B, C_ + S_, L, C_, 1, 0, 1)
                if pre is None:                                      # not kept: recompute y = DilConv(h + part_t) + b
                    pt = part[n * C_:(n + 1) * C_]
                    N.check(lib.ap_affine_nchw(N.ptr(hs[n]), N.ptr(self.ones), N.ptr(pt), N.ptr(u), B, C_, L, C_, 0, 0, st),
                            "ap_affine_nchw")
                    self._conv(lib, u, lay["a"], lay["b1"], None, a, B, C_, L, 2 * C_, 3, d, d)
                N.check(lib.ap_gate_bwd(N.ptr(a if pre is None else pre[n]), N.ptr(dg), N.ptr(da), B, C_, L, st), "ap_gate_bwd")
                self._conv(lib, da, lay["u"], None, t1, dh, B, 2 * C_, L, C_, 3, d, d)
        dx = torch.empty((B, 1, L), device=dev)
        N.check(lib.ap_init_conv_bwd(N.ptr(hs[0]), N.ptr(self.w0), N.ptr(dh), N.ptr(dx), B, C_, L, st), "ap_init_conv_bwd")
        return dx


def _axpby(x, y, a, b):
    """a x + b y on the library (``ap_axpbyc``); y None -> a x.  Shapes may differ as long as the element counts agree."""
    x = x if x.is_contiguous() else x.contiguous()
    if y is not None:
        y = y.float()
        y = y if y.is_contiguous() else y.contiguous()
        assert y.numel() == x.numel()
    out = torch.empty_like(x)
    N.check(N.lib().ap_axpbyc(N.ptr(x), N.ptr(y), N.ptr(out), float(a), float(b) if y is not None else 0.0, 0.0, x.numel(),
                              N.stream()), "ap_axpbyc")
    return out


SAVE_BUDGET_BYTES = 96 << 30      # ceiling per chain of what the links keep for the backward pass (288 GB of HBM)
SAVE_FREE_FRACTION = 0.6          # ... and never more than this share of the device memory that is free when the chain starts


def _chain_budget(device) -> int:
    """What one chain may keep: the ceiling, capped by a share of the memory that is actually free (several chains -- EOT
    samples, sample_step > 1 -- start one after the other, each seeing what the earlier ones hold)."""
    try:
        free, _ = torch.cuda.mem_get_info(device)
        # blocks torch's caching allocator holds but has free are as reusable as driver-free memory: after the first chain of a
        # PGD loop tens of GB sit there, and counting only the driver's figure would shrink every later chain's budget
        free += max(torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device), 0)
    except (RuntimeError, AssertionError):
        return SAVE_BUDGET_BYTES
    return int(min(SAVE_BUDGET_BYTES, SAVE_FREE_FRACTION * free))


def _saved_bytes(saved) -> int:
    n = 0
    stack = [saved]
    while stack:
        o = stack.pop()
        if isinstance(o, torch.Tensor):
            n += o.numel() * o.element_size()
        elif isinstance(o, (tuple, list)):
            stack.extend(o)
        elif isinstance(o, dict):
            stack.extend(o.values())
    return n


def _save_level(held, once, full, lean, budget):
    """What the next link of a chain keeps: ("full", "lean" or None, held', once').  ``held``: bytes the earlier links keep;
    ``once``: a buffer the first saving link allocates and every later one reuses, so it is charged to that link only."""
    if held + once + full <= budget:
        return "full", held + once + full, 0
    if lean < full and held + once + lean <= budget:
        return "lean", held + once + lean, 0
    return None, held, once


class _ChainFn(torch.autograd.Function):
    """x_out = chain(x_in): q-sample then the links (step, ca, cb, cs); noise tensors given explicitly.

    Every elementwise update is an ``ap_axpbyc`` call.  A link's eps-evaluation keeps its per-layer inputs and (fp32
    arithmetic) pre-gate activations for the backward pass while the chain's total stays under ``SAVE_BUDGET_BYTES`` (one
    evaluation of the shipped net is 1.8 GB per clip that way, 0.6 GB with the layer inputs only: a PGD batch of 8 clips x
    5 links is 72 GB of the 288); past the budget a link keeps the layer inputs only (its backward recomputes the dilated
    conv), then only the state entering it (the evaluation is recomputed in the backward pass: the adjoint's trade)."""

    @staticmethod
    def forward(ctx, x, grad, steps, qa, qs, zs):
        """zs[k] = draw k of the chain ([B,1,L] or [B,L]); draw 0 is the q-sample's (the numbering of ap_purify_chain)."""
        xs, saves, held = [], [], 0
        cur = x.detach().float().contiguous()
        eps_only = getattr(grad, "eps_only", None)
        with torch.no_grad():
            if qs != 0.0:
                cur = _axpby(cur, zs[0], qa, qs)
            elif qa != 1.0:
                cur = _axpby(cur, None, qa, 0.0)
            budget = _chain_budget(cur.device)
            sizes = getattr(grad, "saved_bytes", None)           # analytic sizes where the gradient object knows them: nothing is
            full = lean = None                                   # allocated to find out that it does not fit
            once = 0                                             # (a buffer the first saving link allocates and every later one reuses)
            if sizes:
                full, once = sizes(cur, True, split=True)
                lean, _ = sizes(cur, False, split=True)
            for (t, ca, cb, cs, draw) in steps:
                xs.append(cur)
                saved = None
                if full is None:                                 # (a gradient object without sizes: measure its first link)
                    eps, saved = grad.forward_save(cur, t)
                    lean_saved = saved.lean() if hasattr(saved, "lean") else saved   # (no lean(): no lean form)
                    full, lean = _saved_bytes(saved), _saved_bytes(lean_saved)
                    level, held, once = _save_level(held, once, full, lean, budget)
                    saved = {"full": saved, "lean": lean_saved, None: None}[level]
                else:
                    level, held, once = _save_level(held, once, full, lean, budget)
                    if level is None:
                        eps = eps_only(cur, t) if eps_only is not None else grad.forward_save(cur, t)[0]
                    else:                                        # "lean": layer inputs only, the backward recomputes the dilated conv
                        eps, saved = grad.forward_save(cur, t) if level == "full" else grad.forward_save(cur, t, acts=False)
                saves.append(saved)
                nxt = _axpby(cur, eps, ca, cb)
                if cs != 0.0 and draw:
                    nxt = _axpby(nxt, zs[draw], 1.0, cs)
                cur = nxt
        ctx.grad, ctx.steps, ctx.qa, ctx.xs, ctx.saves = grad, steps, qa, xs, saves
        return cur

    @staticmethod
    def backward(ctx, g):
        g = g.detach().float().contiguous()
        with torch.no_grad():
            for k in range(len(ctx.steps) - 1, -1, -1):
                (t, ca, cb, cs, draw), xt = ctx.steps[k], ctx.xs[k]
                saved = ctx.saves[k]
                ctx.saves[k] = None
                if saved is None:                                # over budget in the forward pass: recompute this link -- with the
                    sizes = getattr(ctx.grad, "saved_bytes", None)   # pre-gate activations only if they fit what is free NOW
                    lean_only = sizes is not None and sizes(xt, True) > _chain_budget(xt.device)
                    _, saved = ctx.grad.forward_save(xt, t, acts=False) if lean_only else ctx.grad.forward_save(xt, t)
                g = _axpby(g, ctx.grad.backward(saved, g), ca, cb)
                del saved
            if ctx.qa != 1.0:
                g = _axpby(g, None, ctx.qa, 0.0)
        return g, None, None, None, None, None


class _EpsFn(torch.autograd.Function):
    """eps_theta(x, t) with its input gradient (the reference's network is plain differentiable torch, WaveNet.py:164-172)."""

    @staticmethod
    def forward(ctx, x, grad, step):
        with torch.no_grad():
            eps, saved = grad.forward_save(x.detach().float().contiguous(), step)
        ctx.grad, ctx.saved = grad, saved
        return eps

    @staticmethod
    def backward(ctx, g):
        with torch.no_grad():
            dx = ctx.grad.backward(ctx.saved, g.detach().float().contiguous())
        ctx.saved = None
        return dx, None, None


def _eps_grad_of(net):
    if getattr(net, "_eps_grad", None) is None or net._eps_grad.net is not net:
        net._eps_grad = EpsGrad(net)
    return net._eps_grad


def differentiable_chain(net, x, steps, qa, qs, zs):
    """The sampling chain as an autograd node (gradient with respect to ``x`` only)."""
    return _ChainFn.apply(x, _eps_grad_of(net), list(steps), float(qa), float(qs), zs)


def differentiable_eps(net, x, step):
    return _EpsFn.apply(x, _eps_grad_of(net), float(step))
