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
decided in one place, ``_link_plan`` (the table of kernels per arithmetic mode is its docstring).  The attack differentiates
with respect to the audio only (parameters are frozen at evaluation, ``adaptive_attack_eval.py:98-101``), so the chain forms
no parameter gradients.

Training does (``DiffWave_Unconditional/util.py:161-185`` ``training_loss``, then ``loss.backward()`` in ``train.py``):
``EpsGrad.backward(saved, d_eps, param_grads)`` contracts, in the same sweep, every cotangent it forms with the activation
it belongs to -- ``ap_wgrad_corr`` for the conv weights, ``ap_rowsum`` for the biases, the FiLM vectors, the init conv and
``final_conv.2``, ``ap_embed_bwd`` for the step-embedding MLP -- into a ``ParamGrads``, whose ``finish()`` takes the folded
weights' gradients back to ``weight_g`` / ``weight_v`` (``ap_weight_norm_bwd``).  ``training_eps`` is the autograd node over
(x_t, parameters) that ``util.training_loss`` calls.  fp32 arithmetic only.
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
                b1=net.pad_rows(blocks[n].dilated_conv_layer.conv.bias.detach().float(), 2).contiguous()))
        s = float(torch.tensor(math.sqrt(1.0 / NL), dtype=torch.float32))             # WaveNet.py:135
        wf1 = folded(3, 0, S_ * S_).reshape(S_, S_) * s
        self.wf1 = pack(wf1.reshape(S_, S_, 1, 1))                                    # skip_sum -> r (scale folded in)
        self.wf1_t = pack(wf1.t().reshape(S_, S_, 1, 1))                              # dr -> dskip
        self.bf1 = net.pad_rows(net.final_conv[0].conv.bias.detach().float()).contiguous()
        self.wf2 = net.pad_rows(net.final_conv[2].conv.weight.detach().float().reshape(-1)).contiguous()
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

    def backward(self, saved, d_eps: torch.Tensor, param_grads: "Optional[ParamGrads]" = None) -> torch.Tensor:
        """J_eps(x, t)^T d_eps for the evaluation ``saved`` came from; the per-layer form follows what the save holds and the flags
        as they are now (_backward_form).  ``param_grads``: also add this evaluation's parameter gradients to it (fp32 mode; the
        object must have been told the evaluation's input and step: ``ParamGrads.at``); None: the same launches as ever."""
        pg = param_grads
        if pg is not None:
            _require_f32(self.net, "EpsGrad.backward(param_grads=...)")
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
        if pg is not None:                                        # final_conv (WaveNet.py:160-162), before r is reused
            pg.begin(self, eng, B, L, dev)
            pg.rowsum(r, d_eps, r, pg.f2_w, B, S_, L, bcast=True)            # d f2.weight[s] = sum relu(r)[s] d_eps
            pg.rowsum(d_eps, None, None, pg.f2_b, B, 1, L)
            pg.rowsum(dr, None, None, pg.f1_b, B, S_, L)
            pg.corr(dr, skip, None, pg.f1_w, B, S_, S_, L, 1, 1, _WG_PLAIN, math.sqrt(1.0 / NL))   # d f1.weight = sum dr (x) (s skip)
        dskip = r                                                 # reuse
        self._conv(lib, dr, self.wf1_t, None, None, dskip, B, S_, L, S_, 1, 0, 1)
        if pg is not None:
            pg.rowsum(dskip, None, None, pg.skip_b, B, S_, L)     # d skip.bias: the same for every layer
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
                if pg is not None:                                # (fp32 form only: dy [B][2C][L] fp32, the gate from pre_gate[n])
                    pg.layer(n, self.layers[n]["d"], dy, hs[n], part[n * C_:(n + 1) * C_], dh, dskip, pre[n], dh2, B, L)
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
                if pg is not None:                                # dh still holds dh'; the conv below overwrites it with dh_in
                    pg.layer(n, d, da, hs[n], part[n * C_:(n + 1) * C_], dh, dskip, a if pre is None else pre[n], None, B, L)
                self._conv(lib, da, lay["u"], None, t1, dh, B, 2 * C_, L, C_, 3, d, d)
                if pg is not None:
                    pg.film(n, dh, B, L)
        dx = torch.empty((B, 1, L), device=dev)
        N.check(lib.ap_init_conv_bwd(N.ptr(hs[0]), N.ptr(self.w0), N.ptr(dh), N.ptr(dx), B, C_, L, st), "ap_init_conv_bwd")
        if pg is not None:
            pg.end(hs[0], dh, part[NL * C_:], B, L)
        return dx


_MODE_NAMES = {N.AP_PREC_F32: "f32", N.AP_PREC_BF16: "bf16", N.AP_PREC_F32_SPLIT: "f32s", N.AP_PREC_BF16_STORE: "bf16s"}
_WG_PLAIN, _WG_FILM, _WG_GATE = 0, 1, 2     # ap_wgrad_corr's staging modes


def _require_f32(net, who: str) -> None:
    """Parameter gradients exist in fp32 arithmetic only: refuse the other modes by name, before any launch."""
    if net._precision != N.AP_PREC_F32:
        raise N.NativeError(f"{who}: parameter gradients are built for set_precision('f32') / ('f32d') only; this network is in "
                            f"{_MODE_NAMES.get(net._precision, net._precision)!r} mode")


class ParamGrads:
    """fp32 device buffers shaped like the folded weights and the biases of one WaveNet_Speech_Commands, which
    ``EpsGrad.backward(saved, d_eps, param_grads)`` adds one evaluation's gradients to (always ``accumulate = 1`` onto zeros, so
    sub-batches add up in call order), and ``finish()``: the gradients of the parameters themselves, weight-norm unfolded."""

    def __init__(self, net):
        _require_f32(net, "ParamGrads")
        self.net = net
        cfg = net.config
        self.width = cfg["res_channels"]                                         # the parameters' own width; the buffers have the native one
        C_ = S_ = net.native_width()                                             # (the library is built for skip = res channels)
        NL = cfg["num_res_layers"]
        Ein, Emid, Eout = (cfg["diffusion_step_embed_dim_in"], cfg["diffusion_step_embed_dim_mid"], cfg["diffusion_step_embed_dim_out"])
        self.C, self.S, self.NL = C_, S_, NL
        dev = next(net.parameters()).device
        z = lambda *shape: torch.zeros(shape, device=dev, dtype=torch.float32)
        self.w0, self.b0 = z(C_), z(C_)                                          # init conv (folded [C][1])
        self.fc1_w, self.fc1_b, self.fc2_w, self.fc2_b = z(Emid, Ein), z(Emid), z(Eout, Emid), z(Eout)
        self.fct_w, self.fct_b = z(NL, C_, Eout), z(NL, C_)
        self.w1, self.b1 = z(NL, 2 * C_, C_, 3), z(NL, 2 * C_)                   # dilated conv (folded)
        self.res_w, self.res_b = z(NL, C_, C_), z(NL, C_)                        # (the last block's stay unused: WaveNet.py:133)
        self.skip_w, self.skip_b = z(NL, S_, C_), z(S_)                          # skip.bias: one sum serves every layer
        self.f1_w, self.f1_b, self.f2_w, self.f2_b = z(S_, S_), z(S_), z(S_), z(1)
        self.dpart = torch.zeros((NL, C_), device=dev, dtype=torch.float64)      # FiLM cotangents of the evaluation in flight (fp64: ap_embed_bwd)
        self._ws = self._scratch = self._x = self._step = None

    def at(self, x: torch.Tensor, step: float) -> "ParamGrads":
        """Name the evaluation the next ``EpsGrad.backward`` call belongs to: its input x [B,1,L] (the init conv's weight gradient
        needs it) and its step (the embedding MLP is recomputed from it)."""
        self._x, self._step = x.detach().float().contiguous(), float(step)
        return self

    # ---- called by EpsGrad.backward, in sweep order ---------------------------------------------------------
    def begin(self, grad, eng, B, L, dev):
        if self._x is None or tuple(self._x.shape) != (B, 1, L):
            raise N.NativeError("ParamGrads: call at(x, step) with this evaluation's input before EpsGrad.backward")
        self.lib, self.ctx = eng.lib, eng.ctx
        if self._scratch is None:
            self._scratch = torch.empty(self.lib.ap_embed_bwd_scratch_elems(self.ctx), device=dev, dtype=torch.float32)

    def corr(self, P, Q, film, G, B, M, Nn, L, taps, dil, mode, scale):
        need = self.lib.ap_wgrad_workspace_bytes(B, M, Nn, L, taps)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, device=P.device, dtype=torch.uint8)
        N.check(self.lib.ap_wgrad_corr(N.ptr(P), N.ptr(Q), N.ptr(film), N.ptr(G), self._ws.data_ptr(), self._ws.numel(), B, M, Nn, L,
                                       taps, dil, mode, float(scale), 1, N.stream()), "ap_wgrad_corr")

    def rowsum(self, A, W, R, out, B, M, L, bcast=False, scale=1.0, accumulate=1):
        N.check(self.lib.ap_rowsum(N.ptr(A), N.ptr(W), N.ptr(R), N.ptr(out), B, M, L, 1 if bcast else 0, float(scale), accumulate,
                                   N.stream()), "ap_rowsum")

    def layer(self, n, d, dy, h_in, film, dh_out, dskip, y, du, B, L):
        """Block n (WaveNet.py:75-97): dy = d loss / d (DilConv(u) + b), u = h_in + film; y: its pre-gate activations; dh_out =
        d loss / d h'; du = d loss / d u (None: handed to film() later)."""
        C_, S_ = self.C, self.S
        self.corr(dy, h_in, film, self.w1[n], B, 2 * C_, C_, L, 3, d, _WG_FILM, 1.0)
        self.rowsum(dy, None, None, self.b1[n], B, 2 * C_, L)
        if n + 1 < self.NL:                                       # the last block's h' is unused: no gradient, no launch
            self.corr(dh_out, y, None, self.res_w[n], B, C_, C_, L, 1, 1, _WG_GATE, _RS)
            self.rowsum(dh_out, None, None, self.res_b[n], B, C_, L, scale=_RS)
        self.corr(dskip, y, None, self.skip_w[n], B, S_, C_, L, 1, 1, _WG_GATE, 1.0)
        if du is not None:
            self.film(n, du, B, L)

    def film(self, n, du, B, L):
        N.check(self.lib.ap_rowsum_f64(N.ptr(du), self.dpart[n].data_ptr(), B, self.C, L, 0, N.stream()), "ap_rowsum_f64")   # dpart_n = sum du_n (this evaluation's alone)

    def end(self, h0, dh0, emb, B, L):
        self.rowsum(dh0, self._x, h0, self.w0, B, self.C, L, bcast=True)         # dw0[c] = sum dh0[c] [h0[c] > 0] x
        self.rowsum(dh0, None, h0, self.b0, B, self.C, L)
        N.check(self.lib.ap_embed_bwd(self.ctx, self._step, self.dpart.data_ptr(), N.ptr(emb), N.ptr(self.fct_w), N.ptr(self.fct_b),
                                      N.ptr(self.fc1_w), N.ptr(self.fc1_b), N.ptr(self.fc2_w), N.ptr(self.fc2_b), N.ptr(self._scratch), 1,
                                      N.stream()), "ap_embed_bwd")
        self._x = self._step = None

    # ---- after the sweep(s) ---------------------------------------------------------------------------
    def _unfold(self, dW, conv):
        """(d weight_g, d weight_v) of a weight-normed conv from the gradient of its folded weight."""
        g, v = conv.weight_g.detach(), conv.weight_v.detach()
        dg, dv = torch.empty_like(g), torch.empty_like(v)
        rows = v.shape[0]
        N.check(N.lib().ap_weight_norm_bwd(N.ptr(dW), N.ptr(v), N.ptr(g), N.ptr(dg), N.ptr(dv), rows, v.numel() // rows, N.stream()),
                "ap_weight_norm_bwd")
        return dg, dv

    def finish(self) -> list:
        """Gradients in the order of ``net._blob_tensors()`` (the state dict's); None for the last block's res_conv, as the
        reference's autograd leaves them."""
        net, NL, W, Cp = self.net, self.NL, self.width, self.C
        rows = lambda t: t[:W]                                                   # the real channels of a native-width buffer
        sq = lambda t: t[:W, :W].contiguous() if W != Cp else t
        halves = lambda t: torch.cat([t[:W], t[Cp:Cp + W]], 0)[:, :W].contiguous() if W != Cp else t   # tanh rows, sigmoid rows
        ic, f0 = net.init_conv[0].conv, net.final_conv[0].conv
        out = [rows(self.b0), *self._unfold(rows(self.w0), ic), self.fc1_w, self.fc1_b, self.fc2_w, self.fc2_b]
        for n, b in enumerate(net.residual_layer.residual_blocks):
            b1 = torch.cat([self.b1[n][:W], self.b1[n][Cp:Cp + W]]) if W != Cp else self.b1[n]
            out += [rows(self.fct_w[n]), rows(self.fct_b[n]), b1, *self._unfold(halves(self.w1[n]), b.dilated_conv_layer.conv)]
            out += [rows(self.res_b[n]), *self._unfold(sq(self.res_w[n]), b.res_conv)] if n + 1 < NL else [None, None, None]
            out += [rows(self.skip_b).clone(), *self._unfold(sq(self.skip_w[n]), b.skip_conv)]
        out += [rows(self.f1_b), *self._unfold(sq(self.f1_w), f0), rows(self.f2_w).reshape(1, -1, 1), self.f2_b]
        return out


def step_groups(steps) -> list:
    """Clips grouped by distinct step, as WaveNet_Speech_Commands.forward groups them: [(step, [clip indices ascending])], the
    groups in the order of their first clip."""
    groups = {}
    for i, t in enumerate(steps):
        groups.setdefault(float(t), []).append(i)
    return sorted(groups.items(), key=lambda kv: kv[1][0])


def plan_sub_batches(steps, bytes_of, budget) -> list:
    """The eps evaluations of one training step: [(step, [clip indices])].  Every group of ``step_groups`` is cut into runs of the
    largest clip count k whose save fits (``bytes_of(k) <= budget``, ``bytes_of`` non-decreasing; one clip always goes), in
    ascending clip order -- so every clip is evaluated exactly once whatever the budget.  Pure host logic."""
    out = []
    for t, idx in step_groups(steps):
        lo, hi = 1, len(idx)                                     # largest k in [1, len] that fits (k = 1 regardless)
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if bytes_of(mid) <= budget else (lo, mid - 1)
        out += [(t, idx[s:s + lo]) for s in range(0, len(idx), lo)]
    return out


class _TrainEpsFn(torch.autograd.Function):
    """eps_theta(x_t, steps) with per-clip steps, differentiable in x_t and in the network's parameters (``params``: exactly
    ``net._blob_tensors()``, handed over so that autograd routes their gradients).  One saving forward per sub-batch of
    ``plan_sub_batches``; a sub-batch's save is kept for the backward pass while the total fits the budget (``_save_level``, as a
    chain's links) and recomputed otherwise; the backward pass walks the sub-batches in the same order into one ParamGrads."""

    @staticmethod
    def forward(ctx, x_t, grad, steps, *params):
        x = x_t.detach().float().contiguous()
        eps = torch.empty_like(x)
        budget = _chain_budget(x.device)
        batches = plan_sub_batches(steps, lambda k: grad.saved_bytes(x[:k], True), budget)
        saves, held, once = [], 0, 0
        with torch.no_grad():
            for t, idx in batches:
                sel = torch.tensor(idx, device=x.device)
                xs = x[sel]
                full, first = grad.saved_bytes(xs, True, split=True)
                e, saved = grad.forward_save(xs, t)
                level, held, once = _save_level(held, max(once, first), full, full, budget)
                saves.append(saved if level is not None else None)
                eps[sel] = e
                del saved
        ctx.grad, ctx.batches, ctx.saves, ctx.x = grad, batches, saves, x
        return eps

    @staticmethod
    def backward(ctx, g):
        grad, x = ctx.grad, ctx.x
        g = g.detach().float().contiguous()
        dx = torch.empty_like(x)
        with torch.no_grad():
            pg = ParamGrads(grad.net)
            for k, (t, idx) in enumerate(ctx.batches):
                sel = torch.tensor(idx, device=x.device)
                xs = x[sel]
                saved, ctx.saves[k] = ctx.saves[k], None
                if saved is None:                                # over budget in the forward pass: the adjoint's trade
                    _, saved = grad.forward_save(xs, t)
                dx[sel] = grad.backward(saved, g[sel], pg.at(xs, t))
                del saved
            grads = pg.finish()
        return (dx, None, None, *grads)


class _QSampleFn(torch.autograd.Function):
    """x_t = sqrt(abar[t_b]) X_b + sqrt(1 - abar[t_b]) z_b per clip (util.py:183), ``ap_affine_noise`` per group of clips sharing a step."""

    @staticmethod
    def forward(ctx, X, z, groups):
        x = X.detach().float().contiguous()
        B, _, L = x.shape
        out = torch.empty_like(x)
        with torch.no_grad():
            for (ca, cs), idx in groups:
                sel = torch.tensor(idx, device=x.device)
                xs, zs = x[sel], z[sel]
                o = torch.empty_like(xs)
                N.check(N.lib().ap_affine_noise(N.ptr(xs), N.ptr(o), float(ca), float(cs), N.ptr(zs), 0, 0, 0, len(idx), L, N.stream()),
                        "ap_affine_noise")
                out[sel] = o
        ctx.groups = groups
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.detach().float().contiguous()
        dX = torch.empty_like(g)
        with torch.no_grad():
            for (ca, _), idx in ctx.groups:
                sel = torch.tensor(idx, device=g.device)
                dX[sel] = _axpby(g[sel], None, ca, 0.0)
        return dX, None, None


def q_sample_per_clip(X, z, groups):
    """``groups``: [((sqrt(abar_t), sqrt(1 - abar_t)), [clip indices])]."""
    return _QSampleFn.apply(X, z, groups)


def training_eps(net, x_t, steps):
    """eps_theta(x_t, steps) as an autograd node over x_t and every parameter of ``net`` (``steps``: one value per clip)."""
    _require_f32(net, "training_eps")
    if not torch.is_grad_enabled():                              # an evaluation of the loss only: the plain forward, nothing kept
        return net((x_t, torch.tensor([float(t) for t in steps])))
    return _TrainEpsFn.apply(x_t, _eps_grad_of(net), tuple(float(t) for t in steps), *net._blob_tensors())


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
