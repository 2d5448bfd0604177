"""The mode contract of the per-layer C-ABI (include/audiopure.h): every block entry point that takes an ap_ctx, in every arithmetic
form of the DiffWave block, either serves the context or returns -22.

Columns: one 12-layer mini net per precision mode at C = 256 ("f32", "f32d", "f32s", "f32sw", "bf16", "bf16s", set through
set_precision) and "f32c64", AP_PREC_F32 at C = 64 -- the only mode built for another width, which every 256-only entry point refuses.
Rows: the entry points.  EXPECTED holds one "serve" / "refuse" per (row, column); HEADER cites the lines of include/audiopure.h
that state each row's modes (test_header_citations_name_their_entry_point keeps them honest).

A refusal returns -22, names in ap_last_error() the mode(s) the entry point is built for, leaves every output bit untouched (NaN
sentinels with a recognisable payload, compared as integers) and leaves no sticky error behind (a valid launch right after it
succeeds).  A served call meets the fp64 oracle of its mode (oracle/diffwave_oracle.py) PER CLIP -- B = 3 distinct clips, clip 1
scaled by 1e-3 -- at the tolerances the mode-specific suites use, and writes nothing outside its outputs (guard bands of 512
128-sample tile rows' worth of elements on each side).  Tolerances (max deviation over the clip's largest reference magnitude):
  fp32 forms 5e-6 (tests/test_gpu_parity.py::test_resblock_matches_oracle and the split / F(2,3) block tests);
  bf16 h' 2e-3, skip 4e-3 (test_gpu_parity.py::test_bf16_resblock_matches_bf16_emulating_oracle);
  bf16s stored image 6e-3 with mean 3e-4 (test_gpu_bf16_store.py::test_bf16_store_block_matches_the_bf16_store_oracle), its
    init image within one bf16 ulp (::test_init_conv_image_is_relu_conv_plus_film_rounded_once);
  backward: fp32 1e-5 (test_gpu_grad.py::test_fused_block_backward_matches_autograd_through_the_oracle), bf16 / bf16s cosine
    >= 0.999 and 2e-2 (test_gpu_grad.py::test_bf16_block_backward_matches_autograd_through_the_bf16_oracle,
    test_gpu_bf16_store.py::test_bf16_store_block_backward_from_its_kept_gate_factors), against fp64 autograd of the oracle block;
  final_affine: eps 2e-5 in the fp32 forms (test_gpu_grad.py::test_eps_vjp_matches_oracle_autograd), 4e-3 in the bf16 modes (the
    bf16 GEMM bar above).
"""
import math
import os
import re
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiopure_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

COLUMNS = ("f32", "f32d", "f32s", "f32sw", "bf16", "bf16s", "f32c64")
S, R = "serve", "refuse"


def _row(**cells):
    assert set(cells) == set(COLUMNS)
    return cells


EXPECTED = {}
for _name, _cells in {
    "ap_init_conv": _row(f32=S, f32d=S, f32s=S, f32sw=S, bf16=S, bf16s=S, f32c64=S),
    "ap_resblock_fwd": _row(f32=S, f32d=S, f32s=S, f32sw=S, bf16=S, bf16s=R, f32c64=S),
    "ap_resblock_fwd_save": _row(f32=S, f32d=S, f32s=R, f32sw=R, bf16=R, bf16s=R, f32c64=S),
    "ap_resblock_fwd_gate": _row(f32=R, f32d=R, f32s=R, f32sw=R, bf16=S, bf16s=R, f32c64=R),
    "ap_resblock_fwd_gate_save": _row(f32=R, f32d=R, f32s=R, f32sw=R, bf16=S, bf16s=R, f32c64=R),
    "ap_skip_gemm": _row(f32=R, f32d=R, f32s=R, f32sw=R, bf16=S, bf16s=S, f32c64=R),
    "ap_init_conv_u": _row(f32=R, f32d=R, f32s=R, f32sw=R, bf16=R, bf16s=S, f32c64=R),
    "ap_resblock_fwd_u": _row(f32=R, f32d=R, f32s=R, f32sw=R, bf16=R, bf16s=S, f32c64=R),
    "ap_resblock_fwd_u_save": _row(f32=R, f32d=R, f32s=R, f32sw=R, bf16=R, bf16s=S, f32c64=R),
    "ap_resblock_bwd": _row(f32=S, f32d=S, f32s=R, f32sw=R, bf16=R, bf16s=R, f32c64=R),
    "ap_resblock_bwd_bf16": _row(f32=R, f32d=R, f32s=R, f32sw=R, bf16=S, bf16s=R, f32c64=R),
    "ap_resblock_bwd_bf16_saved": _row(f32=R, f32d=R, f32s=R, f32sw=R, bf16=S, bf16s=S, f32c64=R),
    "ap_final_affine": _row(f32=S, f32d=S, f32s=S, f32sw=S, bf16=S, bf16s=S, f32c64=S),
    "ap_ctx_set_skip_group": _row(f32=R, f32d=R, f32s=R, f32sw=R, bf16=S, bf16s=S, f32c64=R),
    "ap_ctx_set_f32_form": _row(f32=S, f32d=S, f32s=S, f32sw=S, bf16=R, bf16s=R, f32c64=S),
    "ap_ctx_prepare_backward": _row(f32=S, f32d=S, f32s=R, f32sw=R, bf16=S, bf16s=S, f32c64=R),
    # (the queries: "serve" = returns 1 for every shape of SHAPES)
    "ap_resblock_bwd_available": _row(f32=S, f32d=S, f32s=R, f32sw=R, bf16=R, bf16s=R, f32c64=R),
    "ap_resblock_bwd_bf16_available": _row(f32=R, f32d=R, f32s=R, f32sw=R, bf16=S, bf16s=S, f32c64=R),
}.items():
    for _col, _v in _cells.items():
        EXPECTED[(_name, _col)] = _v

# include/audiopure.h lines (first, last) that state each row's modes
HEADER = {
    "ap_init_conv": (170, 171),
    "ap_resblock_fwd": (174, 179),
    "ap_resblock_fwd_save": (243, 246),
    "ap_resblock_fwd_gate": (198, 199),
    "ap_resblock_fwd_gate_save": (290, 291),
    "ap_skip_gemm": (198, 199),
    "ap_init_conv_u": (215, 217),
    "ap_resblock_fwd_u": (215, 217),
    "ap_resblock_fwd_u_save": (215, 217),
    "ap_resblock_bwd": (260, 262),
    "ap_resblock_bwd_bf16": (276, 280),
    "ap_resblock_bwd_bf16_saved": (290, 291),
    "ap_final_affine": (250, 254),
    "ap_ctx_set_skip_group": (198, 199),
    "ap_ctx_set_f32_form": (237, 239),
    "ap_ctx_prepare_backward": (268, 270),
    "ap_resblock_bwd_available": (261, 262),
    "ap_resblock_bwd_bf16_available": (279, 280),
}

# the mode(s) a refusal must name (ap_last_error)
BUILT_FOR = {
    "ap_resblock_fwd": ("AP_PREC_F32", "AP_PREC_F32_SPLIT", "AP_PREC_BF16"),
    "ap_resblock_fwd_save": ("AP_PREC_F32",),
    "ap_resblock_fwd_gate": ("AP_PREC_BF16",),
    "ap_resblock_fwd_gate_save": ("AP_PREC_BF16",),
    "ap_skip_gemm": ("AP_PREC_BF16", "AP_PREC_BF16_STORE"),
    "ap_init_conv_u": ("AP_PREC_BF16_STORE",),
    "ap_resblock_fwd_u": ("AP_PREC_BF16_STORE",),
    "ap_resblock_fwd_u_save": ("AP_PREC_BF16_STORE",),
    "ap_resblock_bwd": ("AP_PREC_F32",),
    "ap_resblock_bwd_bf16": ("AP_PREC_BF16",),
    "ap_resblock_bwd_bf16_saved": ("AP_PREC_BF16", "AP_PREC_BF16_STORE"),
    "ap_ctx_set_skip_group": ("AP_PREC_BF16", "AP_PREC_BF16_STORE"),
    "ap_ctx_set_f32_form": ("AP_PREC_F32", "AP_PREC_F32_SPLIT"),
    "ap_ctx_prepare_backward": ("AP_PREC_F32", "AP_PREC_BF16", "AP_PREC_BF16_STORE"),
}

# (B, L, layer): L = 1; one past a 128-sample tile; dilation >= L (layer 9: d = 512 > 200); B = 1; a whole-tile clip.  All of them sit
# below the one-tile-per-CU rule of the small-batch twins (B ceil(L / 128) <= 256, ap_resblock_bf16s.hip / ap_resblock_bf16us.hip);
# WIDE_B clips of the last shape sit above it (ap_resblock_fwd_gate, ap_resblock_fwd_u: bit-identical twins).
SHAPES = [(3, 1, 0), (3, 129, 6), (3, 200, 9), (1, 640, 1), (3, 384, 5)]
WIDE_B = 86                                                       # 86 x 3 tiles = 258 > 256: the persistent kernels
SEED = 3
GUARD = 131072                                                    # elements on each side: 512 tile rows of 128 samples (bytes for uint8)
NAN32, NAN16, BYTE = 0x7FC0DEAD, 0x7FDE, 0xA5                     # quiet NaNs with a payload; 0xA5 for opaque byte images


def _swap23(p):
    return (p & ~12) | ((p & 4) << 1) | ((p & 8) >> 1)


PERM = torch.tensor([_swap23(p) for p in range(32)])             # u image: position p of a row holds channel PERM[p] of its chunk


def to_uimg(u):
    B, C_, L = u.shape
    x = u.reshape(B, C_ // 32, 32, L)[:, :, PERM.to(u.device), :]
    return x.permute(0, 1, 3, 2).contiguous().to(torch.bfloat16)


def from_uimg(img):
    B, NC, L, _ = img.shape
    x = img.float().permute(0, 1, 3, 2)[:, :, PERM.to(img.device), :]
    return x.reshape(B, NC * 32, L).contiguous()


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


class Out:
    """An output inside guard bands of sentinel bits: `view` is what the call gets; checks compare bit patterns."""
    _INT = {torch.float32: (torch.int32, NAN32), torch.bfloat16: (torch.int16, NAN16), torch.uint8: (torch.uint8, BYTE)}

    def __init__(self, shape, dtype, dev):
        itype, self.sent = self._INT[dtype]
        self.n = 1
        for v in shape:
            self.n *= int(v)
        self.raw = torch.full((self.n + 2 * GUARD,), self.sent, dtype=itype, device=dev)
        self.view = self.raw[GUARD:GUARD + self.n].view(dtype).view(*shape)

    @property
    def p(self):
        return self.view.data_ptr()

    def guards_intact(self):
        return bool((self.raw[:GUARD] == self.sent).all()) and bool((self.raw[GUARD + self.n:] == self.sent).all())

    def untouched(self):
        return bool((self.raw == self.sent).all())

    def fully_written(self):
        return not bool((self.raw[GUARD:GUARD + self.n] == self.sent).any())


# ---- contexts (one per column, module lifetime) ----------------------------------------------------------------------------------
_COLS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    yield torch.device("cuda:0")
    _COLS.clear()
    _ORACLE.clear()


def _col(col, dev):
    if col not in _COLS:
        from oracle import diffwave_oracle as O
        from audiopure_amd.diffusion_models.DiffWave_Unconditional.WaveNet import WaveNet_Speech_Commands
        C_ = 64 if col == "f32c64" else 256
        cfg = synth.mini_wavenet_config(C_, 12, 12)
        sd = synth.wavenet_state_dict(cfg, SEED)
        net = WaveNet_Speech_Commands(**cfg)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        net = net.to(dev).set_precision("f32" if col == "f32c64" else col)
        eng = net.engine()
        w = {k: v.double() for k, v in O.fold_state_dict(sd).items()}
        _COLS[col] = types.SimpleNamespace(col=col, net=net, eng=eng, lib=eng.lib, ctx=eng.ctx, C=C_, NL=12, w=w, dev=dev,
                                           flags="bf16s" if col == "bf16s" else "bf16" if col == "bf16" else "f32")
    return _COLS[col]


# ---- inputs and the fp64 oracle, once per (width, shape, mode flags) -------------------------------------------------------------
def _inputs(C_, B, L):
    def clips(name, shape, seed, lo, hi):
        t = torch.from_numpy(synth.uniform(f"mc/{name}/{C_}/{B}/{L}", shape, seed, lo, hi)).double()
        if B > 1:
            t[1] *= 1e-3                                          # a small clip between large ones: per-clip errors cannot hide
        return t
    return dict(h=clips("h", (B, C_, L), 1, -1.5, 1.5), gh=clips("gh", (B, C_, L), 2, -1.0, 1.0),
                gs=clips("gs", (B, C_, L), 3, -1.0, 1.0), skip=clips("sk", (B, C_, L), 4, -6.0, 6.0),
                x=clips("x", (B, 1, L), 5, -1.0, 1.0), z=clips("z", (B, 1, L), 6, -1.0, 1.0),
                emb=torch.from_numpy(synth.uniform("mc/emb", (1, 512), 1, -1.0, 1.0)).double().repeat(B, 1))


_ORACLE = {}


def _oracle(T, B, L, layer):
    key = (T.C, T.flags, B, L, layer)
    if key in _ORACLE:
        return _ORACLE[key]
    import torch.nn.functional as F
    from oracle import diffwave_oracle as O
    w, C_ = T.w, T.C
    inp = _inputs(C_, B, L)
    d = 2 ** (layer % 12)
    kw = dict(bf16_operands=T.flags == "bf16", bf16_store=T.flags == "bf16s")
    q = _bf16 if T.flags != "f32" else (lambda t: t)

    def part(n):
        p = f"residual_layer.residual_blocks.{n}"
        return F.linear(inp["emb"][:1], w[p + ".fc_t.weight"], w[p + ".fc_t.bias"]).reshape(-1)
    p = f"residual_layer.residual_blocks.{layer}"
    pt, ptn = part(layer), part(layer + 1)
    hr = inp["h"].clone().requires_grad_(True)
    h_ref, s_ref = O.residual_block(w, layer, d, hr, inp["emb"], **kw)
    (g_ref,) = torch.autograd.grad([h_ref, s_ref], hr, [inp["gh"], inp["gs"]])
    with torch.no_grad():
        u = inp["h"] + pt.view(1, -1, 1)
        y = F.conv1d(q(_bf16(u) if T.flags == "bf16s" else u), q(w[p + ".dilated_conv_layer.conv.weight"]),
                     w[p + ".dilated_conv_layer.conv.bias"], dilation=d, padding=d)
        g = torch.tanh(y[:, :C_]) * torch.sigmoid(y[:, C_:])
        ys = inp["skip"] * math.sqrt(1.0 / T.NL)
        r = F.relu(F.conv1d(q(ys), q(w["final_conv.0.conv.weight"]), w["final_conv.0.conv.bias"]))
        eps = F.conv1d(r, w["final_conv.2.conv.weight"], w["final_conv.2.conv.bias"])
        h0 = F.relu(F.conv1d(inp["x"], w["init_conv.0.conv.weight"], w["init_conv.0.conv.bias"]))
        gq = _bf16(g)                                             # a bf16 g image as ap_skip_gemm reads it, and its skip contribution
        s_of_gq = F.conv1d(gq, _bf16(w[p + ".skip_conv.weight"]), w[p + ".skip_conv.bias"])
    o = dict(inp, d=d, pt=pt, ptn=ptn, h_ref=h_ref.detach(), s_ref=s_ref.detach(), g_ref=g_ref, y=y, eps=eps, h0=h0, gq=gq,
             s_of_gq=s_of_gq, u_out=_bf16(h_ref.detach() + ptn.view(1, -1, 1)), pt0=part(0).detach())
    _ORACLE[key] = o
    return o


def _dev32(t, dev):
    return t.detach().float().contiguous().to(dev)


def _clip_errs(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return [float((got[b] - ref[b]).abs().max() / (ref[b].abs().max() + 1e-300)) for b in range(ref.shape[0])]


def _assert_clips(got, ref, tol, what):
    errs = _clip_errs(got, ref)
    assert max(errs) < tol, (what, errs)


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm() + 1e-300))


def _assert_bwd_clips(got, ref, flags, what):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert torch.isfinite(got).all(), what
    if flags == "f32":
        _assert_clips(got, ref, 1e-5, what)
        return
    for b in range(ref.shape[0]):
        c, e = _cos(got[b], ref[b]), _clip_errs(got[b:b + 1], ref[b:b + 1])[0]
        assert c >= 0.999 and e <= 2e-2, (what, b, c, e)


def _guards(*outs):
    torch.cuda.synchronize()
    for o in outs:
        assert o.guards_intact(), "write outside an output buffer"


def _assert_alive(T):
    """A valid launch on the same context right after a refusal succeeds: no sticky error."""
    from audiopure_amd import _native as N
    x = torch.full((1, 1, 5), 0.5, device=T.dev)
    h = torch.empty((1, T.C, 5), device=T.dev)
    assert T.lib.ap_init_conv(T.ctx, N.ptr(x), N.ptr(h), 1, 5, N.stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(h).all())


def _assert_refused(T, row, rc, outs):
    assert rc == -22, (row, T.col, rc)
    msg = (T.lib.ap_last_error() or b"").decode(errors="replace")
    for mode in BUILT_FOR[row]:
        assert re.search(rf"\b{mode}\b", msg), (row, T.col, msg)
    torch.cuda.synchronize()
    for o in outs:
        assert o.untouched(), (row, T.col, "a refused call wrote to an output")
    _assert_alive(T)


# ---- the rows ----------------------------------------------------------------------------------------------------------------------
def _r_init_conv(T, serve):
    from audiopure_amd import _native as N
    for B, L, layer in SHAPES:
        o = _oracle(T, B, L, layer)
        x = _dev32(o["x"], T.dev)
        h = Out((B, T.C, L), torch.float32, T.dev)
        N.check(T.lib.ap_init_conv(T.ctx, N.ptr(x), h.p, B, L, N.stream()))
        _guards(h)
        assert h.fully_written()
        _assert_clips(h.view, o["h0"], 5e-6, ("h0", B, L))


def _fwd_inputs(T, o):
    return _dev32(o["h"], T.dev), _dev32(o["pt"], T.dev)


def _r_resblock_fwd(T, serve, save=False):
    from audiopure_amd import _native as N
    row = "ap_resblock_fwd_save" if save else "ap_resblock_fwd"
    for B, L, layer in SHAPES:
        o = _oracle(T, B, L, layer)
        hd, pt = _fwd_inputs(T, o)
        hout, sk = Out((B, T.C, L), torch.float32, T.dev), Out((B, T.C, L), torch.float32, T.dev)
        pre = Out((B, 2 * T.C, L), torch.float32, T.dev)
        if save:
            rc = T.lib.ap_resblock_fwd_save(T.ctx, layer, N.ptr(hd), N.ptr(pt), hout.p, sk.p, pre.p, 0, B, L, N.stream())
        else:
            rc = T.lib.ap_resblock_fwd(T.ctx, layer, N.ptr(hd), N.ptr(pt), hout.p, sk.p, 0, B, L, N.stream())
        outs = (hout, sk, pre) if save else (hout, sk)
        if not serve:
            _assert_refused(T, row, rc, outs)
            return
        assert rc == 0, T.lib.ap_last_error()
        _guards(*outs)
        assert all(x.fully_written() for x in outs)
        th, ts = (2e-3, 4e-3) if T.flags == "bf16" else (5e-6, 5e-6)
        _assert_clips(hout.view, o["h_ref"], th, (row, "h'", B, L, layer))
        _assert_clips(sk.view, o["s_ref"], ts, (row, "skip", B, L, layer))
        if save:
            _assert_clips(pre.view, o["y"], 5e-6, (row, "pre-gate", B, L, layer))


def _gate_call(T, o, B, L, layer, save, hd=None, pt=None):
    from audiopure_amd import _native as N
    if hd is None:
        hd, pt = _fwd_inputs(T, o)
    hout, gi = Out((B, T.C, L), torch.float32, T.dev), Out((B, L, T.C), torch.bfloat16, T.dev)
    fac = Out((int(T.lib.ap_gate_factor_bytes(B, L)),), torch.uint8, T.dev)
    if save:
        rc = T.lib.ap_resblock_fwd_gate_save(T.ctx, layer, N.ptr(hd), N.ptr(pt), hout.p, gi.p, fac.p, B, L, N.stream())
        return rc, (hout, gi, fac)
    rc = T.lib.ap_resblock_fwd_gate(T.ctx, layer, N.ptr(hd), N.ptr(pt), hout.p, gi.p, B, L, N.stream())
    return rc, (hout, gi)


def _skip_of(T, layer, gimg, B, L):
    from audiopure_amd import _native as N
    sk = Out((B, T.C, L), torch.float32, T.dev)
    N.check(T.lib.ap_skip_gemm(T.ctx, layer, 1, gimg.data_ptr(), sk.p, 0, B, L, N.stream()))
    _guards(sk)
    assert sk.fully_written()
    return sk.view


def _r_fwd_gate(T, serve, save=False):
    row = "ap_resblock_fwd_gate_save" if save else "ap_resblock_fwd_gate"
    for B, L, layer in SHAPES:
        o = _oracle(T, B, L, layer)
        rc, outs = _gate_call(T, o, B, L, layer, save)
        if not serve:
            _assert_refused(T, row, rc, outs)
            return
        assert rc == 0, T.lib.ap_last_error()
        _guards(*outs)
        hout, gi = outs[0], outs[1]
        assert hout.fully_written() and gi.fully_written()
        _assert_clips(hout.view, o["h_ref"], 2e-3, (row, "h'", B, L, layer))
        _assert_clips(_skip_of(T, layer, gi.view, B, L), o["s_ref"], 4e-3, (row, "skip via g image", B, L, layer))
        if save:                                                  # bit-identical to ap_resblock_fwd_gate (include/audiopure.h)
            rc2, (h2, g2) = _gate_call(T, o, B, L, layer, False)
            assert rc2 == 0
            torch.cuda.synchronize()
            assert torch.equal(h2.raw, hout.raw) and torch.equal(g2.raw, gi.raw)
        elif (B, L, layer) == SHAPES[-1]:
            _twin_gate(T, o, B, L, layer, hout, gi)


def _wide(T, o, B, L, key):
    """WIDE_B clips: the oracle's B clips first, then other clips of the same shape."""
    extra = torch.from_numpy(synth.uniform(f"mc/wide/{key}/{T.C}/{L}", (WIDE_B - B, T.C, L), 7, -1.5, 1.5)).double()
    return torch.cat([o[key], extra], 0)


def _twin_gate(T, o, B, L, layer, hout, gi):
    """Above the one-tile-per-CU rule the persistent kernel runs: a clip's h' and g image are the same bits (audiopure.h)."""
    from audiopure_amd import _native as N
    assert WIDE_B * ((L + 127) // 128) > 256 >= B * ((L + 127) // 128)
    hw = _dev32(_wide(T, o, B, L, "h"), T.dev)
    pt = _dev32(o["pt"], T.dev)
    rc, (h2, g2) = _gate_call(T, o, WIDE_B, L, layer, False, hw, pt)
    assert rc == 0
    _guards(h2, g2)
    assert h2.fully_written() and g2.fully_written()
    for b in range(B):
        assert torch.equal(h2.view[b].view(torch.int32), hout.view[b].view(torch.int32)), ("twin h'", b)
        assert torch.equal(g2.view[b].view(torch.int16), gi.view[b].view(torch.int16)), ("twin g image", b)


def _r_skip_gemm(T, serve):
    from audiopure_amd import _native as N
    for B, L, layer in SHAPES:
        o = _oracle(T, B, L, layer)
        gimg = o["gq"].permute(0, 2, 1).contiguous().to(torch.bfloat16).to(T.dev)      # [B][L][C]
        sk = Out((B, T.C, L), torch.float32, T.dev)
        rc = T.lib.ap_skip_gemm(T.ctx, layer, 1, gimg.data_ptr(), sk.p, 0, B, L, N.stream())
        if not serve:
            _assert_refused(T, "ap_skip_gemm", rc, (sk,))
            return
        assert rc == 0, T.lib.ap_last_error()
        _guards(sk)
        assert sk.fully_written()
        _assert_clips(sk.view, o["s_of_gq"], 4e-3, ("skip gemm", B, L, layer))


def _r_init_conv_u(T, serve):
    from audiopure_amd import _native as N
    for B, L, layer in SHAPES:
        o = _oracle(T, B, L, layer)
        x, pt0 = _dev32(o["x"], T.dev), _dev32(o["pt0"], T.dev)
        img = Out((B, T.C // 32, L, 32), torch.bfloat16, T.dev)
        rc = T.lib.ap_init_conv_u(T.ctx, N.ptr(x), N.ptr(pt0), img.p, B, L, N.stream())
        if not serve:
            _assert_refused(T, "ap_init_conv_u", rc, (img,))
            return
        assert rc == 0, T.lib.ap_last_error()
        _guards(img)
        assert img.fully_written()
        # (in fp32, as the kernel forms it: where h0 + part_t cancels, the fp32 sum's absolute error is many bf16 ulps of the result)
        ref = _bf16(o["h0"].float() + o["pt0"].float().view(1, -1, 1))
        got = from_uimg(img.view).cpu()
        a = ref.abs().clamp_min(1e-30)
        ulp = torch.exp2(torch.floor(torch.log2(a)) - 7)
        for b in range(B):                                        # fma vs mul + add before the rounding: at most one ulp
            assert bool(((got[b] - ref[b]).abs() <= ulp[b]).all()), ("u_0", b, B, L)


def _u_call(T, o, B, L, layer, save, uin=None):
    from audiopure_amd import _native as N
    if uin is None:
        uin = to_uimg(_bf16(o["h"] + o["pt"].view(1, -1, 1)).float().to(T.dev))
    ptn = _dev32(o["ptn"], T.dev)
    uo, gi = Out((B, T.C // 32, L, 32), torch.bfloat16, T.dev), Out((B, L, T.C), torch.bfloat16, T.dev)
    if save:
        fac = Out((int(T.lib.ap_gate_factor_bytes(B, L)),), torch.uint8, T.dev)
        rc = T.lib.ap_resblock_fwd_u_save(T.ctx, layer, uin.data_ptr(), N.ptr(ptn), uo.p, gi.p, fac.p, B, L, N.stream())
        return rc, (uo, gi, fac), uin
    rc = T.lib.ap_resblock_fwd_u(T.ctx, layer, uin.data_ptr(), N.ptr(ptn), uo.p, gi.p, B, L, N.stream())
    return rc, (uo, gi), uin


def _r_fwd_u(T, serve, save=False):
    row = "ap_resblock_fwd_u_save" if save else "ap_resblock_fwd_u"
    for B, L, layer in SHAPES:
        o = _oracle(T, B, L, layer)
        rc, outs, uin = _u_call(T, o, B, L, layer, save)
        if not serve:
            _assert_refused(T, row, rc, outs)
            return
        assert rc == 0, T.lib.ap_last_error()
        _guards(*outs)
        uo, gi = outs[0], outs[1]
        assert uo.fully_written() and gi.fully_written()
        got, ref = from_uimg(uo.view).cpu().double(), o["u_out"]
        for b in range(B):
            m, dd = float(ref[b].abs().max()), (got[b] - ref[b]).abs()
            assert float(dd.max()) < 6e-3 * m and float(dd.mean()) < 3e-4 * m, (row, "u'", b, B, L, layer, float(dd.max()) / m)
        _assert_clips(_skip_of(T, layer, gi.view, B, L), o["s_ref"], 4e-3, (row, "skip via g image", B, L, layer))
        if save:                                                  # u' and g image bit-identical to ap_resblock_fwd_u
            rc2, (u2, g2), _ = _u_call(T, o, B, L, layer, False, uin)
            assert rc2 == 0
            torch.cuda.synchronize()
            assert torch.equal(u2.raw, uo.raw) and torch.equal(g2.raw, gi.raw)
        elif (B, L, layer) == SHAPES[-1]:
            assert WIDE_B * ((L + 127) // 128) > 256 >= B * ((L + 127) // 128)
            uw = to_uimg(_bf16(_wide(T, o, B, L, "h") + o["pt"].view(1, -1, 1)).float().to(T.dev))
            rc2, (u2, g2), _ = _u_call(T, o, WIDE_B, L, layer, False, uw)
            assert rc2 == 0
            _guards(u2, g2)
            for b in range(B):
                assert torch.equal(u2.view[b].view(torch.int16), uo.view[b].view(torch.int16)), ("twin u'", b)
                assert torch.equal(g2.view[b].view(torch.int16), gi.view[b].view(torch.int16)), ("twin g image", b)


def _r_bwd(T, serve):
    from audiopure_amd import _native as N
    T.lib.ap_ctx_prepare_backward(T.ctx, N.stream())
    for B, L, layer in SHAPES:
        o = _oracle(T, B, L, layer)
        ghd, gsd, pre = _dev32(o["gh"], T.dev), _dev32(o["gs"], T.dev), _dev32(o["y"], T.dev)
        dy, dh = Out((B, 2 * T.C, L), torch.float32, T.dev), Out((B, T.C, L), torch.float32, T.dev)
        rc = T.lib.ap_resblock_bwd(T.ctx, layer, N.ptr(ghd), N.ptr(gsd), N.ptr(pre), dy.p, dh.p, B, L, N.stream())
        if not serve:
            _assert_refused(T, "ap_resblock_bwd", rc, (dy, dh))
            return
        assert rc == 0, T.lib.ap_last_error()
        _guards(dy, dh)
        assert dh.fully_written()
        _assert_bwd_clips(dh.view, o["g_ref"], T.flags, ("ap_resblock_bwd", B, L, layer))


def _r_bwd_bf16(T, serve):
    from audiopure_amd import _native as N
    T.lib.ap_ctx_prepare_backward(T.ctx, N.stream())
    for B, L, layer in SHAPES:
        o = _oracle(T, B, L, layer)
        hd, pt = _fwd_inputs(T, o)
        ghd, gsd = _dev32(o["gh"], T.dev), _dev32(o["gs"], T.dev)
        dy, dh = Out((B, L, 2 * T.C), torch.bfloat16, T.dev), Out((B, T.C, L), torch.float32, T.dev)
        rc = T.lib.ap_resblock_bwd_bf16(T.ctx, layer, N.ptr(hd), N.ptr(pt), N.ptr(ghd), N.ptr(gsd), dy.p, dh.p, B, L, N.stream())
        if not serve:
            _assert_refused(T, "ap_resblock_bwd_bf16", rc, (dy, dh))
            return
        assert rc == 0, T.lib.ap_last_error()
        _guards(dy, dh)
        assert dh.fully_written()
        _assert_bwd_clips(dh.view, o["g_ref"], T.flags, ("ap_resblock_bwd_bf16", B, L, layer))


def _r_bwd_bf16_saved(T, serve):
    from audiopure_amd import _native as N
    T.lib.ap_ctx_prepare_backward(T.ctx, N.stream())
    for B, L, layer in SHAPES:
        o = _oracle(T, B, L, layer)
        if T.flags == "bf16s":                                    # the factors of this context's own saving forward
            rc, outs, _ = _u_call(T, o, B, L, layer, True)
            fac = outs[2]
        elif T.flags == "bf16":
            rc, outs = _gate_call(T, o, B, L, layer, True)
            fac = outs[2]
        else:                                                     # (no saving forward in this mode: any bytes)
            rc, fac = 0, Out((int(T.lib.ap_gate_factor_bytes(B, L)),), torch.uint8, T.dev)
        assert rc == 0
        ghd, gsd = _dev32(o["gh"], T.dev), _dev32(o["gs"], T.dev)
        dy, dh = Out((B, L, 2 * T.C), torch.bfloat16, T.dev), Out((B, T.C, L), torch.float32, T.dev)
        rc = T.lib.ap_resblock_bwd_bf16_saved(T.ctx, layer, fac.p, N.ptr(ghd), N.ptr(gsd), 0, dy.p, dh.p, B, L, N.stream())
        if not serve:
            _assert_refused(T, "ap_resblock_bwd_bf16_saved", rc, (dy, dh))
            return
        assert rc == 0, T.lib.ap_last_error()
        _guards(fac, dy, dh)
        assert dh.fully_written()
        _assert_bwd_clips(dh.view, o["g_ref"], T.flags, ("ap_resblock_bwd_bf16_saved", B, L, layer))


def _r_final_affine(T, serve):
    from audiopure_amd import _native as N
    ca, cb, cs = 1.01, -0.2, 0.05
    for B, L, layer in SHAPES:
        o = _oracle(T, B, L, layer)
        skip, x, z = _dev32(o["skip"], T.dev), _dev32(o["x"], T.dev), _dev32(o["z"], T.dev)
        eps, out = Out((B, 1, L), torch.float32, T.dev), Out((B, 1, L), torch.float32, T.dev)
        N.check(T.lib.ap_final_affine(T.ctx, N.ptr(skip), N.ptr(x), eps.p, out.p, ca, cb, cs, N.ptr(z), 0, 0, 0, B, L, N.stream()))
        _guards(eps, out)
        assert eps.fully_written() and out.fully_written()
        tol = 2e-5 if T.flags == "f32" else 4e-3
        _assert_clips(eps.view, o["eps"], tol, ("eps", B, L))
        _assert_clips(out.view, ca * o["x"] + cb * o["eps"] + cs * o["z"], tol, ("out", B, L))


def _r_set_skip_group(T, serve):
    G, (B, L, _) = 4, SHAPES[-1]
    assert T.lib.ap_ctx_set_skip_group(T.ctx, 0) == 0              # (accepted in every mode)
    ws0 = T.lib.ap_workspace_bytes(T.ctx, B, L)
    rc = T.lib.ap_ctx_set_skip_group(T.ctx, G)
    ws = T.lib.ap_workspace_bytes(T.ctx, B, L)
    if not serve:
        _assert_refused(T, "ap_ctx_set_skip_group", rc, ())
        assert ws == ws0                                          # nothing about the context changed
        return
    try:
        assert rc == 0, T.lib.ap_last_error()
        slot = B * L * T.C * 2                                    # one [B][L][C] bf16 g image per layer of a group
        if T.flags == "bf16":                                     # (0: the fused block, no images)
            assert ws - ws0 == G * slot
        else:                                                     # (bf16 storage: 0 means one group of all layers)
            assert ws0 - ws == (T.NL - G) * slot
    finally:
        assert T.lib.ap_ctx_set_skip_group(T.ctx, 0) == 0


def _r_set_f32_form(T, serve):
    before = T.lib.ap_ctx_get_f32_form(T.ctx)
    rc = T.lib.ap_ctx_set_f32_form(T.ctx, 1)
    if not serve:
        _assert_refused(T, "ap_ctx_set_f32_form", rc, ())
        assert T.lib.ap_ctx_get_f32_form(T.ctx) == before
        return
    try:
        assert rc == 0, T.lib.ap_last_error()
        assert T.lib.ap_ctx_get_f32_form(T.ctx) == (1 if T.C == 256 else 0)    # C = 64: accepted, the direct form runs
    finally:
        assert T.lib.ap_ctx_set_f32_form(T.ctx, int(T.net._f32_form)) == 0


def _r_prepare_backward(T, serve):
    from audiopure_amd import _native as N
    rc = T.lib.ap_ctx_prepare_backward(T.ctx, N.stream())
    if not serve:
        _assert_refused(T, "ap_ctx_prepare_backward", rc, ())
        return
    assert rc == 0, T.lib.ap_last_error()
    assert T.lib.ap_ctx_prepare_backward(T.ctx, N.stream()) == 0  # a second call is a no-op


def _r_available(name, launch_row):
    def run(T, serve):
        assert EXPECTED[(name, T.col)] == EXPECTED[(launch_row, T.col)], "the query answers for its launch"
        for B, L, _ in SHAPES + [(WIDE_B, SHAPES[-1][1], 0)]:
            assert getattr(T.lib, name)(T.ctx, B, L) == (1 if serve else 0), (name, T.col, B, L)
    return run


ROWS = {
    "ap_init_conv": _r_init_conv,
    "ap_resblock_fwd": _r_resblock_fwd,
    "ap_resblock_fwd_save": lambda T, s: _r_resblock_fwd(T, s, save=True),
    "ap_resblock_fwd_gate": _r_fwd_gate,
    "ap_resblock_fwd_gate_save": lambda T, s: _r_fwd_gate(T, s, save=True),
    "ap_skip_gemm": _r_skip_gemm,
    "ap_init_conv_u": _r_init_conv_u,
    "ap_resblock_fwd_u": _r_fwd_u,
    "ap_resblock_fwd_u_save": lambda T, s: _r_fwd_u(T, s, save=True),
    "ap_resblock_bwd": _r_bwd,
    "ap_resblock_bwd_bf16": _r_bwd_bf16,
    "ap_resblock_bwd_bf16_saved": _r_bwd_bf16_saved,
    "ap_final_affine": _r_final_affine,
    "ap_ctx_set_skip_group": _r_set_skip_group,
    "ap_ctx_set_f32_form": _r_set_f32_form,
    "ap_ctx_prepare_backward": _r_prepare_backward,
    "ap_resblock_bwd_available": _r_available("ap_resblock_bwd_available", "ap_resblock_bwd"),
    "ap_resblock_bwd_bf16_available": _r_available("ap_resblock_bwd_bf16_available", "ap_resblock_bwd_bf16_saved"),
}


@pytest.mark.parametrize("col", COLUMNS)
@pytest.mark.parametrize("row", list(ROWS))
def test_mode_contract_cell(dev, row, col):
    """One cell of the matrix: the entry point serves this context (oracle per clip, guard bands) or refuses it (-22, the modes
    named, outputs untouched, no sticky error).  A cell missing from EXPECTED fails: classify a new entry point or mode first."""
    assert (row, col) in EXPECTED, f"({row}, {col}) is not classified in EXPECTED"
    T = _col(col, dev)
    ROWS[row](T, EXPECTED[(row, col)] == S)
    torch.cuda.synchronize()


def test_expected_table_is_exactly_the_matrix(dev):
    assert set(EXPECTED) == {(r, c) for r in ROWS for c in COLUMNS}
    assert set(HEADER) == set(ROWS)
    assert set(EXPECTED.values()) == {S, R}


def test_header_citations_name_their_entry_point(dev):
    with open(os.path.join(ROOT, "include", "audiopure.h")) as f:
        lines = f.read().split("\n")
    for row, (a, b) in HEADER.items():
        text = " ".join(lines[a - 1:b])
        assert re.search(rf"\b{row}\b", text), (row, a, b)


# ---- memory accounting of the differentiable chain (audiopure_amd/diffusion_models/_grad.py) ------------------------------------
def _acct_net(mode, dev):
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.WaveNet import WaveNet_Speech_Commands
    cfg = synth.mini_wavenet_config(256, 12, 12)
    net = WaveNet_Speech_Commands(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.wavenet_state_dict(cfg, SEED).items()}, strict=True)
    return net.to(dev).set_precision(mode)


@pytest.mark.parametrize("mode,acts,keep", [("f32", True, True), ("f32", False, True), ("bf16", True, True), ("bf16", True, False),
                                            ("bf16s", True, True)])
def test_saved_bytes_estimate_equals_what_forward_save_keeps(dev, mode, acts, keep):
    """EpsGrad.saved_bytes(x, acts) -- what _ChainFn budgets with -- against the bytes forward_save(x, t, acts) actually returns plus
    the gate-image buffer that call newly allocated: equal to 1 %, never below, with a fresh and with a warm EpsGrad."""
    from audiopure_amd.diffusion_models import _grad as G
    net = _acct_net(mode, dev)
    eg = G.EpsGrad(net)
    eg.keep_gate_factors = keep
    x = torch.from_numpy(synth.waveforms(2, 1500, seed=4)).to(dev)
    for state in ("fresh", "warm"):
        est = eg.saved_bytes(x, acts)
        had = eg._gimg
        _, saved = eg.forward_save(x, 2.0, acts)
        new_buf = eg._gimg.numel() * eg._gimg.element_size() if eg._gimg is not None and eg._gimg is not had else 0
        actual = G._saved_bytes(saved) + new_buf
        assert actual <= est <= 1.01 * actual, (mode, acts, keep, state, est, actual)
        if state == "fresh":                                      # the one-off buffer is reported apart from what the link keeps
            probe = G.EpsGrad(net)
            probe.keep_gate_factors = keep
            per_link, once = probe.saved_bytes(x, acts, split=True)
            assert once == new_buf and per_link + once == est, (per_link, once, new_buf, est)
        del saved


@pytest.mark.parametrize("C_,mode,acts,keep", [(64, "f32", True, True), (64, "f32", False, True), (256, "f32", True, True),
                                               (256, "f32", False, True), (256, "f32s", True, True), (256, "bf16", True, True),
                                               (256, "bf16", True, False), (256, "bf16s", True, True)])
def test_saved_bytes_is_exactly_what_forward_save_keeps(dev, C_, mode, acts, keep):
    """saved_bytes sums the list forward_save allocates from (_grad._link_buffers): the link's bytes and the one-off gate-image
    buffer's agree to the byte, not to 1 %."""
    from audiopure_amd.diffusion_models import _grad as G
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.WaveNet import WaveNet_Speech_Commands
    cfg = synth.mini_wavenet_config(C_, 12, 12)
    net = WaveNet_Speech_Commands(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.wavenet_state_dict(cfg, SEED).items()}, strict=True)
    eg = G.EpsGrad(net.to(dev).set_precision(mode))
    eg.keep_gate_factors = keep
    x = torch.from_numpy(synth.waveforms(2, 1500, seed=4)).to(dev)
    per_link, once = eg.saved_bytes(x, acts, split=True)
    _, saved = eg.forward_save(x, 2.0, acts)
    assert per_link == G._saved_bytes(saved), (per_link, G._saved_bytes(saved))
    assert once == (eg._gimg.numel() * eg._gimg.element_size() if eg._gimg is not None else 0)
    assert eg.saved_bytes(x, acts, split=True) == (per_link, 0)   # (warm: the buffer is there)


def test_chain_keeps_exactly_the_links_the_budget_holds(dev):
    """A 5-link bf16 chain under SAVE_BUDGET_BYTES = the one-off gate-image buffer + 2 x one link's true bytes + a margin: exactly two
    links keep their saves, and what they keep plus that buffer stays within the budget (restored in a finally, as in
    test_gpu_grad.py::test_eps_vjp_is_the_same_with_kept_and_with_recomputed_pre_gate_activations)."""
    from audiopure_amd.diffusion_models import _grad as G
    net = _acct_net("bf16", dev)
    B, L = 2, 1500
    x = torch.from_numpy(synth.waveforms(B, L, seed=8)).to(dev)
    probe = G.EpsGrad(net)
    _, saved = probe.forward_save(x, 2.0)
    link = G._saved_bytes(saved)
    buf = probe._gimg.numel() * probe._gimg.element_size()
    del saved, probe
    steps = [(4.0 - k, 1.0, -0.01, 0.0, 0) for k in range(5)]
    old = G.SAVE_BUDGET_BYTES
    try:
        G.SAVE_BUDGET_BYTES = buf + 2 * link + (1 << 20)
        eg = G.EpsGrad(net)
        xg = x.clone().requires_grad_(True)
        out = G._ChainFn.apply(xg, eg, steps, 1.0, 0.0, [None])
        saves = out.grad_fn.saves
        kept = [s for s in saves if s is not None]
        assert len(kept) == 2, [None if s is None else G._saved_bytes(s) for s in saves]
        held = sum(G._saved_bytes(s) for s in kept) + eg._gimg.numel() * eg._gimg.element_size()
        assert held <= G.SAVE_BUDGET_BYTES, (held, G.SAVE_BUDGET_BYTES)
        out.sum().backward()                                      # and the chain still differentiates
        assert torch.isfinite(xg.grad).all()
    finally:
        G.SAVE_BUDGET_BYTES = old
