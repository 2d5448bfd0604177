"""The F(2,3) fp32 block with the X staging by (channel, quad of four pairs) -- four 16-byte loads per chunk, part_t from the
launch constants' LDS copy, packed adds, sixteen ds_write_b32 (DIET_QUAD_ of audiopure_amd/csrc/ap_resblock_f32w.hip; one
instantiation per dilation class: d = 1, d = 2, d >= 4) -- against the kernel kept verbatim in the tools library
(tools/csrc/ap_resblock_f32w_parent.hip): h', skip and the pre-gate rows bit for bit -- the item moves or merges instructions, every
accumulator sees the operations it always did and every staged value is the same float -- and a second and a third launch equal
to the first.  (Masks 9398 and 13494, with a unit's MFMAs by row tile, passed the same cases before that bit failed the A/B's rule
and left the source: docs/HISTORY.md I.15.)

Every new mask on the h'-writing 16-byte form, the last layer's and the SAVE form at the product's mask, and the product library
through ap_resblock_fwd / ap_resblock_fwd_save.  C = S = 256, B = 3.  Shapes: L = 4096 with d = 1, 2, 4, 16, 32, 2048 (every
dilation class; d = 1, 2, 2048: taps past both ends); L = 192, d = 4 (three tiles, the last partial); L = 196, d = 1, 2, 4 and 32
(L % 8 != 0: a last tile of four pairs, quads past the pair count; d = 1, 2: a last quad of two pairs); L = 64, d = 128 (every +-d piece outside); L = 194 (the 4-byte
form: no item); one grid with at least three tiles per workgroup (the cross-tile request and the carried fragment cross a tile
turn); part_t all negative at d = 1 and d = 2048: out-of-clip taps stay +0 whatever its sign."""
import ctypes as C

import pytest
import torch

import __graft_entry__ as G
from audiopure_amd import synth, _native as N

pytestmark = pytest.mark.gpu

_vp, _i = C.c_void_p, C.c_int
_BLOCK_ARGS = [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]
PRODUCT_MASK = 5302                                               # the mask of the product library and of the tools library's other forms
MASKS = (1206, 5302)                                              # the product before this change, + DIET_QUAD_: the product
FORMS = ("acc0", "acc1", "noh", "save")


@pytest.fixture(scope="module")
def rig():
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.WaveNet import WaveNet_Speech_Commands, embedding_frequencies
    dev = torch.device("cuda:0")
    cfg = synth.mini_wavenet_config(256, 12, 12)
    net = WaveNet_Speech_Commands(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.wavenet_state_dict(cfg, 3).items()})
    net = net.to(dev)
    eng = net.engine()                                            # the product library's context
    assert eng.lib.ap_ctx_get_f32_form(eng.ctx) == 1
    tl = C.CDLL(G.build_hip(tools=True))                          # the tools library: its own context over the same weights
    for name in ("ap_ctx_create", "ap_ctx_destroy", "ap_ctx_load_wavenet", "ap_ctx_set_f32_form", "ap_ctx_get_f32_form", "ap_last_error"):
        getattr(tl, name).restype, getattr(tl, name).argtypes = N.SIGNATURES[name]
    for name in ("ap_debug_resblock_f32w_parent", "ap_debug_resblock_f32w"):
        getattr(tl, name).restype, getattr(tl, name).argtypes = _i, _BLOCK_ARGS
    tl.ap_debug_f32w_diet.restype, tl.ap_debug_f32w_diet.argtypes = _i, [_i]
    ctx = C.c_void_p()
    assert tl.ap_ctx_create(C.byref(eng.cfg), C.byref(ctx)) == 0, tl.ap_last_error()
    with torch.no_grad():
        blob = torch.cat([t.detach().reshape(-1).float() for t in net._blob_tensors()]).contiguous()
        freq = embedding_frequencies(cfg["diffusion_step_embed_dim_in"]).to(dev).contiguous()
    assert tl.ap_ctx_load_wavenet(ctx, N.ptr(blob), blob.numel(), N.ptr(freq), N.stream()) == 0, tl.ap_last_error()
    assert tl.ap_ctx_set_f32_form(ctx, 1) == 0 and tl.ap_ctx_get_f32_form(ctx) == 1
    torch.cuda.synchronize()
    yield dev, eng, tl, ctx
    torch.cuda.synchronize()
    tl.ap_ctx_destroy(ctx)


def _buffers(form, h, skip0, B, L, dev):
    """Outputs start from sentinels / the given running skip."""
    accumulate = 0 if form == "acc0" else 1
    hout = None if form == "noh" else torch.full_like(h, 3.0)
    skip = skip0.clone() if accumulate else torch.full_like(skip0, 7.0)
    pre = torch.full((B, 512, L), 5.0, device=dev) if form == "save" else None
    return accumulate, hout, skip, pre


def _run(fn, ctx, layer, h, pt, skip0, form, B, L, dev):
    """One launch of a form: (h' or None, skip, pre-gate rows or None)."""
    accumulate, hout, skip, pre = _buffers(form, h, skip0, B, L, dev)
    rc = fn(ctx, layer, N.ptr(h), N.ptr(pt), N.ptr(hout), N.ptr(skip), accumulate, B, L, N.stream(), N.ptr(pre))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return hout, skip, pre


def _run_product(eng, layer, h, pt, skip0, form, B, L, dev):
    accumulate, hout, skip, pre = _buffers(form, h, skip0, B, L, dev)
    if form == "save":
        N.check(eng.lib.ap_resblock_fwd_save(eng.ctx, layer, N.ptr(h), N.ptr(pt), N.ptr(hout), N.ptr(skip), N.ptr(pre), accumulate, B, L, N.stream()))
    else:
        N.check(eng.lib.ap_resblock_fwd(eng.ctx, layer, N.ptr(h), N.ptr(pt), N.ptr(hout), N.ptr(skip), accumulate, B, L, N.stream()))
    torch.cuda.synchronize()
    return hout, skip, pre


def _same(a, b, what):
    for x, y, name in zip(a, b, ("h'", "skip", "pre-gate")):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert torch.equal(x, y), f"{what}: {name} differs in {(x != y).sum().item()} of {x.numel()} elements"


def _check(rig, B, L, layer, pt_sign=0):
    """pt_sign -1: every part_t negative."""
    dev, eng, tl, ctx = rig
    g = torch.Generator(device="cpu").manual_seed(1000 * layer + L + 7)
    h = (torch.rand(B, 256, L, generator=g) * 3 - 1.5).to(dev)
    skip0 = (torch.rand(B, 256, L, generator=g) * 2 - 1).to(dev)
    pt = torch.rand(256, generator=g) * 2 - 1
    if pt_sign < 0:
        pt = -pt.abs() - 0.01
        assert (pt < 0).all()
    pt = pt.to(dev)
    try:
        for form in FORMS:
            what = f"L={L} layer={layer} B={B} {form}"
            ref = _run(tl.ap_debug_resblock_f32w_parent, ctx, layer, h, pt, skip0, form, B, L, dev)   # once per form, shared
            # (the mask selects among the instantiations of the h'-writing form; the last layer's and the SAVE form have one)
            for mask in (MASKS if form in ("acc0", "acc1") else (PRODUCT_MASK,)):
                assert tl.ap_debug_f32w_diet(mask) == 0
                new = _run(tl.ap_debug_resblock_f32w, ctx, layer, h, pt, skip0, form, B, L, dev)
                _same(new, ref, f"{what}, mask {mask}")
                for nth in ("second", "third"):
                    again = _run(tl.ap_debug_resblock_f32w, ctx, layer, h, pt, skip0, form, B, L, dev)
                    _same(again, new, f"{what}, mask {mask}, {nth} launch")
            if form != "noh":                                     # (no per-block entry point of include/audiopure.h reaches the last layer's form)
                new = _run_product(eng, layer, h, pt, skip0, form, B, L, dev)
                _same(new, ref, f"{what}, product library")
                for nth in ("second", "third"):
                    again = _run_product(eng, layer, h, pt, skip0, form, B, L, dev)
                    _same(again, new, f"{what}, product library, {nth} launch")
    finally:
        assert tl.ap_debug_f32w_diet(PRODUCT_MASK) == 0


def test_masks_exist(rig):
    tl = rig[2]
    try:
        for mask in (0, 2, 4, 6, 22, 54, 150, 182) + MASKS:
            assert tl.ap_debug_f32w_diet(mask) == 0, mask
        for mask in (118, 694, 2230, 3766, 4096, 9398, 13494):   # (no such instantiation: refused, not served by another)
            assert tl.ap_debug_f32w_diet(mask) != 0, mask
    finally:
        assert tl.ap_debug_f32w_diet(PRODUCT_MASK) == 0


@pytest.mark.parametrize("layer", [0, 1, 2, 4, 5, 11])
def test_dilations(rig, layer):
    _check(rig, 3, 4096, layer)                                   # d = 1, 2 (a class each), 4, 16 (d < 32), 32, 2048; d = 1, 2, 2048: taps past both ends


def test_partial_last_tile(rig):
    _check(rig, 3, 192, 2)                                        # d = 4: 96 pairs = three tiles, the last one partial


@pytest.mark.parametrize("layer", [0, 1, 2, 5])
def test_last_tile_of_four_pairs(rig, layer):
    # L % 8 != 0.  d = 4, 32: 100 pairs, the fourth tile holds one quad, seven are past the pair count; d = 1, 2: 98 pairs, the last
    # quad holds two of them
    _check(rig, 3, 196, layer)


def test_dilation_past_the_clip(rig):
    _check(rig, 3, 64, 7)                                         # d = 128 >= L: every second output masked, every +-d piece outside


def test_three_tiles_per_workgroup(rig):
    dev = rig[0]
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    L, layer = 4096, 3                                            # d = 8: 2048 pairs = 64 tiles per clip
    B = (3 * ncu + 63) // 64 + 1
    assert B * 64 >= 3 * ncu + 8                                  # (the walk hands each XCD an equal share: every workgroup gets >= 3)
    _check(rig, B, L, layer)


def test_four_byte_form_untouched(rig):
    _check(rig, 3, 194, 2)                                        # ragged length: 97 pairs, the 4-byte epilogue, no item


@pytest.mark.parametrize("layer", [0, 11])
def test_negative_part_t(rig, layer):
    _check(rig, 3, 4096, layer, pt_sign=-1)                       # d = 1, 2048, every part_t negative: out-of-clip taps stay +0 whatever its sign
