"""The F(2,3) fp32 block after its GEMM1 diet (the wrapped weight loads carried as the next tile's prefetch, no X request past the
last chunk, launch constants in LDS: audiopure_amd/csrc/ap_resblock_f32w.hip) against the kernel it replaced,
kept verbatim in the tools library (tools/csrc/ap_resblock_f32w_parent.hip): every output bit for bit -- the diet changes no
arithmetic and no summation order -- and two launches on the same inputs equal (a race in LDS would show there).

C = S = 256 throughout.  Shapes: L = 192 (16-byte epilogue) and 194 (ragged: the 4-byte form), both with a last partial tile;
L = 4096 with d = 1, 16 (d < 32), 32, 64 (d >= 32) and 2048 (a tail of orphan pairs); L = 64 with d = 128 (d >= L: every second
output masked); and one grid on which every workgroup owns at least three tiles, so that the carried prefetch crosses tile
turns.  Forms: h' with accumulate 0 and 1, the last layer's form (no h'), the SAVE form."""
import ctypes as C

import pytest
import torch

import __graft_entry__ as G
from audiopure_amd import synth, _native as N

pytestmark = pytest.mark.gpu

_vp, _i = C.c_void_p, C.c_int
_BLOCK_ARGS = [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]


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


def _run(fn, ctx, layer, h, pt, skip0, form, B, L, dev):
    """One launch of a form: (h' or None, skip, pre-gate rows or None).  Outputs start from sentinels / the given running skip."""
    accumulate = 0 if form == "acc0" else 1
    hout = None if form == "noh" else torch.full_like(h, 3.0)
    skip = skip0.clone() if accumulate else torch.full_like(skip0, 7.0)
    pre = torch.full((B, 512, L), 5.0, device=dev) if form == "save" else None
    rc = fn(ctx, layer, N.ptr(h), N.ptr(pt), N.ptr(hout), N.ptr(skip), accumulate, B, L, N.stream(), N.ptr(pre))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return hout, skip, pre


def _same(a, b, what):
    for x, y, name in zip(a, b, ("h'", "skip", "pre-gate")):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert torch.equal(x, y), f"{what}: {name} differs in {(x != y).sum().item()} of {x.numel()} elements"


def _check(rig, B, L, layer, forms):
    dev, eng, tl, ctx = rig
    g = torch.Generator(device="cpu").manual_seed(1000 * layer + L)
    h = (torch.rand(B, 256, L, generator=g) * 3 - 1.5).to(dev)
    skip0 = (torch.rand(B, 256, L, generator=g) * 2 - 1).to(dev)
    pt = (torch.rand(256, generator=g) * 2 - 1).to(dev)
    for form in forms:
        ref = _run(tl.ap_debug_resblock_f32w_parent, ctx, layer, h, pt, skip0, form, B, L, dev)
        new = _run(tl.ap_debug_resblock_f32w, ctx, layer, h, pt, skip0, form, B, L, dev)
        _same(new, ref, f"L={L} layer={layer} {form}")
        again = _run(tl.ap_debug_resblock_f32w, ctx, layer, h, pt, skip0, form, B, L, dev)
        _same(again, new, f"L={L} layer={layer} {form}, second launch")
        if form != "noh":                                         # the product library, through the entry points of include/audiopure.h
            accumulate = 0 if form == "acc0" else 1
            hout = torch.full_like(h, 3.0)
            skip = skip0.clone() if accumulate else torch.full_like(skip0, 7.0)
            pre = torch.full((B, 512, L), 5.0, device=dev) if form == "save" else None
            if form == "save":
                N.check(eng.lib.ap_resblock_fwd_save(eng.ctx, layer, N.ptr(h), N.ptr(pt), N.ptr(hout), N.ptr(skip), N.ptr(pre), accumulate, B, L, N.stream()))
            else:
                N.check(eng.lib.ap_resblock_fwd(eng.ctx, layer, N.ptr(h), N.ptr(pt), N.ptr(hout), N.ptr(skip), accumulate, B, L, N.stream()))
            torch.cuda.synchronize()
            _same((hout, skip, pre), ref, f"L={L} layer={layer} {form}, product library")


FORMS = ("acc0", "acc1", "noh", "save")


@pytest.mark.parametrize("L", [192, 194])
def test_partial_last_tile_both_epilogues(rig, L):
    _check(rig, 3, L, 2, FORMS)                                   # d = 4: 96 / 97 pairs = three full tiles and a partial one


@pytest.mark.parametrize("layer", [0, 4, 5, 6, 11])
def test_dilations(rig, layer):
    _check(rig, 3, 4096, layer, FORMS)                            # d = 1, 16, 32, 64, 2048


def test_dilation_past_the_clip(rig):
    _check(rig, 3, 64, 7, FORMS)                                  # d = 128 >= L: second outputs all masked


def test_three_tiles_per_workgroup(rig):
    dev = rig[0]
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    L, layer = 4096, 3                                            # d = 8: 2048 pairs = 64 tiles per clip
    B = (3 * ncu + 63) // 64 + 1
    assert B * 64 >= 3 * ncu + 8                                  # (the walk hands each XCD an equal share: every workgroup gets >= 3)
    _check(rig, B, L, layer, ("acc1", "save"))


def test_each_item_alone_equals_the_parent(rig):
    """The single-item instantiations tools/ab_f32w.py times (DIET masks 0, 2, 4 of the h'-writing 16-byte form) are the same
    function too, across tile turns -- an A/B figure must not come from a wrong kernel."""
    dev, eng, tl, ctx = rig
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    B, L, layer = (3 * ncu + 63) // 64 + 1, 4096, 5
    g = torch.Generator(device="cpu").manual_seed(77)
    h = (torch.rand(B, 256, L, generator=g) * 3 - 1.5).to(dev)
    skip0 = (torch.rand(B, 256, L, generator=g) * 2 - 1).to(dev)
    pt = (torch.rand(256, generator=g) * 2 - 1).to(dev)
    tl.ap_debug_f32w_diet.restype, tl.ap_debug_f32w_diet.argtypes = _i, [_i]
    ref = _run(tl.ap_debug_resblock_f32w_parent, ctx, layer, h, pt, skip0, "acc1", B, L, dev)
    try:
        for mask in (0, 2, 4):
            assert tl.ap_debug_f32w_diet(mask) == 0
            _same(_run(tl.ap_debug_resblock_f32w, ctx, layer, h, pt, skip0, "acc1", B, L, dev), ref, f"DIET mask {mask}")
    finally:
        assert tl.ap_debug_f32w_diet(6) == 0
