"""The F(2,3) fp32 block with fewer vector-ALU issue slots (audiopure_amd/csrc/ap_resblock_f32w.hip: DIET_PK_, the output transform and
the gate on accumulator register pairs -- gate2 of ap_device.h, v_pk_add / v_pk_mul / v_pk_fma_f32; DIET_ZERO_, chunk 0 peeled and
m1, m3, m4 started from the matrix instruction's constant 0 instead of zeroed registers) against the kernel kept verbatim in the tools library (tools/csrc/ap_resblock_f32w_parent.hip): h', skip and
the pre-gate rows bit for bit -- every element sees the operations it always did -- and a second launch equal to the first.

Every new mask (54, 150 = one item on top of 22; 182 = the product) on the h'-writing 16-byte form, the last layer's and the SAVE
form at the product's mask, and the product library through ap_resblock_fwd / ap_resblock_fwd_save.  C = S = 256, B = 3.  Shapes:
L = 192 (partial last tile); L = 4096 with d = 1, 16, 32, 2048 (d = 1 and 2048: out-of-clip taps on both sides); L = 64 with d = 128
(d >= L); L = 194 (the 4-byte form: no item); one grid with at least three tiles per workgroup.  Gate range: h scaled until the
PARENT's pre-gate rows pass the tanh clamp (+-15), the sigmoid clamp (-80) and F's large-argument side (+80) with every output
finite -- gate2's clamp, large- and tiny-argument paths then stand under the same bit equality.  One case with every
part_t negative: the zero padding of out-of-clip taps must not depend on part_t's sign."""
import ctypes as C

import pytest
import torch

import __graft_entry__ as G
from audiopure_amd import synth, _native as N

pytestmark = pytest.mark.gpu

_vp, _i = C.c_void_p, C.c_int
_BLOCK_ARGS = [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]
PRODUCT_MASK = 182
MASKS = (54, 150, 182)
FORMS = ("acc0", "acc1", "noh", "save")
GATE_SCALE = 64.0                                                 # x the plain cases' range of h (+-1.5): see test_gate_range


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


def _check(rig, B, L, layer, scale=1.0, pt_sign=0, on_parent_save=None):
    """pt_sign -1: every part_t negative.  on_parent_save(pre-gate rows, outputs): the input condition, stated on the parent's launch."""
    dev, eng, tl, ctx = rig
    g = torch.Generator(device="cpu").manual_seed(1000 * layer + L + 7)
    h = ((torch.rand(B, 256, L, generator=g) * 3 - 1.5) * scale).to(dev)
    skip0 = (torch.rand(B, 256, L, generator=g) * 2 - 1).to(dev)
    pt = torch.rand(256, generator=g) * 2 - 1
    if pt_sign < 0:
        pt = -pt.abs() - 0.01
        assert (pt < 0).all()
    pt = pt.to(dev)
    try:
        for form in FORMS:
            what = f"L={L} layer={layer} B={B} scale={scale} {form}"
            ref = _run(tl.ap_debug_resblock_f32w_parent, ctx, layer, h, pt, skip0, form, B, L, dev)   # once per form, shared
            if form == "save" and on_parent_save is not None:
                on_parent_save(ref[2], ref)
            # (the mask selects among the instantiations of the h'-writing form; the last layer's and the SAVE form have one)
            for mask in (MASKS if form in ("acc0", "acc1") else (PRODUCT_MASK,)):
                assert tl.ap_debug_f32w_diet(mask) == 0
                new = _run(tl.ap_debug_resblock_f32w, ctx, layer, h, pt, skip0, form, B, L, dev)
                _same(new, ref, f"{what}, mask {mask}")
                again = _run(tl.ap_debug_resblock_f32w, ctx, layer, h, pt, skip0, form, B, L, dev)
                _same(again, new, f"{what}, mask {mask}, second launch")
            if form != "noh":                                     # (no per-block entry point of include/audiopure.h reaches the last layer's form)
                new = _run_product(eng, layer, h, pt, skip0, form, B, L, dev)
                _same(new, ref, f"{what}, product library")
                again = _run_product(eng, layer, h, pt, skip0, form, B, L, dev)
                _same(again, new, f"{what}, product library, second launch")
    finally:
        assert tl.ap_debug_f32w_diet(PRODUCT_MASK) == 0


def test_masks_exist(rig):
    tl = rig[2]
    try:
        for mask in (0, 2, 4, 6, 22) + MASKS:
            assert tl.ap_debug_f32w_diet(mask) == 0, mask
        assert tl.ap_debug_f32w_diet(118) != 0                    # (no such instantiation: refused, not served by another)
    finally:
        assert tl.ap_debug_f32w_diet(PRODUCT_MASK) == 0


def test_partial_last_tile(rig):
    _check(rig, 3, 192, 2)                                        # d = 4: 96 pairs = three tiles, the last one partial


@pytest.mark.parametrize("layer", [0, 4, 5, 11])
def test_dilations(rig, layer):
    _check(rig, 3, 4096, layer)                                   # d = 1, 16 (d < 32), 32 (d >= 32), 2048; d = 1, 2048: taps past both ends


def test_dilation_past_the_clip(rig):
    _check(rig, 3, 64, 7)                                         # d = 128 >= L: every second output masked, every +-d tap outside


def test_three_tiles_per_workgroup(rig):
    dev = rig[0]
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    L, layer = 4096, 3                                            # d = 8: 2048 pairs = 64 tiles per clip
    B = (3 * ncu + 63) // 64 + 1
    assert B * 64 >= 3 * ncu + 8                                  # (the walk hands each XCD an equal share: every workgroup gets >= 3)
    _check(rig, B, L, layer)


def test_four_byte_form_untouched(rig):
    _check(rig, 3, 194, 2)                                        # ragged length: 97 pairs, the 4-byte epilogue, no item


@pytest.mark.parametrize("L", [192, 4096])
def test_gate_range(rig, L):
    """h at GATE_SCALE x the plain range: the parent's own pre-gate rows must reach past both clamps and F's overflow side."""
    def reaches(pre, outs):
        th, sg = pre[:, :256], pre[:, 256:]
        figures = (f"tanh half [{th.min().item():.1f}, {th.max().item():.1f}], sigmoid half [{sg.min().item():.1f}, {sg.max().item():.1f}]; "
                   f"beyond +-15: {(th.abs() > 15).sum().item()}, below -80: {(sg < -80).sum().item()}, above +80: {(sg > 80).sum().item()}")
        print(f"gate range L={L} scale={GATE_SCALE}: {figures}")
        assert (th > 15).any() and (th < -15).any(), figures
        assert (sg < -80).any(), figures
        assert (sg > 80).any(), figures
        for t in outs:
            assert torch.isfinite(t).all(), figures
    _check(rig, 3, L, 5, scale=GATE_SCALE, on_parent_save=reaches)


def test_negative_part_t(rig):
    _check(rig, 3, 4096, 0, pt_sign=-1)                           # d = 1, every part_t negative: out-of-clip taps stay +0 whatever its sign
