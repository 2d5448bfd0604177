"""ap_conv2d_wgrad where conv2d_wgrad_kernel branches, through the C-ABI on INTEGER data compared EXACTLY with the float64 reference
(the method of test_gpu_wgrad_edges.py): every sum stays below 2^24, so any summation order gives the same integers and one
misplaced sample, one padded position read as data, one column of the wrong group or one dropped chunk fails.  dW and the workspace
start NaN-filled on every call; the workspace has exactly the size the query returned."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiopure_amd import synth  # noqa: E402
from audiopure_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")

# name: (B, Cin, H, W, Cout, k, stride, pad, groups, x_cstride, x_coff) -- each the smallest geometry at which something branches
CASES = {
    "one_tile_one_chunk": (2, 32, 4, 4, 32, 1, 1, 0, 1, 32, 0),            # k1 s1, M = N = 32, K = 32: both operands by 16-byte loads
    "stem_9_columns": (3, 1, 8, 8, 64, 3, 1, 1, 1, 1, 0),                  # Cin = 1: 9 columns, gathered x
    "group_width_16": (2, 32, 8, 8, 32, 3, 2, 1, 2, 32, 0),                # 8x8 -> 4x4, groups 2 of width 16: narrower than a tile
    "odd_7x7": (2, 32, 7, 7, 32, 3, 2, 1, 1, 32, 0),                       # 7x7 -> 4x4: padding reaches one side only at the far edge
    "shortcut_k1_s2": (2, 32, 8, 8, 64, 1, 2, 0, 1, 32, 0),                # the strided 1 x 1: gathered although k = 1
    "resnet_stem_7x7": (2, 1, 16, 16, 64, 7, 2, 3, 1, 1, 0),               # 49 columns
    "linear": (5, 64, 1, 1, 10, 1, 1, 0, 1, 64, 0),                        # H = W = 1: K = B = 5 below one chunk, M = 10 ragged, scalar loads
    "groups_8x64": (2, 512, 4, 4, 512, 3, 1, 1, 8, 512, 0),                # tiles must not cross groups
    "remainder_tiles": (2, 96, 4, 4, 160, 3, 1, 1, 1, 96, 0),              # M = 160 = 128 + 32, N = 864 = 13 x 64 + 32
    "slice_operand": (2, 32, 4, 4, 32, 3, 1, 1, 1, 64, 16),                # x = channels [16, 48) of 64
    "slice_operand_k1": (2, 32, 4, 4, 64, 1, 1, 0, 1, 64, 16),             # ... by 16-byte loads
    "deep_K": (9, 64, 16, 16, 256, 3, 1, 1, 1, 64, 0),                     # K = 2304 = 72 chunks over 29 slices of 2 or 3, walking image to image
    "deep_K_odd": (9, 32, 5, 5, 32, 3, 1, 1, 1, 32, 0),                    # OH OW = 25: chunks straddle images, scalar dy loads
}


def geometry(c):
    B, Cin, H, W, Cout, k, s, pad, g, cs, co = c
    return (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


@functools.lru_cache(maxsize=None)
def integer_inputs(name):
    """x in {-2..2}, dy in {-1, 0, 1} (asymmetric patterns, keyed by name), an integer prior; and the float64 reference."""
    c = CASES[name]
    B, Cin, H, W, Cout, k, s, pad, g, cs, co = c
    OH, OW = geometry(c)
    x = torch.from_numpy(synth.uniform("cwg/x/" + name, (B, cs, H, W), 0, -2.49, 2.49)).round()
    dy = torch.from_numpy(synth.uniform("cwg/dy/" + name, (B, Cout, OH, OW), 0, -1.49, 1.49)).round()
    prior = torch.from_numpy(synth.uniform("cwg/pr/" + name, (Cout, Cin // g, k, k), 0, -8.49, 8.49)).round()
    return x, dy, prior, reference(x, dy, c)


def reference(x, dy, c):
    B, Cin, H, W, Cout, k, s, pad, g, cs, co = c
    xs = x[:, co:co + Cin].double().requires_grad_(False)
    w = torch.zeros((Cout, Cin // g, k, k), dtype=torch.float64, requires_grad=True)
    F.conv2d(xs, w, None, s, pad, 1, g).backward(dy.double())
    assert float(w.grad.abs().max()) < 2 ** 24
    return w.grad.detach()


def wgrad(dev, x, dy, c, dW=None, accumulate=0):
    lib = N.lib()
    B, Cin, H, W, Cout, k, s, pad, g, cs, co = c
    need = lib.ap_conv2d_wgrad_workspace_bytes(B, Cin, H, W, Cout, k, k, s, pad, g)
    assert need > 0 and need % 4 == 0
    ws = torch.full((need // 4,), NAN, device=dev)
    if dW is None:
        dW = torch.full((Cout, Cin // g, k, k), NAN, device=dev)
    N.check(lib.ap_conv2d_wgrad(N.ptr(dy), N.ptr(x), N.ptr(dW), ws.data_ptr(), need, B, Cin, H, W, Cout, k, k, s, pad, g, cs, co, accumulate,
                                N.stream()), "ap_conv2d_wgrad")
    return dW


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", list(CASES))
def test_integer_data_gives_the_exact_sum(dev, name):
    """From a NaN-filled dW and workspace; then accumulate = 1 onto an integer prior; then the same call again: equal bits."""
    c = CASES[name]
    x, dy, prior, ref = integer_inputs(name)
    xd, dyd = x.to(dev), dy.to(dev)
    G = wgrad(dev, xd, dyd, c)
    Gc = G.cpu().double()
    assert not torch.isnan(Gc).any(), "the reduction read a workspace slot this call did not write, or an element was not stored"
    bad = Gc != ref
    assert torch.equal(Gc, ref), (f"{int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}, by up to "
                                  f"{float((Gc - ref).abs().max())}")
    assert float(ref.abs().max()) > 0
    G2 = wgrad(dev, xd, dyd, c, dW=prior.to(dev), accumulate=1)
    assert torch.equal(G2.cpu().double(), prior.double() + ref)
    assert torch.equal(wgrad(dev, xd, dyd, c), G)


def test_nine_one_image_calls_add_up_to_the_nine_image_call(dev):
    """Batch additivity: each image alone has another slicing (8 chunks in 8 slices), the integers are the same."""
    name = "deep_K"
    c = CASES[name]
    x, dy, _, ref = integer_inputs(name)
    xd, dyd = x.to(dev), dy.to(dev)
    whole = wgrad(dev, xd, dyd, c)
    acc = torch.zeros_like(whole)
    one = (1,) + c[1:]
    for b in range(c[0]):
        wgrad(dev, xd[b:b + 1].contiguous(), dyd[b:b + 1].contiguous(), one, dW=acc, accumulate=1)
    assert torch.equal(acc, whole) and torch.equal(whole.cpu().double(), ref)


def test_real_data_two_runs_equal_bits_and_within_float32_of_float64(dev):
    """Uniform data on the deep case.  A slice is an fp32 fma chain of at most 96 positions (one rounding of unit u = 2^-24 per
    product), the 29 slices are added in fp64: with rounding errors adding up as a random walk an element's error is about
    sqrt(96) u sum |dy x|, the bound here (the worst case, 96 u sum |dy x|, is ten times it)."""
    c = CASES["deep_K"]
    B, Cin, H, W, Cout, k, s, pad, g, cs, co = c
    x = torch.from_numpy(synth.uniform("cwg/rx", (B, cs, H, W), 1, -2.0, 2.0))
    dy = torch.from_numpy(synth.uniform("cwg/rdy", (B, Cout, H, W), 1, -1.0, 1.0))
    ref, mag = reference(x, dy, c), reference(x.abs(), dy.abs(), c)
    G1 = wgrad(dev, x.to(dev), dy.to(dev), c)
    G2 = wgrad(dev, x.to(dev), dy.to(dev), c)
    assert torch.equal(G1, G2)
    ratio = float(((G1.cpu().double() - ref).abs() / (96 ** 0.5 * 2.0 ** -24 * mag)).max())
    print(f"max |dW - ref| / (sqrt(96) u sum |dy x|) = {ratio:.3f}; max |dW - ref| / max |ref| = "
          f"{float((G1.cpu().double() - ref).abs().max()) / float(ref.abs().max()):.3e}")
    assert ratio <= 1.0


def test_refused_before_any_launch(dev):
    lib = N.lib()
    t = torch.ones(2 * 32 * 8 * 8, device=dev)
    G = torch.full((32 * 32 * 9,), NAN, device=dev)
    ws = torch.full((1 << 20,), NAN, device=dev)
    wsb = ws.numel() * 4

    def call(Cin=32, Cout=32, kh=3, kw=3, stride=1, pad=1, groups=1, cs=32, co=0, w=ws.data_ptr(), wb=wsb):
        return lib.ap_conv2d_wgrad(N.ptr(t), N.ptr(t), N.ptr(G), w, wb, 2, Cin, 8, 8, Cout, kh, kw, stride, pad, groups, cs, co, 0, N.stream())

    assert call(kh=3, kw=1) == -22 and b"square" in lib.ap_last_error()
    assert call(pad=3) == -22 and b"pad" in lib.ap_last_error()
    assert call(groups=3) == -22 and b"groups" in lib.ap_last_error()
    assert call(Cin=30, groups=4) == -22 and call(kh=5, kw=5) == -22 and call(stride=3) == -22 and call(co=1) == -22
    assert call(w=None) == -22 and call(wb=16) == -22 and b"workspace" in lib.ap_last_error()
    assert lib.ap_conv2d_wgrad_workspace_bytes(2, 32, 8, 8, 32, 3, 1, 1, 1, 1) == 0
    torch.cuda.synchronize()
    assert torch.isnan(G).all() and torch.isnan(ws).all()         # nothing was launched
    N.check(call(), "ap_conv2d_wgrad")                            # and the same arguments, valid, are served
    torch.cuda.synchronize()
    assert not torch.isnan(G).any()


def test_pack_bwd_writes_the_image_of_the_flipped_transposed_weight(dev):
    """ap_conv2d_pack_bwd on the live weight == ap_conv2d_pack of the torch permute / flip NativeConvNet._prepare_backward builds,
    bit for bit, for a grouped 3 x 3, a streamed-weight 1 x 1 and the stem."""
    lib = N.lib()
    for Cout, Cg, k, g in ((32, 16, 3, 2), (128, 64, 1, 1), (64, 1, 7, 1), (64, 64, 3, 1)):
        w = torch.from_numpy(synth.uniform(f"cwg/w{Cout}{k}", (Cout, Cg, k, k), 0)).to(dev)
        n = lib.ap_conv2d_packed_elems(g * Cg, Cout // g, k, k, g)
        got, want = torch.full((n,), NAN, device=dev), torch.full((n,), NAN, device=dev)
        scratch = torch.full((w.numel(),), NAN, device=dev)
        N.check(lib.ap_conv2d_pack_bwd(N.ptr(w), N.ptr(got), N.ptr(scratch), Cout, Cg, k, k, g, N.stream()), "ap_conv2d_pack_bwd")
        wt = w.reshape(g, Cout // g, Cg, k, k).permute(0, 2, 1, 3, 4).flip(3, 4).reshape(g * Cg, Cout // g, k, k).contiguous()
        N.check(lib.ap_conv2d_pack(N.ptr(wt), None, N.ptr(want), g * Cg, Cout // g, k, k, g, N.stream()), "ap_conv2d_pack")
        assert torch.equal(scratch.view_as(wt), wt)
        assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0))
    assert lib.ap_conv2d_pack_bwd(N.ptr(w), N.ptr(got), N.ptr(scratch), 64, 64, 3, 1, 1, N.stream()) == -22
