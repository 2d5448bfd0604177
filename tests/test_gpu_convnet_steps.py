"""The 2-D classifier executor (audiopure_amd/convnet.py on ap_convnet.hip / ap_backward.hip) one step at a time and off the 32 x 32
square: every forward step against the plan oracle on the executor's own input buffers, the input gradient and every intermediate
gradient against the oracle's linearised replay (ReLU masks and max-pool positions taken from the native forward, so no selection
can flip between the two and the comparison is to rounding), the element-wise entry points alone, and ap_conv2d_fwd with H != W.

Inputs 1 x 40 x 32 (the scripts' mel40 front-end) and 1 x 33 x 47: at 33 x 47 the stride-2 convolutions have
(H + 2 pad - k) % stride == 0 on one or both axes (1 x 1: (0, 0); 3 x 3 / pad 1: (0, 0) on 33 x 47, (0, 1) on 17 x 24), so the
transposed convolution's zero-inserted map has no extra row / column there, and the poolings floor an odd map (2/2/0 on 5 x 4,
3/2/1 on 17 x 24, 4/4/0 on 5 x 6).

GRAD_TOL.  The reference's own arithmetic error: the same linearised replay evaluated in float32 and in float64 on the CPU, selections
from a float32 pass over the plan, B = 3, worst of {input gradient, every step's output gradient}, max |a - b| / max |b|:

    network     1 x 32 x 32   1 x 40 x 32   1 x 33 x 47
    vgg19_bn/8    7.70e-07      7.46e-07      8.38e-07
    DenseDPN      4.34e-07      5.41e-07      3.92e-07
    _CatSliceNet  2.62e-07      3.11e-07      3.18e-07

Worst 8.38e-07 (REPLAY_F32_ERR = 8.4e-7); the kernels sum in another order than torch and split the reduction across MFMA tiles, so
four times the worst value is allowed: GRAD_TOL = 3.35e-6.  (tests/test_convnet_lowering_cpu.py re-measures the figure on every run
and holds the replay itself to autograd through the module.)"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from audiopure_amd import synth
from audiopure_amd import _native as N
from audiopure_amd.convnet import NativeConvNet
from conftest import rel_err
from oracle.convnet_plan_oracle import read_val, replay_gradients, step_torch
from synth_convnets import FAMILIES, synth_init, vgg19_bn
from test_convnet_lowering_cpu import DenseDPN
from test_gpu_convnets import TOL
from test_gpu_grad import _CatSliceNet, _guarded

pytestmark = pytest.mark.gpu

REPLAY_F32_ERR = 8.4e-7
GRAD_TOL = 3.35e-6
CONV_TOL = 6e-6          # tools/fuzz_conv.py's bound for the same kernels at K = 3200 (these nets: K <= 576)
STEP_NETS = {"vgg19_bn_w8": lambda: vgg19_bn(10, 1, width_div=8), "DenseDPN": DenseDPN, "CatSliceNet": _CatSliceNet}
STEP_SHAPES = [(1, 40, 32), (1, 33, 47)]
GRAD_SHAPES = [(1, 32, 32), (1, 40, 32), (1, 33, 47)]


def step_case(name, chw, B=3):
    """-> (eval-mode module, input [B, *chw], cotangent of its output): fixed by (name, chw) alone."""
    m = synth_init(STEP_NETS[name](), 5).eval()
    x = torch.from_numpy(synth.uniform(f"st/{name}", (B,) + tuple(chw), 1, -2.0, 2.0))
    with torch.no_grad():
        n_out = m(x[:1]).shape[1]
    return m, x, torch.from_numpy(synth.uniform("st/dout", (B, n_out), 1, -1.0, 1.0))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _describe(i, s):
    return f"step {i} {s.kind} {s.p} out={s.out} ins={s.ins}"


# ---------------------------------------------------------------------------------------------------------
# a. forward, one step at a time
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "f32s"])
@pytest.mark.parametrize("chw", STEP_SHAPES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("name", sorted(STEP_NETS))
def test_every_forward_step_matches_the_plan_oracle_on_its_own_inputs(dev, name, chw, mode):
    """Each step's output buffer against oracle.step_torch on the NATIVE input buffers: copy / add / max-pool bit-identical to the
    float32 computation (one fp32 add, or a selection, has one right answer), affine / average pool within 1e-6 of float64 (one
    fused-vs-unfused rounding), conv within fuzz_conv's 6e-6; and the logits against the fp32 module."""
    m, x, _ = step_case(name, chw)
    net = NativeConvNet(m, chw).eval().set_precision(mode)
    with torch.no_grad():
        out, bufs = net._run(x.to(dev))
        ref = m(x)
    torch.cuda.synchronize()
    cb = {k: v.cpu() for k, v in bufs.items()}
    plan = net.plan
    kinds = set()
    for i, s in enumerate(plan.steps):
        got = read_val(cb, s.out)
        exact = s.kind in ("copy", "add") or (s.kind == "pool" and s.p["is_max"])
        kinds.add(s.kind)
        if exact:
            assert torch.equal(got, step_torch(plan, s, cb, torch.float32)), _describe(i, s)
        else:
            e = rel_err(got.numpy(), step_torch(plan, s, cb, torch.float64).numpy())
            print(f"{name} {chw} {mode} step {i} {s.kind}: {e:.2e}")
            assert e < (CONV_TOL if s.kind == "conv" else 1e-6), (e, _describe(i, s))
    assert {"conv", "pool"} <= kinds
    e = rel_err(out.cpu().numpy(), ref.numpy())
    print(f"{name} {chw} {mode} logits: {e:.2e}")
    assert e < TOL


# resnext29_8_64 and resnet50 are left out: their own `view` before the classifier fails at 1 x 40 x 32 on the CPU as well (the
# pooled map is no longer 1 x 1), so there is nothing to compare with
@pytest.mark.parametrize("name", ["vgg19_bn", "wideresnet28_10", "dpn92", "densenet_bc_100_12"])
def test_full_width_families_on_the_mel40_input(dev, name):
    """The families of models/__init__.py that accept the mel40 front-end's 1 x 40 x 32 at full width: logits against the module."""
    m = synth_init(FAMILIES[name](), 0).eval()
    x = torch.from_numpy(synth.uniform("mel40", (2, 1, 40, 32), 3, -2.0, 2.0))
    with torch.no_grad():
        ref = m(x).numpy()
    y = NativeConvNet(m, (1, 40, 32)).eval()(x.to(dev)).cpu().numpy()
    e = rel_err(y, ref)
    print(f"{name} 1x40x32 logits: {e:.2e}")
    assert y.shape == ref.shape and e < TOL


# ---------------------------------------------------------------------------------------------------------
# b. input gradient, and every step's output gradient, against the linearised replay
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "f32s"])
@pytest.mark.parametrize("chw", GRAD_SHAPES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("name", sorted(STEP_NETS))
def test_every_gradient_of_the_reverse_sweep_matches_the_linearised_replay(dev, name, chw, mode):
    """NativeConvNet._input_grad's input gradient AND the gradient of every step's output value against the float64 replay of the
    plan with the native forward's ReLU masks and max-pool positions (oracle.replay_linearised): with the selections shared the
    map dout -> gradients is linear, so GRAD_TOL is rounding only -- a border window of pool2d_bwd_kernel, one wrong tap of a
    flipped / grouped weight image, a slice offset of ap_acc_channels or a mis-sized zero-inserted map cannot hide under it."""
    m, x, dout = step_case(name, chw)
    net = NativeConvNet(m, chw).eval().set_precision(mode)
    keep = {}
    with torch.no_grad():
        out, bufs = net._run(x.to(dev))
        dx = net._input_grad(bufs, dout.to(dev), keep=keep)
    torch.cuda.synchronize()
    cb = {k: v.cpu() for k, v in bufs.items()}
    cg = {k: v.cpu() for k, v in keep.items()}
    plan = net.plan
    dx_ref, g_ref = replay_gradients(plan, cb, dout)
    worst = 0.0
    for i in range(len(plan.steps) - 1, -1, -1):                     # the sweep's order: the first failure is the step at fault
        s, ref = plan.steps[i], g_ref[i]
        got = read_val(cg, s.out) if s.out.buf in cg else None
        if ref is None:                                              # nothing downstream reads this value
            assert got is None or not bool(got.any()), _describe(i, s)
            continue
        got = torch.zeros(ref.shape) if got is None else got
        e = rel_err(got.numpy(), ref.numpy())
        worst = max(worst, e)
        assert e < GRAD_TOL, (f"gradient of the output of {_describe(i, s)}: {e:.3e}")
    e = rel_err(dx.cpu().numpy(), dx_ref.numpy())
    print(f"{name} {chw} {mode}: input gradient {e:.2e}, worst step gradient {worst:.2e}")
    assert dx.shape == x.shape and e < GRAD_TOL, e
    # the default call (no keep) is the same arithmetic
    with torch.no_grad():
        assert torch.equal(net._input_grad(bufs, dout.to(dev)), dx)


# ---------------------------------------------------------------------------------------------------------
# c. the element-wise entry points alone
# ---------------------------------------------------------------------------------------------------------
def _u(name, shape, seed=1, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform(name, tuple(shape), seed, lo, hi))


@pytest.mark.parametrize("quantised", [False, True], ids=["continuous", "ties"])
@pytest.mark.parametrize("k,stride,pad", [(2, 2, 0), (3, 2, 1), (3, 1, 1), (4, 4, 0), (8, 1, 0)])
@pytest.mark.parametrize("is_max", [1, 0], ids=["max", "avg"])
def test_pool2d_and_its_backward(dev, is_max, k, stride, pad, quantised):
    """ap_pool2d / ap_pool2d_bwd against torch on the CPU: forward and max backward bit-identical to the float32 computation (the
    same selections -- with ties, the first maximum in row-major order -- and the same order of the fp32 sums), everything within
    1e-6 of float64; odd maps whose last rows / columns no window covers, windows over the padding, overlapping windows."""
    lib = N.lib()
    BC, ran = 7, 0
    for (H, W) in [(5, 4), (17, 24), (7, 9), (8, 8)]:
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        if H + 2 * pad < k or W + 2 * pad < k:
            continue                                                 # empty output
        ran += 1
        x = _u(f"pl/x{H}{W}", (1, BC, H, W), 2, -2.0, 2.0)
        if quantised:
            x = torch.round(x * 2) / 2                               # multiples of 0.5: windows hold ties
        dy = _u(f"pl/dy{Ho}{Wo}", (1, BC, Ho, Wo), 3)
        pool = F.max_pool2d if is_max else F.avg_pool2d
        xr, xr64 = x.clone().requires_grad_(True), x.double().requires_grad_(True)
        y32, y64 = pool(xr, k, stride, pad), pool(xr64, k, stride, pad)
        assert tuple(y32.shape) == (1, BC, Ho, Wo)
        (dx32,) = torch.autograd.grad(y32, xr, dy)
        (dx64,) = torch.autograd.grad(y64, xr64, dy.double())
        xd, dyd = x.to(dev), dy.to(dev)
        _, y, y_ok = _guarded((1, BC, Ho, Wo), dev)
        _, dx, dx_ok = _guarded((1, BC, H, W), dev)
        N.check(lib.ap_pool2d(N.ptr(xd), N.ptr(y), BC, H, W, k, stride, pad, is_max, N.stream()))
        N.check(lib.ap_pool2d_bwd(N.ptr(xd), N.ptr(dyd), N.ptr(dx), BC, H, W, k, stride, pad, is_max, N.stream()))
        case = (H, W, k, stride, pad, is_max, quantised)
        assert torch.equal(y.cpu(), y32.detach()), case
        assert rel_err(y.cpu().numpy(), y64.detach().numpy()) < 1e-6, case
        if is_max:
            assert torch.equal(dx.cpu(), dx32), case
        assert rel_err(dx.cpu().numpy(), dx64.numpy()) < 1e-6, case
        y_ok(); dx_ok()
    assert ran >= 2


@pytest.mark.parametrize("stride", [2, 3])
def test_zero_insert2d(dev, stride):
    """out [BC][Hz][Wz] = dy on the stride grid, zeros elsewhere, with Hz - ((Ho - 1) s + 1) in {0, 1} independently per axis (0: the
    strided convolution's (H + 2 pad - k) % s == 0); a map too small for the grid is refused and nothing is written."""
    lib = N.lib()
    BC, Ho, Wo = 5, 3, 4
    dy = _u("zi/dy", (BC, Ho, Wo), stride)
    dyd = dy.to(dev)
    for eh in (0, 1):
        for ew in (0, 1):
            Hz, Wz = (Ho - 1) * stride + 1 + eh, (Wo - 1) * stride + 1 + ew
            ref = torch.zeros(BC, Hz, Wz)
            ref[:, 0:(Ho - 1) * stride + 1:stride, 0:(Wo - 1) * stride + 1:stride] = dy
            _, out, ok = _guarded((BC, Hz, Wz), dev)
            N.check(lib.ap_zero_insert2d(N.ptr(dyd), N.ptr(out), BC, Ho, Wo, Hz, Wz, stride, N.stream()))
            assert torch.equal(out.cpu(), ref), (stride, eh, ew)
            ok()
    for (Hz, Wz) in (((Ho - 1) * stride, (Wo - 1) * stride + 1), ((Ho - 1) * stride + 1, (Wo - 1) * stride)):
        _, out, ok = _guarded((BC, Hz, Wz), dev)
        assert lib.ap_zero_insert2d(N.ptr(dyd), N.ptr(out), BC, Ho, Wo, Hz, Wz, stride, N.stream()) == -22
        torch.cuda.synchronize()
        assert bool((out == 5.0).all())
        ok()


@pytest.mark.parametrize("HW", [1, 25, 64])
def test_acc_channels(dev, HW):
    """dst[:, d_coff : d_coff + C] += src[:, s_coff : s_coff + C] with both sides slices of wider tensors at non-zero offsets and a
    non-zero destination: exactly dst + src inside the slice, untouched outside; a source slice past its tensor is refused."""
    lib = N.lib()
    B, Cn, s_cs, s_co, d_cs, d_co = 2, 5, 9, 3, 11, 4
    src, dst0 = _u("ac/s", (B, s_cs, HW), HW), _u("ac/d", (B, d_cs, HW), HW + 1)
    ref = dst0.clone()
    ref[:, d_co:d_co + Cn] = dst0[:, d_co:d_co + Cn] + src[:, s_co:s_co + Cn]
    srcd = src.to(dev)
    _, dst, ok = _guarded((B, d_cs, HW), dev)
    dst.copy_(dst0)
    N.check(lib.ap_acc_channels(N.ptr(srcd), N.ptr(dst), B, Cn, HW, s_cs, s_co, d_cs, d_co, N.stream()))
    assert torch.equal(dst.cpu(), ref)
    ok()
    assert lib.ap_acc_channels(N.ptr(srcd), N.ptr(dst), B, Cn, HW, s_co + Cn - 1, s_co, d_cs, d_co, N.stream()) == -22
    assert lib.ap_acc_channels(N.ptr(srcd), N.ptr(dst), B, Cn, HW, s_cs, s_co, d_co + Cn - 1, d_co, N.stream()) == -22
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), ref)
    ok()


def test_relu_mask(dev):
    """out = y > 0 ? dy : 0 -- +0.0 and -0.0 are not positive; n is no multiple of the workgroup."""
    lib = N.lib()
    n = 1037
    y, dy = _u("rm/y", (n,), 1), _u("rm/dy", (n,), 2)
    y[::7] = 0.0
    y[3::11] = -0.0
    ref = torch.where(y > 0, dy, torch.zeros(()))
    yd, dyd = y.to(dev), dy.to(dev)
    _, out, ok = _guarded((n,), dev)
    N.check(lib.ap_relu_mask(N.ptr(dyd), N.ptr(yd), N.ptr(out), n, N.stream()))
    got = out.cpu()
    assert torch.equal(got, ref) and float(got[0]) == 0.0 and float(got[3]) == 0.0 and 0 < int((got != 0).sum()) < n
    ok()


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("scaled", [False, True])
def test_affine_nchw(dev, scaled, relu):
    """y = [relu](x * scale[c] + shift[c]) of a channel slice: within 1e-6 of float64 (one fused-vs-unfused rounding); without scale
    a (ReLU'd) copy of the slice, exact.  scale without shift is refused."""
    lib = N.lib()
    B, Cn, HW, cs, co = 2, 5, 35, 9, 2
    x = _u("af/x", (B, cs, HW), 1, -2.0, 2.0)
    sc, sh = _u("af/s", (Cn,), 2, 0.5, 2.0), _u("af/h", (Cn,), 3)
    ref = x[:, co:co + Cn].double()
    if scaled:
        ref = ref * sc.double().view(1, -1, 1) + sh.double().view(1, -1, 1)
    if relu:
        ref = F.relu(ref)
    xd, scd, shd = x.to(dev), sc.to(dev), sh.to(dev)
    _, y, ok = _guarded((B, Cn, HW), dev)
    N.check(lib.ap_affine_nchw(N.ptr(xd), N.ptr(scd) if scaled else None, N.ptr(shd) if scaled else None, N.ptr(y), B, Cn, HW, cs, co,
                               relu, N.stream()))
    if scaled:
        assert rel_err(y.cpu().numpy(), ref.numpy()) < 1e-6
    else:
        assert torch.equal(y.cpu(), ref.float())
    ok()
    if scaled and not relu:
        _, y2, ok2 = _guarded((B, Cn, HW), dev)
        assert lib.ap_affine_nchw(N.ptr(xd), N.ptr(scd), None, N.ptr(y2), B, Cn, HW, cs, co, 0, N.stream()) == -22
        torch.cuda.synchronize()
        assert bool((y2 == 5.0).all())
        ok2()


@pytest.mark.parametrize("relu", [0, 1])
def test_add_nchw(dev, relu):
    """y = [relu](a + b) on two different channel slices: one fp32 add, exact."""
    lib = N.lib()
    B, Cn, HW = 3, 6, 35
    a, b = _u("ad/a", (B, 10, HW), 1, -2.0, 2.0), _u("ad/b", (B, 13, HW), 2, -2.0, 2.0)
    ref = a[:, 3:3 + Cn] + b[:, 7:7 + Cn]
    if relu:
        ref = F.relu(ref)
    ad, bd = a.to(dev), b.to(dev)
    _, y, ok = _guarded((B, Cn, HW), dev)
    N.check(lib.ap_add_nchw(N.ptr(ad), N.ptr(bd), N.ptr(y), B, Cn, HW, 10, 3, 13, 7, relu, N.stream()))
    assert torch.equal(y.cpu(), ref)
    ok()


def test_silu(dev):
    """x * sigmoid(x) on [-20, 20], n no multiple of the workgroup: within 1e-6 of float64."""
    lib = N.lib()
    n = 4099
    x = _u("si/x", (n,), 1, -20.0, 20.0)
    x[0], x[1], x[2] = -20.0, 20.0, 0.0
    xd = x.to(dev)
    _, y, ok = _guarded((n,), dev)
    N.check(lib.ap_silu(N.ptr(xd), N.ptr(y), n, N.stream()))
    ref = x.double() * torch.sigmoid(x.double())
    assert rel_err(y.cpu().numpy(), ref.numpy()) < 1e-6
    ok()


@pytest.mark.parametrize("L", [1, 63, 64, 130])
@pytest.mark.parametrize("Cn", [64, 30, 7])
def test_init_conv_bwd(dev, Cn, L):
    """dx[b][t] = sum_c [h0 > 0] w0[c] dh0[b][c][t]: channel quarters of uneven size (30: 8 8 8 6, 7: 2 2 2 1), the 8-wide loop
    with and without a tail, one sample up to three 64-sample workgroups with a ragged last one."""
    lib = N.lib()
    B = 2
    h0, w0, dh0 = _u(f"ic/h{Cn}", (B, Cn, L), L), _u("ic/w", (Cn,), Cn), _u(f"ic/d{Cn}", (B, Cn, L), L + 1)
    h0[:, ::3] = F.relu(h0[:, ::3])                                  # what a ReLU output looks like: exact zeros
    ref = ((h0 > 0).double() * w0.double().view(1, -1, 1) * dh0.double()).sum(1, keepdim=True)
    h0d, w0d, dh0d = h0.to(dev), w0.to(dev), dh0.to(dev)
    _, dx, ok = _guarded((B, 1, L), dev)
    N.check(lib.ap_init_conv_bwd(N.ptr(h0d), N.ptr(w0d), N.ptr(dh0d), N.ptr(dx), B, Cn, L, N.stream()))
    assert rel_err(dx.cpu().numpy(), ref.numpy()) < 1e-6, (Cn, L)
    ok()


# ---------------------------------------------------------------------------------------------------------
# d. ap_conv2d_fwd off the square
# ---------------------------------------------------------------------------------------------------------
# (B, Cin, H, W, Cout, k, stride, pad, groups, bias, residual, relu): test_conv2d_primitive_edge_shapes' layers with W != H -- an
# H / W mix-up in the addressing (stride 2 and groups included) passes every square case -- and padding above k // 2, which the
# backward pass needs when the forward padding is below k // 2 (k - 1 - pad).
OFF_SQUARE = [(3, 8, 9, 5, 12, 3, 1, 1, 1, 1, 0, 1), (2, 16, 16, 10, 40, 3, 2, 1, 4, 1, 1, 0), (5, 33, 7, 4, 70, 1, 1, 0, 1, 0, 1, 1),
              (33, 32, 32, 20, 200, 3, 1, 1, 1, 1, 1, 1), (70, 64, 31, 18, 272, 3, 2, 1, 2, 1, 0, 1), (40, 48, 30, 17, 160, 1, 1, 0, 1, 1, 1, 0),
              (36, 24, 32, 12, 136, 3, 1, 1, 1, 0, 0, 1), (7, 32, 5, 9, 200, 3, 1, 1, 1, 1, 1, 1), (9, 128, 16, 6, 176, 3, 1, 1, 2, 0, 1, 0),
              (4, 16, 6, 11, 64, 3, 1, 2, 1, 1, 0, 1), (2, 8, 5, 8, 24, 5, 1, 4, 1, 1, 1, 0),
              # narrowing W takes the three largest layers below the 512 tiles of the 128 x 128 kernels (streamed-weight and LDS-staged):
              # the same layers with W != H and their tile count kept
              (33, 32, 32, 40, 200, 3, 1, 1, 1, 1, 1, 1), (70, 64, 31, 36, 272, 3, 2, 1, 2, 1, 0, 1), (36, 24, 32, 30, 136, 3, 1, 1, 1, 0, 1, 1)]
# kernel classes (ap_conv_profile_read: 0 big2<128,128>, 1 big2<64,128>, 2 big2<128,64> / <64,64>, 3 split-operand, 4 LDS-staged
# 128 x 128, 5 generic) that test_conv2d_primitive_edge_shapes' square list reaches, per flag word -- printed once on the MI355X
# (per layer of that list: flags 0 -> 5 5 5 5 5 0 0 2 4 2 1; AP_CONV_SPLIT and AP_CONV_SPLIT_F16 -> 5 5 5 5 5 3 3 3 4 3 3; the
# list below, per layer: flags 0 -> 5 5 5 2 2 2 5 2 1 1 5 0 0 4; the split flags -> 5 5 5 3 3 3 5 3 3 3 5 3 3 4)
SQUARE_CLASSES = {0: {0, 1, 2, 4, 5}, 0x100: {3, 4, 5}, 0x400: {3, 4, 5}}
_conv_refs = {}


def _off_square_case(case):
    """Inputs and the float64 reference of one layer, computed once and shared by the three flag words."""
    if case not in _conv_refs:
        B, Cin, H, W, Cout, k, s, p, g, has_b, has_r, relu = case
        x = _u(f"os/x{Cin}{H}{W}", (B, Cin, H, W), 1)
        w = _u(f"os/w{Cin}{Cout}{k}", (Cout, Cin // g, k, k), 1)
        b = _u(f"os/b{Cout}", (Cout,), 1) if has_b else None
        ref = F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride=s, padding=p, groups=g)
        r = _u(f"os/r{Cout}{H}{W}", tuple(ref.shape), 2) if has_r else None
        if r is not None:
            ref = ref + r.double()
        if relu:
            ref = F.relu(ref)
        _conv_refs[case] = (x, w, b, r, ref.float())
    return _conv_refs[case]


def _conv_class(lib):
    ms, fl, n = (C.c_double * 8)(), (C.c_double * 8)(), (C.c_int64 * 8)()
    N.check(lib.ap_conv_profile_read(ms, fl, n, 8))
    assert sum(n) == 1, list(n)
    return list(n).index(1)


@pytest.mark.parametrize("flags", [0, 0x100, 0x400])
def test_conv2d_primitive_off_the_square(dev, flags):
    """ap_conv2d_fwd with H != W against float64 conv2d (bias / residual / ReLU mixed over the cases), output between guard bands,
    the kernel class of every launch read from ap_conv_profile_read: together the cases reach every class the square list reaches."""
    lib = N.lib()
    reached = set()
    N.use_conv_workspace(dev)
    for case in OFF_SQUARE:
        B, Cin, H, W, Cout, k, s, p, g, has_b, has_r, relu = case
        x, w, b, r, ref = _off_square_case(case)
        xd, wd = x.to(dev), w.to(dev)
        bd, rd = (None if b is None else b.to(dev)), (None if r is None else r.to(dev))
        wT = torch.empty(lib.ap_conv2d_packed_elems(Cout, Cin // g, k, k, g), device=dev)
        N.check(lib.ap_conv2d_pack(N.ptr(wd), None, N.ptr(wT), Cout, Cin // g, k, k, g, N.stream()))
        _, out, ok = _guarded(tuple(ref.shape), dev)
        N.check(lib.ap_conv_profile_enable(1))
        try:
            N.check(lib.ap_conv2d_fwd(N.ptr(xd), N.ptr(wT), N.ptr(bd), N.ptr(rd), N.ptr(out), B, Cin, H, W, Cout, k, k, s, p, g,
                                      relu | flags, Cin, 0, N.stream()))
            cls = _conv_class(lib)
        finally:
            N.check(lib.ap_conv_profile_enable(0))
        reached.add(cls)
        e = rel_err(out.cpu().numpy(), ref.numpy())
        print(f"flags {flags:#x} {case[:9]}: class {cls}, {e:.2e}")
        assert e < CONV_TOL, (case, cls, e)
        ok()
    print(f"flags {flags:#x}: classes reached off the square {sorted(reached)}")
    assert reached >= SQUARE_CLASSES[flags], (sorted(reached), sorted(SQUARE_CLASSES[flags]))
