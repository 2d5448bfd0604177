"""float64 restatement of a TRAIN plan of audiopure_amd.convnet with live dropout (``lower(module, chw, train=True, dropout=True)``):
the plan walker of convnet_train_restate.py with the ``drop`` kind, on the masks of ``ap_dropout``'s documented rule
(unet_train_restate.dropout_mask: Philox4x32-10 over (element // 4, draw, sample), kept iff u >= p, scale fp32(1 / (1 - p))).  Test
infrastructure only: test_convnet_dropout_cpu.py pins it to each module's own float32 step with ``F.dropout`` patched to the same mask
and to the reference's own VGG and WideResNet(dropRate=0.3) classes patched likewise (tests/golden/golden_convnet_dropout_v1.npz), and
asserts the conditions the bounds rest on; test_gpu_convnet_dropout.py pins ``NativeConvNet.set_dropout`` to it.

    python tests/convnet_dropout_restate.py        # find the seeds, re-measure the float32 errors (CPU, about a minute)

Bounds (measured as in 3.12): 4 x the error of the patched float32 torch step on the CPU against this restatement, per
quantity as max |d| / max |ref| per tensor, maximised over tensors, steps and cases; gradients AT THE IMPLEMENTATION'S ReLU DECISIONS
(convnet_train_restate.py explains why):
    forward (logits, loss, running statistics after one and two steps)   FWD_F32_ERR    vgg 5.1e-6 (its last stage normalises B = 4 values per channel), wideresnetD 1.6e-7
    gradients (every parameter; dx)                                      GRAD_F32_ERR   vgg 1.3e-5 (the same last stage), wideresnetD 1.1e-6
"""
import copy
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnet_train_restate as R  # noqa: E402
from unet_train_restate import dropout_mask  # noqa: E402
import synth_convnets as S  # noqa: E402
from audiopure_amd import synth  # noqa: E402
from audiopure_amd.convnet import lower  # noqa: E402

B, CHW, NUM_CLASSES = 4, (1, 32, 32), 10
DROP_SEED, SAMPLE_OFFSET = 0x9E3779B97F4A7C15, 7     # the fixed stream of the tests: set_dropout(("philox", DROP_SEED, SAMPLE_OFFSET))
CASES = {
    "vgg": lambda: S.vgg19_bn(NUM_CLASSES, 1, width_div=8),                                       # nn.Dropout() twice, p = 0.5
    "wideresnetD": lambda: S.WideResNet28_10(NUM_CLASSES, 1, depth=10, widen=1, drop_rate=0.3),   # F.dropout in each block
}
DROPS = {"vgg": [0.5, 0.5], "wideresnetD": [0.3, 0.3, 0.3]}      # p per drop step in execution order (depth 10: one block per stack)
# seeds of weights and input per case: the first of 0, 1, ... at which the float64 restatement alone meets the conditions of
# convnet_train_restate.py (undecided share, max-pool gap, variance over eps), with this file's FWD_BOUND
SEED = {"vgg": 0, "wideresnetD": 0}

FWD_F32_ERR = 5.2e-6
GRAD_F32_ERR = 1.3e-5
FWD_BOUND = 4 * FWD_F32_ERR
GRAD_BOUND = 4 * GRAD_F32_ERR
MAX_UNDECIDED = R.MAX_UNDECIDED


class patched_dropout:
    """``torch.nn.functional.dropout`` (nn.Dropout calls it too) on ap_dropout's masks: the k-th live call of a forward multiplies by
    dropout_mask(seed, k, sample_offset, ...) in its input's dtype."""

    def __init__(self, seed=DROP_SEED, offset=SAMPLE_OFFSET):
        self.seed, self.offset = seed, offset

    def __enter__(self):
        self.orig, self.k = F.dropout, 0

        def dropout(input, p=0.5, training=True, inplace=False):
            if not training or p == 0:
                return input
            m = mask(self.seed, self.k, self.offset, input.shape[0], input[0].numel(), p).reshape(input.shape)
            self.k += 1
            return input * m.to(input.dtype)
        torch.nn.functional.dropout = dropout
        return self

    def __exit__(self, *exc):
        torch.nn.functional.dropout = self.orig


@functools.lru_cache(maxsize=None)
def mask(seed, draw, offset, b, n, p):
    return torch.from_numpy(dropout_mask(seed, draw, offset, b, n, p))


def inputs(name, seed=None):
    seed = SEED[name] if seed is None else seed
    x = torch.from_numpy(synth.uniform("cnd/x/" + name, (B,) + CHW, seed, -2.0, 2.0))
    return x, torch.arange(B) % NUM_CLASSES


def build(name, seed=None):
    seed = SEED[name] if seed is None else seed
    m = R.init(CASES[name](), seed)
    x, y = inputs(name, seed)
    return m, lower(m, CHW, train=True, dropout=True), x, y


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (the module in train() mode with seeded float32 weights, its train plan with drop steps, x, labels).  Shared: do not modify."""
    return build(name)


def run_plan(plan, st, x, info=None, flips=None, seed=DROP_SEED, offset=SAMPLE_OFFSET):
    """convnet_train_restate.run_plan with the ``drop`` kind (and this file's FWD_BOUND as the undecided threshold)."""
    pieces = {plan.input.buf: {0: x}}
    new_running = {}
    n_relu = n_undecided = n_forced_decided = 0
    masks = []
    min_var, min_gap = float("inf"), float("inf")

    def read(v):
        ps = pieces[v.buf]
        t = ps[0] if len(ps) == 1 and 0 in ps else torch.cat([ps[k] for k in sorted(ps)], 1)
        assert t.shape[1] == v.cstride, "a buffer read before every slice of it was written"
        return t[:, v.coff:v.coff + v.C]

    def relu(t):
        nonlocal n_relu, n_undecided, n_forced_decided
        own = t.detach() > 0
        a = t.detach().abs()
        tau = FWD_BOUND * float(a.max())
        n_relu += t.numel()
        n_undecided += int(((a > 0) & (a < tau)).sum())
        number = len(masks)
        masks.append(own)
        if flips and number in flips:
            idx = flips[number]
            m = own.clone().reshape(-1)
            m[idx] = ~m[idx]
            n_forced_decided += int((a.reshape(-1)[idx] >= tau).sum())
            return t * m.reshape(t.shape)
        return F.relu(t)

    for s in plan.steps:
        p, o = s.p, s.out
        if s.kind == "conv":
            w = st[p["wname"]].reshape(p["wshape"])
            r = F.conv2d(read(s.ins[0]), w, None if p["bname"] is None else st[p["bname"]], p["stride"], p["pad"], 1, p["groups"])
            if p["res"] is not None:
                r = r + read(p["res"])
            assert not p["relu"]
        elif s.kind == "bn":
            xin = read(s.ins[0])
            n = xin.shape[0] * xin.shape[2] * xin.shape[3]
            mu = xin.mean((0, 2, 3))
            var = ((xin - mu[None, :, None, None]) ** 2).mean((0, 2, 3))
            r = (xin - mu[None, :, None, None]) / torch.sqrt(var + p["eps"])[None, :, None, None]
            r = r * st[p["wname"]][None, :, None, None] + st[p["bname"]][None, :, None, None]
            mom = p["momentum"] if p["momentum"] is not None else 1.0 / (int(st[p["nbtname"]]) + 1)
            new_running[p["rmname"]] = ((1 - mom) * st[p["rmname"]] + mom * mu).detach()
            new_running[p["rvname"]] = ((1 - mom) * st[p["rvname"]] + mom * var * (n / (n - 1))).detach()
            new_running[p["nbtname"]] = st[p["nbtname"]] + 1
            min_var = min(min_var, float(var.detach().min()) / p["eps"])
            if p["relu"]:
                r = relu(r)
        elif s.kind == "drop":
            xin = read(s.ins[0])
            assert s.ins[0].full and o.full
            r = xin * mask(seed, p["draw"], offset, xin.shape[0], xin[0].numel(), p["p"]).reshape(xin.shape).to(xin.dtype)
        elif s.kind == "affine":
            assert p["sk"] is None
            r = read(s.ins[0])
            if p["relu"]:
                r = relu(r)
        elif s.kind == "add":
            r = read(s.ins[0]) + read(s.ins[1])
            if p["relu"]:
                r = relu(r)
        elif s.kind == "copy":
            r = read(s.ins[0])
        elif s.kind == "pool":
            xin = read(s.ins[0])
            if p["is_max"]:
                r = F.max_pool2d(xin, p["k"], p["stride"], p["pad"])
                win = F.unfold(F.pad(xin.detach(), (p["pad"],) * 4, value=float("-inf")), p["k"], stride=p["stride"])
                top = win.reshape(xin.shape[0], xin.shape[1], p["k"] ** 2, -1).topk(2, dim=2).values
                live = top[:, :, 0] > 0
                min_gap = min(min_gap, float((top[:, :, 0] - top[:, :, 1])[live].min()) / float(xin.detach().abs().max()))
            else:
                r = F.avg_pool2d(xin, p["k"], p["stride"], p["pad"])
        else:
            raise AssertionError(s.kind)
        pieces.setdefault(o.buf, {})[o.coff] = r
    out = read(plan.output)
    if info is not None:
        info.update(relu_inputs=n_relu, undecided=n_undecided, min_var_over_eps=min_var, min_pool_gap=min_gap, masks=masks,
                    forced_decided=n_forced_decided)
    return (out.flatten(1) if plan.output.H == 1 and plan.output.W == 1 else out), new_running


def train_step(plan, st, x, y, info=None, flips=None):
    """convnet_train_restate.train_step on this file's walker"""
    leaves = {k: v.clone().requires_grad_(True) for k, v in st.items() if v.is_floating_point() and "running_" not in k}
    xs = x.clone().requires_grad_(True)
    full = dict(st)
    full.update(leaves)
    logits, running = run_plan(plan, full, xs, info, flips)
    loss = F.cross_entropy(logits, y)
    names = list(leaves)
    gs = torch.autograd.grad(loss, [xs] + [leaves[k] for k in names], allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(names, gs[1:])}
    return dict(logits=logits.detach().to(x.dtype), loss=loss.detach(), running=running, grads=grads, dx=gs[0])


def module_step(m, x, y):
    """The module's own .train() step with F.dropout patched to the restatement's masks (its buffers move)."""
    with patched_dropout():
        return R.module_step(m, x, y)


def module_masks(m, x):
    """The ReLU decisions of the module's own patched train-mode forward on x, in execution order; on a copy."""
    from audiopure_amd.convnet import _Tape, _opname
    tape = _Tape()
    with torch.no_grad(), patched_dropout(), tape:
        copy.deepcopy(m).train()(x)
    return [out > 0 for func, _, _, out in tape.entries if _opname(func) in ("relu", "relu_")]


def _two_steps(m, plan, x, y, flips=None):
    st = R.state(m, torch.float64)
    info = {}
    s1 = train_step(plan, st, x.double(), y, info, flips)
    st2 = dict(st)
    st2.update(s1["running"])
    s2 = train_step(plan, st2, x.double(), y, None, flips)
    return s1, s2, info


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 restatement of two consecutive steps at fixed parameters -> (step 1, step 2, info of step 1).  Shared: never modified."""
    m, plan, x, y = case(name)
    return _two_steps(m, plan, x, y)


def flips_of(name, masks):
    own = reference(name)[2]["masks"]
    assert len(own) == len(masks) and all(a.numel() == b.numel() for a, b in zip(own, masks))     # (a ReLU behind a Linear: [B, n] or [B, n, 1, 1])
    out = []
    for i, (a, b) in enumerate(zip(own, masks)):
        idx = (a.reshape(-1) != b.cpu().reshape(-1)).nonzero().reshape(-1)
        if idx.numel():
            out.append((i, tuple(idx.tolist())))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference_at(name, flips=()):
    """The restatement at an implementation's ReLU decisions (convnet_train_restate.reference_at) -> (step 1, step 2, flipped inputs
    that were NOT within the forward bound of 0: asserted 0 by the callers)."""
    if not flips:
        return reference(name)[0], reference(name)[1], 0
    m, plan, x, y = case(name)
    s1, s2, info = _two_steps(m, plan, x, y, {i: torch.tensor(idx, dtype=torch.long) for i, idx in flips})
    return s1, s2, info["forced_decided"]


def conditions_met(info):
    return (info["undecided"] <= MAX_UNDECIDED * info["relu_inputs"] and info["min_pool_gap"] >= FWD_BOUND and info["min_var_over_eps"] > 1.0)


def find_seed(name):
    for seed in range(16):
        m, plan, x, y = build(name, seed)
        info = {}
        with torch.no_grad():
            run_plan(plan, R.state(m, torch.float64), x.double(), info)
        if conditions_met(info):
            return seed
    raise AssertionError(name)


def measure_f32(name):
    """the patched float32 torch step (two steps on the CPU) against the restatement -> (forward error, gradient error)"""
    m, plan, x, y = case(name)
    m32 = copy.deepcopy(m)
    r1, r2, decided = reference_at(name, flips_of(name, module_masks(m32, x)))
    assert decided == 0, "float32 torch decided a ReLU input that is not within the forward bound of 0 the other way"
    g1 = module_step(m32, x, y)
    g2 = module_step(m32, x, y)
    (f1, d1), (f2, d2) = compare(g1, r1, plan), compare(g2, r2, plan)
    return max(f1, f2), max(d1, d2)


def bias_scales(plan, grads):
    """A conv bias in front of a BatchNorm (every conv of the VGG's features) has a gradient that is zero but for rounding -- in
    float64 too, 1e-17 of its layer's: its error is scaled by its layer's max |dW|, always (convnet_train_restate.bias_scales does
    so where the reference is an exact zero)."""
    bn_in = {s.ins[0].buf for s in plan.steps if s.kind == "bn"}
    return {s.p["bname"]: float(grads[s.p["wname"]].abs().max()) for s in plan.steps
            if s.kind == "conv" and s.p["bname"] is not None and s.out.buf in bn_in}


def compare(got, ref, plan):
    """-> (forward error, gradient error) of one step's dict against `ref`: the largest per-tensor figure of each class"""
    fwd = max([R.rel(got["logits"], ref["logits"]), R.rel(got["loss"], ref["loss"])] +
              [R.rel(got["running"][k], ref["running"][k]) for k in ref["running"] if "running_" in k])
    scales = bias_scales(plan, ref["grads"])
    grad = max([R.rel(got["grads"][k], ref["grads"][k], scales.get(k)) for k in ref["grads"]] + [R.rel(got["dx"], ref["dx"])])
    return fwd, grad


GOLDEN_FULL = R.GOLDEN_FULL


def golden_pick(name, key, n):
    return np.minimum((synth.uniform(f"cnd/pick/{name}/{key}", (64,), 0, 0.0, 1.0).astype(np.float64) * n).astype(np.int64), n - 1)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(R.ROOT, "tests", "golden", "golden_convnet_dropout_v1.npz")))


def golden_flips(name):
    G = golden()
    return tuple((int(k.rsplit("/", 1)[1]), tuple(int(i) for i in G[k])) for k in sorted(G) if k.startswith(f"{name}/flips/"))


def compare_golden(got, name, step, plan, ref, ref_golden=None):
    """convnet_train_restate.compare_golden against this file's golden and picks"""
    G, pre = golden(), f"{name}/{step}/"
    ref_golden = ref if ref_golden is None else ref_golden
    fwd = max([R.rel(got["logits"], torch.from_numpy(G[pre + "logits"])), R.rel(got["loss"], torch.from_numpy(G[pre + "loss"]))] +
              [R.rel(got["running"][k], torch.from_numpy(G[pre + "running/" + k])) for k in got["running"] if "running_" in k])
    scales = bias_scales(plan, ref["grads"])
    grad, pre = 0.0, f"{name}/1/"
    for k, g in list(got["grads"].items()) + [("dx", got["dx"])]:
        g = g.detach().double().cpu().reshape(-1)
        r = (ref["dx"] if k == "dx" else ref["grads"][k]).double().reshape(-1)
        rg = (ref_golden["dx"] if k == "dx" else ref_golden["grads"][k]).double().reshape(-1)
        scale = scales.get(k) or float(r.abs().max())
        if pre + "grad/" + k in G:
            grad = max(grad, float((g - torch.from_numpy(G[pre + "grad/" + k]).double() - (r - rg)).abs().max()) / scale)
        else:
            pick = torch.from_numpy(golden_pick(name, k, g.numel()))
            grad = max(grad, float((g[pick] - torch.from_numpy(G[pre + "gradpick/" + k]).double() - (r - rg)[pick]).abs().max()) / scale,
                       abs(float(g.norm()) - float(G[pre + "gradnorm/" + k]) - (float(r.norm()) - float(rg.norm()))) / float(r.norm()))
    return fwd, grad


if __name__ == "__main__":
    worst_f = worst_g = 0.0
    for name in CASES:
        print(f"{name}: first seed that meets the conditions: {find_seed(name)} (recorded {SEED[name]})")
        f, g = measure_f32(name)
        info = reference(name)[2]
        print("    float32 torch decides differently:", flips_of(name, module_masks(case(name)[0], case(name)[2])))
        worst_f, worst_g = max(worst_f, f), max(worst_g, g)
        print(f"{name:11s} seed {SEED[name]}  fwd {f:.2e}  grad {g:.2e}  undecided {info['undecided']} / {info['relu_inputs']} = "
              f"{info['undecided'] / info['relu_inputs']:.2e}  min var / eps {info['min_var_over_eps']:.3g}  min pool gap {info['min_pool_gap']:.3g}")
    print(f"FWD_F32_ERR {worst_f:.2e} (recorded {FWD_F32_ERR:.2e})   GRAD_F32_ERR {worst_g:.2e} (recorded {GRAD_F32_ERR:.2e})")
