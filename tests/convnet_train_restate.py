"""float64 restatement, in plain torch functionals, of a TRAIN plan of audiopure_amd.convnet (``lower(module, chw, train=True)``):
conv / BatchNorm on batch statistics / ReLU / add / cat / slice / pooling / linear, the running statistics as nn.BatchNorm2d updates
them, gradients by torch autograd.  Every function works in the dtype it is given: the float64 call is the reference, the module's
own float32 forward and backward measure what float32 arithmetic alone costs.  Test infrastructure only:
test_convnet_train_cpu.py pins it to the modules' own train step and to the reference's numbers
(tests/golden/golden_convnet_train_v1.npz), and asserts the conditions the GPU bounds rest on; the GPU tests pin the kernels of
ap_convnet_train.hip to it.

    python tests/convnet_train_restate.py        # re-measure the float32 errors of every case (CPU, under a minute)
"""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import synth_convnets as S  # noqa: E402
from audiopure_amd import synth  # noqa: E402
from audiopure_amd.convnet import lower  # noqa: E402

B, CHW, NUM_CLASSES = 4, (1, 32, 32), 10


class _SmallDPN(S.DPN92):
    """two blocks in the first stage, one in each of the others: (mid, res, blocks, dense) per stage; the 3 x 3 has 32 groups"""
    TABLE = ((32, 64, 2, 8), (32, 128, 1, 8), (64, 256, 1, 8), (64, 512, 1, 8))


# the five dropout-free families as small instances of the block classes of tools/synth_convnets.py; the same constructor arguments
# build the reference's own classes in tests/golden/make_golden_convnet_train.py
CASES = {
    "resnext": lambda: S.CifarResNeXt(NUM_CLASSES, cardinality=2, depth=11, base_width=16, widen_factor=1, in_channels=1),   # group widths 16, 32, 64
    "resnet": lambda: S.ResNet50(NUM_CLASSES, 1, reps=(1, 1, 1, 1)),                     # 7 x 7 / 2 stem, 3 x 3 / 2 max pool, bottlenecks
    "wideresnet": lambda: S.WideResNet28_10(NUM_CLASSES, 1, depth=10, widen=1),          # pre-activation, 1 x 1 projection of the activated input
    "dpn": lambda: _SmallDPN(NUM_CLASSES, 1),                                            # dual path: slices, add, cat
    "densenet": lambda: S.DenseNetBC100(NUM_CLASSES, 1, depth=10, growth=12),            # dense bottleneck, transition with average pool
}
# seeds of weights and input per case: the first of 0, 1, ... at which the float64 restatement alone meets the conditions below
# (resnet: seeds 0, 1, 2 leave a max-pool window whose two largest values are 7.1e-6, 3.6e-6, 9.3e-6 of the tensor's maximum apart)
SEED = {"resnext": 0, "resnet": 3, "wideresnet": 0, "dpn": 0, "densenet": 0}

# ---- bounds: 4 x the error of float32 torch (the module's own .train() step on the CPU) against this float64
# restatement, per quantity as max |d| / max |ref| per tensor, maximised over tensors and cases.  Measured by this file's __main__ and
# re-measured by test_convnet_train_cpu.py:
#   forward (logits, loss, running statistics after one and two steps)   FWD_F32_ERR
#       resnext 2.1e-7, resnet 4.6e-6 (its last stage normalises B = 4 values per channel), wideresnet 1.9e-7, dpn 9.0e-7, densenet 3.6e-7
#   gradients (every parameter; dx)                                      GRAD_F32_ERR
#       resnext 1.3e-6, resnet 3.1e-5 (the same last stage), wideresnet 1.1e-6, dpn 5.6e-6, densenet 2.0e-6
# Gradients are compared AT THE IMPLEMENTATION'S ReLU DECISIONS (`reference_at`).  Of a case's 0.3 - 2 M ReLU inputs, 20 to 200 lie
# within the forward bound of 0 (the `undecided` count below); float32 torch on the CPU decides one of them the other way than float64
# on the resnext case and one on the dpn case, and a single such input moves its channel's d beta by 2 % (resnext,
# stage_2.stage_2_bottleneck_0.bn_reduce.bias, channel 43; 2.9e-2 of the tensor's maximum) and everything upstream with it.  No float32
# arithmetic can be held to a decision on such an input, so the float64 reference takes those decisions -- and only those: a flipped
# input that is NOT within the forward bound of 0 fails the comparison -- from the implementation under test, and what is left is
# rounding.
FWD_F32_ERR = 4.7e-6
GRAD_F32_ERR = 3.2e-5
FWD_BOUND = 4 * FWD_F32_ERR
GRAD_BOUND = 4 * GRAD_F32_ERR
# conditions on the cases: a nonzero ReLU input closer to 0 than the forward bound (times the tensor's largest magnitude) is undecided
# in float32 -- at most this fraction of a case's ReLU inputs; no max-pool window with a positive maximum whose two largest values are
# closer than that; every BatchNorm channel's batch variance above eps
MAX_UNDECIDED = 1e-3


def init(model, seed):
    """synth.synth_init, then the sign of every fifth BatchNorm gamma flipped: a ReLU mask decided before the affine is wrong there
    (a gamma of exactly 0 makes a channel constant and the next layer's statistics degenerate: test_gpu_bn2d_train.py has that case).
    Returns the model in train() mode."""
    synth.synth_init(model, seed)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight[::5] *= -1.0
    return model.train()


def inputs(name):
    x = torch.from_numpy(synth.uniform("cnt/x/" + name, (B,) + CHW, SEED[name], -2.0, 2.0))
    return x, torch.arange(B) % NUM_CLASSES


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (the module in train() mode with seeded float32 weights, its train plan, x, labels).  Shared by the tests: do not modify."""
    m = init(CASES[name](), SEED[name])
    x, y = inputs(name)
    return m, lower(m, CHW, train=True), x, y


def state(m, dtype):
    """the module's parameters and buffers by state-dict key, floating tensors in `dtype` (detached copies)"""
    return {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.detach().clone()) for k, v in m.state_dict().items()}


def run_plan(plan, st, x, info=None, flips=None):
    """Execute a train plan on the tensors of `st` (by name) in x's dtype -> (output, {running statistic name: new value}).
    Differentiable by autograd with respect to x and every tensor of `st`.  `info`: a dict that receives the conditions' figures and
    every ReLU's own decisions (`masks`, in plan order).  `flips` {ReLU number: flat indices}: those inputs are decided the OTHER way
    than this arithmetic decides them (an implementation's decisions on undecided inputs, see `reference_at`); `info["forced_decided"]`
    counts the flipped inputs that are NOT within the forward bound of 0."""
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
        if info is not None:
            n_relu += t.numel()                          # (an exact 0 is a value an earlier ReLU shut: 0 in every precision, decided)
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
                if info is not None:
                    win = F.unfold(F.pad(xin.detach(), (p["pad"],) * 4, value=float("-inf")), p["k"], stride=p["stride"])
                    top = win.reshape(xin.shape[0], xin.shape[1], p["k"] ** 2, -1).topk(2, dim=2).values
                    live = top[:, :, 0] > 0                  # (a tie at 0 behind a ReLU passes no gradient whichever element wins)
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
    """One step of train_speech_commands.py:131-140 without the optimizer: -> dict(logits, loss, running, grads {name: d loss / d
    parameter}, dx), everything in st's dtype.  `st` is not modified."""
    dtype = x.dtype
    leaves = {k: v.clone().requires_grad_(True) for k, v in st.items() if v.is_floating_point() and "running_" not in k}
    xs = x.clone().requires_grad_(True)
    full = dict(st)
    full.update(leaves)
    logits, running = run_plan(plan, full, xs, info, flips)
    loss = F.cross_entropy(logits, y)
    names = list(leaves)
    gs = torch.autograd.grad(loss, [xs] + [leaves[k] for k in names], allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(names, gs[1:])}
    return dict(logits=logits.detach().to(dtype), loss=loss.detach(), running=running, grads=grads, dx=gs[0])


def module_step(m, x, y):
    """The module's own .train() step in its own dtype (its buffers move): the same dict as train_step."""
    xs = x.clone().requires_grad_(True)
    for q in m.parameters():
        q.grad = None
    logits = m(xs)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    sd = m.state_dict()
    running = {k: sd[k].detach().clone() for k in sd if "running_" in k or k.endswith("num_batches_tracked")}
    grads = {k: (q.grad.detach().clone() if q.grad is not None else torch.zeros_like(q)) for k, q in m.named_parameters()}
    return dict(logits=logits.detach(), loss=loss.detach(), running=running, grads=grads, dx=xs.grad.detach())


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 restatement of two consecutive steps at fixed parameters (the second from the first's running statistics):
    -> (step 1, step 2, info of step 1).  Computed once, shared by the tests, never modified."""
    import copy
    m, plan, x, y = case(name)
    st = state(m, torch.float64)
    info = {}
    s1 = train_step(plan, st, x.double(), y, info)
    st2 = dict(st)
    st2.update(s1["running"])
    s2 = train_step(plan, st2, x.double(), y)
    return s1, s2, info


def module_masks(m, x):
    """The ReLU decisions (output > 0) of the module's own train-mode forward on x, in the order the ReLUs run -- which is the order of
    the plan's ReLU-carrying steps (test_convnet_train_cpu.py: the float64 module's decisions ARE the restatement's).  On a copy: the
    module's buffers do not move."""
    import copy
    from audiopure_amd.convnet import _Tape, _opname
    tape = _Tape()
    with torch.no_grad(), tape:
        copy.deepcopy(m).train()(x)
    return [out > 0 for func, _, _, out in tape.entries if _opname(func) in ("relu", "relu_")]


def masks_from_bufs(plan, bufs):
    """The ReLU decisions of an executor that kept every buffer of the plan ({buf id: [B, C, H, W]}): output > 0, in plan order."""
    return [bufs[s.out.buf] > 0 for s in plan.steps if s.p.get("relu")]


def flips_of(name, masks):
    """Where an implementation's ReLU decisions differ from the float64 restatement's own: a hashable ((ReLU number, (flat indices)), ...)"""
    own = reference(name)[2]["masks"]
    assert len(own) == len(masks) and all(a.shape == b.shape for a, b in zip(own, masks))
    out = []
    for i, (a, b) in enumerate(zip(own, masks)):
        idx = (a.reshape(-1) != b.cpu().reshape(-1)).nonzero().reshape(-1)
        if idx.numel():
            out.append((i, tuple(idx.tolist())))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference_at(name, flips=()):
    """The float64 restatement at an implementation's ReLU decisions: `reference(name)` with the inputs named by `flips` decided the
    other way.  A ReLU input within the float32 error of 0 has no decision that float32 arithmetic can be held to (its gradient
    contribution switches on or off as a whole, moving a channel's d beta by percents), so those decisions are taken from the
    implementation under test and everything else is compared at rounding level -- the undecided inputs are set aside, as M5's clip
    seeds do.  Every flipped input must BE undecided: -> (step 1, step 2, flipped inputs that were decided), the
    last asserted 0 by the callers."""
    if not flips:
        return reference(name)[0], reference(name)[1], 0
    m, plan, x, y = case(name)
    fl = {i: torch.tensor(idx, dtype=torch.long) for i, idx in flips}
    st = state(m, torch.float64)
    info = {}
    s1 = train_step(plan, st, x.double(), y, info, fl)
    st2 = dict(st)
    st2.update(s1["running"])
    s2 = train_step(plan, st2, x.double(), y, None, fl)
    return s1, s2, info["forced_decided"]


GOLDEN_FULL = 4096                                   # the golden holds gradients up to this many elements in full


def golden_pick(name, key, n):
    """the 64 seeded element indices of a larger gradient tensor that the golden holds (beside its L2 norm)"""
    return np.minimum((synth.uniform(f"cnt/pick/{name}/{key}", (64,), 0, 0.0, 1.0).astype(np.float64) * n).astype(np.int64), n - 1)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_convnet_train_v1.npz")))


def golden_flips(name):
    """the ReLU decisions of the run that wrote the golden, as `flips_of` gives them (stored by make_golden_convnet_train.py)"""
    G = golden()
    return tuple((int(k.rsplit("/", 1)[1]), tuple(int(i) for i in G[k])) for k in sorted(G) if k.startswith(f"{name}/flips/"))


def compare_golden(got, name, step, plan, ref, ref_golden=None):
    """-> (forward error, gradient error) of one step's dict against the reference's own numbers in the golden, measured like
    ``compare`` (the scale of a picked element or of a norm is the float64 restatement's max |gradient| resp. norm).  `ref`: the
    restatement at got's ReLU decisions; `ref_golden`: at the golden's, where they differ -- the difference of the two restatements
    is then taken out of got - golden, so that what is measured is rounding, not which way an undecided input went."""
    G, pre = golden(), f"{name}/{step}/"
    ref_golden = ref if ref_golden is None else ref_golden
    fwd = max([rel(got["logits"], torch.from_numpy(G[pre + "logits"])), rel(got["loss"], torch.from_numpy(G[pre + "loss"]))] +
              [rel(got["running"][k], torch.from_numpy(G[pre + "running/" + k])) for k in got["running"] if "running_" in k])
    scales = bias_scales(plan, ref["grads"])
    grad, pre = 0.0, f"{name}/1/"                    # gradients: the first step's (at fixed parameters the second's are the same)
    for k, g in list(got["grads"].items()) + [("dx", got["dx"])]:
        g = g.detach().double().cpu().reshape(-1)
        r = (ref["dx"] if k == "dx" else ref["grads"][k]).double().reshape(-1)
        rg = (ref_golden["dx"] if k == "dx" else ref_golden["grads"][k]).double().reshape(-1)
        scale = float(r.abs().max()) or scales.get(k, 1.0)
        if pre + "grad/" + k in G:
            grad = max(grad, float((g - torch.from_numpy(G[pre + "grad/" + k]).double() - (r - rg)).abs().max()) / scale)
        else:
            pick = torch.from_numpy(golden_pick(name, k, g.numel()))
            grad = max(grad, float((g[pick] - torch.from_numpy(G[pre + "gradpick/" + k]).double() - (r - rg)[pick]).abs().max()) / scale,
                       abs(float(g.norm()) - float(G[pre + "gradnorm/" + k]) - (float(r.norm()) - float(rg.norm()))) / float(r.norm()))
    return fwd, grad


def rel(a, ref, scale=None):
    """max |a - ref| / max |ref| (or / `scale`), in float64"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    d = float((a - ref).abs().max())
    s = float(ref.abs().max()) if scale is None else float(scale)
    return d / s if s > 0 else d


def bias_scales(plan, grads):
    """A conv bias in front of a BatchNorm has an exact-zero gradient: its error is scaled by its layer's max |dW| (as for M5)."""
    return {s.p["bname"]: float(grads[s.p["wname"]].abs().max()) for s in plan.steps if s.kind == "conv" and s.p["bname"] is not None}


def compare(got, ref, plan):
    """-> (forward error, gradient error) of one step's dict `got` against `ref`: the largest per-tensor figure of each class"""
    fwd = max([rel(got["logits"], ref["logits"]), rel(got["loss"], ref["loss"])] +
              [rel(got["running"][k], ref["running"][k]) for k in ref["running"] if "running_" in k])
    scales = bias_scales(plan, ref["grads"])
    grad = max([rel(got["grads"][k], ref["grads"][k], scales.get(k) if float(ref["grads"][k].abs().max()) == 0.0 else None)
                for k in ref["grads"]] + [rel(got["dx"], ref["dx"])])
    return fwd, grad


def measure_f32(name):
    """float32 torch (the module's own two steps on the CPU) against the float64 restatement -> (forward error, gradient error)"""
    import copy
    m, plan, x, y = case(name)
    m32 = copy.deepcopy(m)
    r1, r2, decided = reference_at(name, flips_of(name, module_masks(m32, x)))
    assert decided == 0, "float32 torch decided a ReLU input that is not within the forward bound of 0 the other way"
    g1 = module_step(m32, x, y)
    g2 = module_step(m32, x, y)
    (f1, d1), (f2, d2) = compare(g1, r1, plan), compare(g2, r2, plan)
    return max(f1, f2), max(d1, d2)


if __name__ == "__main__":
    worst_f = worst_g = 0.0
    for name in CASES:
        f, g = measure_f32(name)
        info = reference(name)[2]
        print("    float32 torch decides differently:", flips_of(name, module_masks(case(name)[0], case(name)[2])))
        worst_f, worst_g = max(worst_f, f), max(worst_g, g)
        print(f"{name:11s} seed {SEED[name]}  fwd {f:.2e}  grad {g:.2e}  undecided {info['undecided']} / {info['relu_inputs']} = "
              f"{info['undecided'] / info['relu_inputs']:.2e}  min var / eps {info['min_var_over_eps']:.3g}  min pool gap {info['min_pool_gap']:.3g}")
    print(f"FWD_F32_ERR {worst_f:.2e} (recorded {FWD_F32_ERR:.2e})   GRAD_F32_ERR {worst_g:.2e} (recorded {GRAD_F32_ERR:.2e})")
