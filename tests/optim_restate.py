"""float64 restatements of the optimizer updates (torch.optim's default single-tensor path: adam.py _single_tensor_adam, sgd.py
_single_tensor_sgd), of the reference's update_ema (improved_diffusion/nn.py:55-65) and of the squared gradient norm
(train_util.py:254-258), with seeded makers of parameter / gradient tables, and the bounds the native step (audiopure_amd/optim.py,
csrc/ap_optim.hip) is held to.

A table is a list of tensor sizes split into (at most) two param groups with their own lr and weight decay; three steps are run, the
lr of every group halves before the third (what a StepLR does).  In a table of three or more tensors, tensor 1 never gets a grad (its
`step` and state must not move; its EMA copies still do) and the last tensor -- in the second group, whose weight decay is 0 -- gets
all-zero gradients (its bits must not move).

Bounds: nothing is fixed in advance.  Each *_F32_ERR below is the distance of torch.optim's OWN float32 CPU run from the float64 run
on these same tables after three steps (measure_f32(), this file's __main__; re-measured by test_optim_restate_cpu.py), maximised
over the tables of `table_names()` and the kinds of KINDS, in these units:
    parameters, Adam and AdamW    max |p - ref| / lr                       (an Adam step is lr-sized whatever the gradient's scale)
    parameters, SGD               max |p - ref| / (lr max |buf_ref|)       (buf: the momentum buffer, or the effective gradient at mu = 0)
    state and EMA tensors         max |s - ref| / max |s_ref|              per tensor
and *_BOUND = 4 x that: the factor covers a different but equally valid fp32 evaluation order (contraction into fma, the form of the
lerp, a reciprocal square root).  (The kernel in fact pins torch.optim's own rounding sequence on the device and is compared with it
bit for bit by test_gpu_optim.py; these bounds hold it to the float64 truth independently of torch's device code.)
    measured (chunk 4096, slab 47):  ADAM 2.8e-4   SGD 1.5e-3   STATE 5.6e-6   EMA 2.6e-7
The SGD and state figures come from the smallest tensors: a one-element tensor whose momentum buffer nearly cancels (0.9 buf + g with g
of the other sign) has nothing larger to be measured against.
Input condition (check_condition, asserted on the CPU for the float64 and the float32 run): every effective gradient entry -- after
coupled decay -- is exactly 0 or at least 1e-6 = 100 eps in magnitude, so m / (sqrt(v) + eps) is well conditioned.

The squared norm's bound is derived, not measured: the kernel adds exact fp64 squares, relative error <= N 2^-53 for N terms, 1.2e-11
at N = 1e5; SQNORM_BOUND = 1e-10 for the test sizes (N <= 1e5).
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ADAM_F32_ERR = 2.8e-4
SGD_F32_ERR = 1.5e-3
STATE_F32_ERR = 5.7e-6
EMA_F32_ERR = 2.7e-7
ADAM_BOUND = 4 * ADAM_F32_ERR
SGD_BOUND = 4 * SGD_F32_ERR
STATE_BOUND = 4 * STATE_F32_ERR
EMA_BOUND = 4 * EMA_F32_ERR
SQNORM_BOUND = 1e-10
MIN_GRAD = 1e-6
STEPS = 3
EMA_RATES = (0.9999, 0.999, 0.99, 0.9)

# kind -> (torch class name, constructor arguments shared by the groups, the two groups' own lr / weight_decay)
KINDS = {
    "adam": ("Adam", {}, [dict(lr=1e-3, weight_decay=1e-2), dict(lr=3e-3, weight_decay=0.0)]),
    "adamw": ("AdamW", {}, [dict(lr=1e-3, weight_decay=5e-2), dict(lr=2e-3, weight_decay=0.0)]),
    "sgd": ("SGD", dict(momentum=0.9), [dict(lr=1e-2, weight_decay=1e-2), dict(lr=3e-2, weight_decay=0.0)]),
    "sgd0": ("SGD", dict(momentum=0.0), [dict(lr=1e-2, weight_decay=1e-2), dict(lr=3e-2, weight_decay=0.0)]),
}
SMALL = (1, 3, 4, 5, 7, 64, 129)


def chunk_and_slab():
    """(elements per workgroup, tensors per launch) of the built library: host-only calls, usable without a GPU"""
    from audiopure_amd import _native as N
    return N.lib().ap_optim_chunk(), N.lib().ap_optim_slab()


def table_names():
    return ["sizes", "n1", "S-1", "S", "S+1", "2S+1"]


def table_sizes(name, c, S):
    """tensor sizes of a table: every size at which the kernel takes another path, then every tensor count around the slab"""
    if name == "sizes":
        return [1, 3, 4, 5, c - 1, c, c + 1, 2 * c + 3]
    k = {"n1": 1, "S-1": S - 1, "S": S, "S+1": S + 1, "2S+1": 2 * S + 1}[name]
    return [2 * c + 3] if k == 1 else [SMALL[i % len(SMALL)] for i in range(k)]


class Table:
    """sizes, group split, initial parameters and the gradients of STEPS steps (float32 values held as float64 arrays)"""

    def __init__(self, name, c, S, seed=0):
        self.name = name
        self.sizes = table_sizes(name, c, S)
        n = len(self.sizes)
        self.split = n if n == 1 else (n + 1) // 2             # tensors [0, split) are group 0
        self.none = 1 if n >= 3 else -1
        self.zero = n - 1 if n >= 3 else -1
        rng = np.random.default_rng([seed, n, sum(self.sizes)])
        self.p0, self.grads = [], [[] for _ in range(STEPS)]
        for i, sz in enumerate(self.sizes):
            p = rng.uniform(0.1, 1.0, sz) * rng.choice([-1.0, 1.0], sz)
            self.p0.append(p.astype(np.float32).astype(np.float64))
            for s in range(STEPS):
                if i == self.none:
                    self.grads[s].append(None)
                    continue
                g = np.exp(rng.uniform(math.log(2e-2), math.log(2.0), sz)) * rng.choice([-1.0, 1.0], sz)
                g[rng.uniform(size=sz) < 0.05] = 0.0
                if i == self.zero:
                    g[:] = 0.0
                self.grads[s].append(g.astype(np.float32).astype(np.float64))

    def group_of(self, i):
        return 0 if i < self.split else 1

    def groups(self, kind):
        g = KINDS[kind][2]
        return g[:1] if self.split == len(self.sizes) else g


def lr_at(group, step):
    """a group's lr at step 0, 1, 2: halved before the third"""
    return group["lr"] * (0.5 if step >= 2 else 1.0)


# ---- float64 restatements --------------------------------------------------------------------------------------------------------
def adam_update(p, g, st, lr, betas, eps, wd, decoupled):
    """one Adam / AdamW step of one tensor, in place on float64 arrays; st: {"step", "exp_avg", "exp_avg_sq"}.  -> effective gradient"""
    b1, b2 = betas
    st["step"] += 1
    t = st["step"]
    if decoupled:
        p *= 1 - lr * wd
    elif wd != 0:
        g = g + wd * p
    m, v = st["exp_avg"], st["exp_avg_sq"]
    m += (g - m) * (1 - b1)
    v *= b2
    v += (1 - b2) * g * g
    step_size = lr / (1 - b1 ** t)
    denom = np.sqrt(v) / math.sqrt(1 - b2 ** t) + eps
    p -= step_size * (m / denom)
    return g


def sgd_update(p, g, st, lr, mu, wd):
    """one SGD step (dampening 0, no Nesterov) of one tensor, in place; st: {"momentum_buffer"} (None before the first step).
    -> effective gradient"""
    if wd != 0:
        g = g + wd * p
    eff = g
    if mu != 0:
        if st.get("momentum_buffer") is None:
            st["momentum_buffer"] = g.copy()
        else:
            st["momentum_buffer"] *= mu
            st["momentum_buffer"] += g
        g = st["momentum_buffer"]
    p -= lr * g
    return eff


def ema_update(targets, sources, rate):
    """update_ema (nn.py:55-65): targ = rate targ + (1 - rate) src, in place"""
    for t, s in zip(targets, sources):
        t *= rate
        t += (1 - rate) * s


GOLDEN_EMA_RATES = (None, 0.9999)                    # None: the reference's default (0.99); 0.9999: train_util.py's --ema_rate


def golden_ema_inputs():
    """inputs of tests/golden/golden_optim_v1.npz (fixed sizes, independent of the library's constants): -> (targets, per call the
    sources): eight small tensors; the sources drift from the targets by a gradient-sized step per call"""
    table = Table("S", 4096, 8)
    src = []
    for s in range(STEPS):
        src.append([p + 0.01 * (s + 1) * (g if g is not None else 0.0) for p, g in zip(table.p0, table.grads[s])])
    return [p.copy() for p in table.p0], src


def sqnorm(grads):
    return float(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads if g is not None))


def run_restate(kind, table, n_ema=0):
    """STEPS steps in float64 -> result dict (see run_torch) plus "eff": per step and tensor, the effective gradient (None without a grad)"""
    cls, common, _ = KINDS[kind]
    groups = table.groups(kind)
    P = [p.copy() for p in table.p0]
    states = [dict() for _ in P]
    emas = [[p.copy() for p in P] for _ in range(n_ema)]
    eff = [[None] * len(P) for _ in range(STEPS)]
    for s in range(STEPS):
        for i, p in enumerate(P):
            g = table.grads[s][i]
            if g is None:
                continue
            grp = groups[table.group_of(i)]
            lr = lr_at(grp, s)
            if cls == "SGD":
                eff[s][i] = sgd_update(p, g, states[i], lr, common["momentum"], grp["weight_decay"])
            else:
                if not states[i]:
                    states[i].update(step=0, exp_avg=np.zeros_like(p), exp_avg_sq=np.zeros_like(p))
                eff[s][i] = adam_update(p, g, states[i], lr, (0.9, 0.999), 1e-8, grp["weight_decay"], cls == "AdamW")
        for k in range(n_ema):
            ema_update(emas[k], P, EMA_RATES[k])
    return dict(params=P, states=states, emas=emas, eff=eff)


# ---- the same loop on an optimizer object (torch.optim on the CPU in either precision, or the native one on the GPU) ------------------
def reference_update_ema(target_params, source_params, rate=0.99):
    """the reference's function, restated operator by operator (nn.py:64-65)"""
    for targ, src in zip(target_params, source_params):
        targ.detach().mul_(rate).add_(src, alpha=1 - rate)


def make_params(table, dtype, device="cpu", place=None):
    """-> parameters of the table; `place(i, array)` may put tensor i somewhere particular (views with guards on the GPU)"""
    out = []
    for i, p in enumerate(table.p0):
        t = torch.from_numpy(p.copy()).to(dtype).to(device) if place is None else place(i, p)
        out.append(torch.nn.Parameter(t))
    return out


def param_groups(kind, table, params):
    groups = table.groups(kind)
    out = [dict(params=params[:table.split], **groups[0])]
    if len(groups) > 1:
        out.append(dict(params=params[table.split:], **groups[1]))
    return out


def set_grads(table, params, step, place=None):
    for i, p in enumerate(params):
        g = table.grads[step][i]
        if g is None:
            p.grad = None
        else:
            p.grad = torch.from_numpy(g.copy()).to(p.dtype).to(p.device) if place is None else place(i, g)


def collect(opt, params, emas):
    """-> result dict of float64 numpy arrays: params, states (torch's keys; step as a float), emas"""
    states = []
    for p in params:
        st = opt.state.get(p, {})
        states.append({k: (float(v) if k == "step" else v.detach().double().cpu().numpy()) for k, v in st.items() if v is not None})
    return dict(params=[p.detach().double().cpu().numpy() for p in params], states=states,
                emas=[[e.detach().double().cpu().numpy() for e in es] for es in emas])


def run_torch(kind, table, dtype, n_ema=0):
    """STEPS steps of torch.optim's own optimizer on the CPU in `dtype`, the EMA copies by the reference's update_ema"""
    cls, common, _ = KINDS[kind]
    params = make_params(table, dtype)
    opt = getattr(torch.optim, cls)(param_groups(kind, table, params), **common)
    emas = [[p.detach().clone() for p in params] for _ in range(n_ema)]
    base = [g["lr"] for g in opt.param_groups]
    for s in range(STEPS):
        for g, lr in zip(opt.param_groups, base):
            g["lr"] = lr * (0.5 if s >= 2 else 1.0)
        set_grads(table, params, s)
        opt.step()
        for k in range(n_ema):
            reference_update_ema(emas[k], params, EMA_RATES[k])
    return collect(opt, params, emas)


def _maxabs(a):
    return float(np.abs(a).max()) if a.size else 0.0


def compare(kind, table, got, ref):
    """-> {"param", "state", "ema"}: the largest per-tensor error of each class, in the units of the module docstring"""
    cls, common, _ = KINDS[kind]
    groups = table.groups(kind)
    err = dict(param=0.0, state=0.0, ema=0.0)
    for i, (p, r) in enumerate(zip(got["params"], ref["params"])):
        lr = lr_at(groups[table.group_of(i)], STEPS - 1)
        d = _maxabs(p - r)
        if table.grads[0][i] is None:
            assert d == 0.0 and not got["states"][i], "a parameter without a grad moved"
            continue
        if cls == "SGD":
            buf = ref["states"][i].get("momentum_buffer") if common["momentum"] != 0 else ref["eff"][STEPS - 1][i]
            scale = lr * _maxabs(buf)
            err["param"] = max(err["param"], d / scale if scale > 0 else d)
        else:
            err["param"] = max(err["param"], d / lr)
        for k, rv in ref["states"][i].items():
            if k == "step":
                assert got["states"][i]["step"] == rv, (got["states"][i]["step"], rv)
                continue
            s = _maxabs(rv)
            dv = _maxabs(got["states"][i][k] - rv)
            err["state"] = max(err["state"], dv / s if s > 0 else dv)
    for es, rs in zip(got["emas"], ref["emas"]):
        for e, r in zip(es, rs):
            err["ema"] = max(err["ema"], _maxabs(e - r) / _maxabs(r))
    return err


def plain_err(got, ref):
    """largest max |a - ref| / max |ref| over every parameter, state and EMA tensor (the float64 comparison against torch.optim: one
    float64 ulp of a parameter near 1 is already 1e-13 lr, so the lr units of `compare` cannot resolve 1e-13 there)"""
    worst = 0.0
    pairs = list(zip(got["params"], ref["params"])) + [(e, r) for es, rs in zip(got["emas"], ref["emas"]) for e, r in zip(es, rs)]
    for gs, rs in zip(got["states"], ref["states"]):
        assert gs.keys() == rs.keys(), (gs.keys(), rs.keys())
        pairs += [(np.asarray(gs[k], dtype=np.float64), np.asarray(rs[k], dtype=np.float64)) for k in rs]
    for a, r in pairs:
        s = _maxabs(r)
        worst = max(worst, _maxabs(a - r) / s if s > 0 else _maxabs(a - r))
    return worst


def check_condition(table, kind, run):
    """every effective gradient entry of a run ({"eff"}: per step, a list of float64 arrays or None) is exactly 0 or at least MIN_GRAD in magnitude"""
    for e in (e for step in run["eff"] for e in step if e is not None):
        a = np.abs(e)
        assert not np.any((a > 0) & (a < MIN_GRAD)), (table.name, kind, float(a[a > 0].min()))


def effective_grads_f32(kind, table):
    """the effective gradients torch's float32 run sees: g + wd p (coupled kinds) on the float32 run's own parameters"""
    cls, common, _ = KINDS[kind]
    params = make_params(table, torch.float32)
    opt = getattr(torch.optim, cls)(param_groups(kind, table, params), **common)
    eff = []
    for s in range(STEPS):
        set_grads(table, params, s)
        eff.append([])
        for g in opt.param_groups:
            wd = 0.0 if cls == "AdamW" else g["weight_decay"]
            eff[-1] += [(p.grad + wd * p.detach()).double().numpy() for p in g["params"] if p.grad is not None]
        opt.step()
    return dict(eff=eff)


def measure_f32(c=None, S=None):
    """torch.optim in float32 on the CPU against the float64 restatement -> {"adam", "sgd", "state", "ema"}, maximised over tables, kinds"""
    if c is None:
        c, S = chunk_and_slab()
    out = dict(adam=0.0, sgd=0.0, state=0.0, ema=0.0)
    for name in table_names():
        table = Table(name, c, S)
        for kind in KINDS:
            n_ema = 4 if kind in ("adamw", "sgd") else 1
            e = compare(kind, table, run_torch(kind, table, torch.float32, n_ema), run_restate(kind, table, n_ema))
            key = "sgd" if KINDS[kind][0] == "SGD" else "adam"
            out[key] = max(out[key], e["param"])
            out["state"] = max(out["state"], e["state"])
            out["ema"] = max(out["ema"], e["ema"])
    return out


if __name__ == "__main__":
    m = measure_f32()
    print(f"chunk, slab = {chunk_and_slab()}")
    print(f"ADAM_F32_ERR {m['adam']:.2e} (recorded {ADAM_F32_ERR:.2e})   SGD_F32_ERR {m['sgd']:.2e} (recorded {SGD_F32_ERR:.2e})   "
          f"STATE_F32_ERR {m['state']:.2e} (recorded {STATE_F32_ERR:.2e})   EMA_F32_ERR {m['ema']:.2e} (recorded {EMA_F32_ERR:.2e})")
