"""ORACLE — test infrastructure only.  Interprets a lowered ConvNet plan (audiopure_amd.convnet.Plan) with plain
PyTorch-CPU ops, so the lowering (ATen tape -> fused plan) can be checked against the original nn.Module without a
GPU, and the HIP executor can be checked against the same plan on the GPU box.  The reference semantics are those of
the module itself: audio_models/ConvNets_SpeechCommands/models/*.py forward()."""
import torch
import torch.nn.functional as F


def run_plan_torch(plan, x: torch.Tensor) -> torch.Tensor:
    B = x.shape[0]
    bufs = {plan.input.buf: x.float()}

    def buf(v):
        if v.buf not in bufs:
            C, H, W = plan.buf_shape[v.buf]
            bufs[v.buf] = torch.full((B, C, H, W), float("nan"))
        return bufs[v.buf]

    def rd(v):
        return buf(v)[:, v.coff:v.coff + v.C].reshape(B, v.C, v.H, v.W)

    def wr(v, t):
        buf(v)[:, v.coff:v.coff + v.C] = t.reshape(B, v.C, *buf(v).shape[2:])

    Wt = plan.weights
    for s in plan.steps:
        p = s.p
        if s.kind == "conv":
            w = Wt[p["wk"]]
            if p["sk"]:
                w = w * Wt[p["sk"]].view(-1, 1, 1, 1)
            y = F.conv2d(rd(s.ins[0]), w, Wt[p["bk"]] if p["bk"] else None, stride=p["stride"], padding=p["pad"],
                         groups=p["groups"])
            if p["res"] is not None:
                y = y + rd(p["res"])
            wr(s.out, F.relu(y) if p["relu"] else y)
        elif s.kind == "affine":
            y = rd(s.ins[0])
            if p["sk"]:
                y = y * Wt[p["sk"]].view(1, -1, 1, 1) + Wt[p["hk"]].view(1, -1, 1, 1)
            wr(s.out, F.relu(y) if p["relu"] else y)
        elif s.kind == "add":
            y = rd(s.ins[0]) + rd(s.ins[1])
            wr(s.out, F.relu(y) if p["relu"] else y)
        elif s.kind == "copy":
            wr(s.out, rd(s.ins[0]))
        elif s.kind == "pool":
            f = F.max_pool2d if p["is_max"] else F.avg_pool2d
            wr(s.out, f(rd(s.ins[0]), p["k"], p["stride"], p["pad"]))
    o = plan.output
    y = rd(o)
    return y.reshape(B, -1) if (o.H == 1 and o.W == 1) else y


# ---------------------------------------------------------------------------------------------------------
# One step at a time, and the plan as a LINEAR map once the native forward has made its selections
# ---------------------------------------------------------------------------------------------------------
def read_val(bufs, v):
    """The [B, C, H, W] value `v` names inside the buffers of a run (``NativeConvNet._run``'s, moved to the CPU)."""
    t = bufs[v.buf]
    return t[:, v.coff:v.coff + v.C].reshape(t.shape[0], v.C, v.H, v.W)


def _folded_weight(plan, p, dtype):
    w = plan.weights[p["wk"]].to(dtype)
    if p["sk"]:
        w = w * plan.weights[p["sk"]].to(dtype).view(-1, 1, 1, 1)     # BatchNorm scale folded in `dtype`
    return w


def _step_value(plan, s, ins, dtype, native_in=None, native_out=None):
    """Output of step `s` from its input values `ins` (already in `dtype`).  With `native_out` every ReLU becomes a
    multiplication with the mask [native_out > 0], with `native_in` a max-pool gathers at the first maxima of `native_in`
    (torch's CPU rule: the first maximum of a window in row-major order wins) -- the step is then linear in `ins`."""
    p, Wt = s.p, plan.weights

    def relu(y):
        if not p.get("relu"):
            return y
        return F.relu(y) if native_out is None else y * (native_out > 0).to(dtype)

    if s.kind == "conv":
        y = F.conv2d(ins[0], _folded_weight(plan, p, dtype), Wt[p["bk"]].to(dtype) if p["bk"] else None, stride=p["stride"],
                     padding=p["pad"], groups=p["groups"])
        if p["res"] is not None:
            y = y + ins[1]
        return relu(y)
    if s.kind == "affine":
        y = ins[0]
        if p["sk"]:
            y = y * Wt[p["sk"]].to(dtype).view(1, -1, 1, 1) + Wt[p["hk"]].to(dtype).view(1, -1, 1, 1)
        return relu(y)
    if s.kind == "add":
        return relu(ins[0] + ins[1])
    if s.kind == "copy":
        return ins[0]
    if s.kind == "pool":
        if not p["is_max"]:
            return F.avg_pool2d(ins[0], p["k"], p["stride"], p["pad"])
        if native_in is None:
            return F.max_pool2d(ins[0], p["k"], p["stride"], p["pad"])
        _, idx = F.max_pool2d(native_in, p["k"], p["stride"], p["pad"], return_indices=True)
        return ins[0].flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
    raise ValueError(f"unknown step kind {s.kind!r}")


def step_torch(plan, step, bufs, dtype=torch.float64):
    """Output [B, C, H, W] of ONE step (a Step of `plan`, or its index) computed in `dtype` from the given input buffers --
    the semantics of run_plan_torch, BatchNorm scale folded into the weight in `dtype`."""
    s = plan.steps[step] if isinstance(step, int) else step
    return _step_value(plan, s, [read_val(bufs, v).to(dtype) for v in s.ins], dtype)


def forward_bufs_torch(plan, x, dtype=torch.float32):
    """run_plan_torch keeping every buffer: {buf id: [B, C, H, W]} as ``NativeConvNet._run`` returns them."""
    B = x.shape[0]
    bufs = {plan.input.buf: x.to(dtype)}
    for s in plan.steps:
        y = step_torch(plan, s, bufs, dtype)
        o = s.out
        if o.buf not in bufs:
            C, H, W = plan.buf_shape[o.buf]
            bufs[o.buf] = torch.full((B, C, H, W), float("nan"), dtype=dtype)
        bufs[o.buf][:, o.coff:o.coff + o.C] = y.reshape(B, o.C, *bufs[o.buf].shape[2:])
    return bufs


def replay_linearised(plan, bufs, dtype=torch.float64):
    """The whole plan as a differentiable torch graph in `dtype`, with the selections of the run that produced `bufs`:
    every ReLU is y * [out > 0] of that run's output buffer, every max-pool gathers where that run's input buffer has its
    first maximum.  -> (x, outs, y): the input leaf (a copy of the run's input), every step's output value (retain_grad set,
    in plan order) and the plan's output.  With the selections fixed, dout -> every gradient is linear: an executor that
    made the same selections must agree with it to rounding."""
    x = bufs[plan.input.buf].detach().to(dtype).clone().requires_grad_(True)
    B = x.shape[0]
    cur = {plan.input.buf: x}

    def rd(v):
        t = cur[v.buf]
        return t[:, v.coff:v.coff + v.C].reshape(B, v.C, v.H, v.W)

    outs = []
    for s in plan.steps:
        nat_in = read_val(bufs, s.ins[0]) if s.kind == "pool" and s.p["is_max"] else None
        y = _step_value(plan, s, [rd(v) for v in s.ins], dtype, native_in=nat_in, native_out=read_val(bufs, s.out))
        y.retain_grad()
        outs.append(y)
        o = s.out
        C, H, W = plan.buf_shape[o.buf]
        if o.coff == 0 and o.C == C:
            cur[o.buf] = y.reshape(B, C, H, W)
        else:                                                       # a slice of a torch.cat destination
            old = cur.get(o.buf)
            if old is None:
                old = torch.zeros((B, C, H, W), dtype=dtype)
            cur[o.buf] = torch.cat([old[:, :o.coff], y.reshape(B, o.C, H, W), old[:, o.coff + o.C:]], 1)
    o = plan.output
    return x, outs, rd(o).reshape(B, -1) if (o.H == 1 and o.W == 1) else rd(o)


def replay_gradients(plan, bufs, dout, dtype=torch.float64):
    """-> (dx, [gradient of every step's output value, None where nothing downstream reads it]) of the linearised replay."""
    x, outs, y = replay_linearised(plan, bufs, dtype)
    y.backward(dout.to(dtype).reshape(y.shape))
    return x.grad, [t.grad for t in outs]
