"""Native execution of the reference's 2-D ConvNet classifiers.

The eval scripts receive the classifier as an arbitrary pickled ``nn.Module`` (``audio_models/create_model.py:8-17``):
VGG19-BN, ResNet, WideResNet, ResNeXt, DPN or DenseNet from ``audio_models/ConvNets_SpeechCommands/models``.  All of
them are static graphs of conv / batch-norm / ReLU / pooling / add / cat / slice / linear, so instead of one
hand-written executor per family the module is *lowered once*: an eval-mode forward on a tiny CPU example is recorded
at the ATen level (``TorchDispatchMode`` — immune to how the Python is written, e.g. ``resnext.py`` calling
``.forward`` directly), BatchNorm is folded into the preceding conv (or becomes a per-channel affine), ReLU / residual
adds are fused where the graph allows, and the resulting plan runs on the HIP primitives of ``include/audiopure.h``
(``ap_conv2d_fwd`` = conv-as-GEMM on the fp32 MFMA, ``ap_affine_nchw``, ``ap_add_nchw``, ``ap_copy_channels``,
``ap_pool2d``).  PyTorch allocates the buffers; no torch operator runs in the eval ``forward``.

In ``train()`` mode (``train_speech_commands.py:122-153``) the same tape is lowered to a *train plan* instead
(``lower(module, chw, train=True)``): BatchNorm stays a ``bn`` step on batch statistics (``ap_bn2d_train_fwd`` / ``_bwd``), the plan
names the module's live parameters, and the reverse sweep also leaves every parameter gradient (``ap_conv2d_wgrad``, ``ap_rowsum``).
The train step's torch operators are bookkeeping only: one fused increment of the ``num_batches_tracked`` counters per forward and the
zero fill of each gradient buffer of the sweep.  Live dropout (every ``vgg*``, ``wideresnet28_10D``) is a ``drop`` step of that plan on
the library's counter-based Philox masks (``ap_dropout``) where the caller asks for it (``NativeConvNet.set_dropout``); by default it
stays a refusal, since those masks are not torch's generator stream.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import Any

import torch
import torch.nn as nn
from torch.utils._python_dispatch import TorchDispatchMode

from . import _native as N


# ---------------------------------------------------------------------------------------------------------
# 1. ATen tape
# ---------------------------------------------------------------------------------------------------------
class _Tape(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.entries = []
        self.keep = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        self.entries.append((func, args, kwargs or {}, out))
        self.keep.append((args, out))
        return out


def _opname(func) -> str:
    return func._schema.name.split("::")[-1]


# ---------------------------------------------------------------------------------------------------------
# 2. plan
# ---------------------------------------------------------------------------------------------------------
@dataclass
class Val:
    """A [B, C, H, W] activation: channels [coff, coff + C) of buffer `buf`, which has `cstride` channels."""
    buf: int
    C: int
    H: int
    W: int
    cstride: int
    coff: int = 0

    @property
    def full(self):
        return self.coff == 0 and self.C == self.cstride


@dataclass
class Step:
    kind: str                      # conv | affine | add | copy | pool | bn, drop (train plans only)
    out: Val = None
    ins: list = field(default_factory=list)
    p: dict = field(default_factory=dict)


class Plan:
    def __init__(self):
        self.steps: list[Step] = []
        self.nbuf = 0
        self.buf_shape = {}            # buf id -> (C, H, W)
        self.input: Val = None
        self.output: Val = None
        self.weights = {}              # name -> host tensor (folded conv weights / biases / affine vectors)
        self.train = False             # a train plan: BatchNorm is a `bn` step, parameters are NAMED (state-dict keys), nothing cloned

    def new_buf(self, C, H, W) -> Val:
        b = self.nbuf
        self.nbuf += 1
        self.buf_shape[b] = (C, H, W)
        return Val(b, C, H, W, C, 0)


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _need(cond, what: str) -> None:
    """A pattern the library has no kernel for is a ``NotImplementedError`` -- the one failure ``NativeConvNet`` may answer by
    leaving the caller's module as it is (and only outside AUDIOPURE_STRICT); everything else propagates."""
    if not cond:
        raise NotImplementedError("convnet lowering: " + what)


def _train_checks(m: nn.Module, dropout: bool = False):
    """What the train plan does not serve, as ``NotImplementedError`` before anything is traced.  ``dropout``: nn.Dropout is served
    (a ``drop`` step); nn.Dropout2d and nn.AlphaDropout, whose semantics differ, stay refused."""
    bn_of = {}
    for mod in m.modules():
        if dropout and isinstance(mod, nn.modules.dropout._DropoutNd) and not isinstance(mod, nn.Dropout) and mod.p > 0:
            raise NotImplementedError(f"convnet lowering: live {type(mod).__name__} is not served (the drop step is nn.Dropout's "
                                      "per-element mask; whole-channel and alpha dropout differ)")
        if not dropout and isinstance(mod, (nn.Dropout, nn.Dropout2d, nn.AlphaDropout)) and mod.p > 0:
            raise NotImplementedError("convnet lowering: live dropout (nn.Dropout(p > 0) in train() mode) has no kernel")
        if isinstance(mod, nn.modules.batchnorm._BatchNorm):
            _need(mod.affine, "BatchNorm(affine=False) is not served in train() mode")
            _need(mod.track_running_stats and mod.running_mean is not None, "BatchNorm(track_running_stats=False) is not served in train() mode")
            bn_of[id(mod.running_mean)] = mod
    return bn_of


class _DropoutAsOneOp:
    """For the duration of a train-plan trace ``torch.nn.functional.dropout`` -- which nn.Dropout calls too -- is one recognisable
    ATen operator (``native_dropout``) instead of its CPU decomposition (empty_like, bernoulli_, div_, mul)."""

    def __enter__(self):
        import torch.nn.functional as F_
        self.F, self.orig = F_, F_.dropout

        def dropout(input, p=0.5, training=True, inplace=False):
            _need(not inplace, "in-place dropout is not lowered")
            return torch.ops.aten.native_dropout(input, float(p), bool(training))[0]
        F_.dropout = dropout

    def __exit__(self, *exc):
        self.F.dropout = self.orig


def lower(module: nn.Module, example_chw=(1, 32, 32), train: bool = False, dropout: bool = False) -> Plan:
    """Record one forward of `module` on a CPU example [2, C, H, W] and turn it into a Plan: an eval forward with BatchNorm folded
    away, or (``train=True``) a train-mode forward whose plan keeps every BatchNorm as a ``bn`` step on batch statistics and
    names the module's live parameters and buffers by their state-dict keys instead of cloning them.  ``dropout=True`` (train plans
    only): a live nn.Dropout / F.dropout is a ``drop`` step (``ap_dropout`` on the library's Philox stream, ``draw`` = its ordinal in
    execution order) instead of a refusal."""
    import contextlib
    m = copy.deepcopy(module).to("cpu").float()
    m.train(train)
    dropout = bool(dropout and train)
    bn_of = _train_checks(m, dropout) if train else {}
    names = {}
    for n_, t in list(m.named_parameters()) + list(m.named_buffers()):
        names[id(t)] = n_
    x = torch.zeros((2,) + tuple(example_chw))
    tape = _Tape()
    with torch.no_grad(), (_DropoutAsOneOp() if dropout else contextlib.nullcontext()), tape:
        y = m(x)
    plan = Plan()
    plan.train = train
    n_drop = 0
    vals: dict[int, Any] = {}         # id(tensor) -> Val | ("param", tensor) | ("paramT", tensor)
    plan.input = plan.new_buf(*example_chw)
    vals[id(x)] = plan.input

    def get(t):
        if id(t) in vals:
            return vals[id(t)]
        if id(t) in names or isinstance(t, nn.Parameter):
            return ("param", t)
        raise NotImplementedError("convnet lowering: tensor with unknown producer")

    wcount = [0]

    def add_weight(t):
        k = f"w{wcount[0]}"
        wcount[0] += 1
        plan.weights[k] = t.detach().float().contiguous().clone()
        return k

    for func, args, kwargs, out in tape.entries:
        op = _opname(func)
        if train and op in ("add", "add_") and id(args[0]) in names and not args[0].is_floating_point():
            continue                                # num_batches_tracked += 1: the executor's bookkeeping
        if op in ("detach", "alias", "clone", "contiguous", "_to_copy", "dropout", "native_dropout"):
            src = args[0]
            if train and op in ("dropout", "native_dropout"):
                live_drop = args[1] > 0 and (len(args) < 3 or args[2] is None or args[2])
                _need(dropout or not live_drop, "live dropout (p > 0 in train() mode) has no kernel")
                if live_drop:
                    v = get(src)
                    _need(args[1] < 1, "dropout with p = 1 is not served")
                    _need(isinstance(v, Val) and v.full, "dropout on a channel slice of a wider buffer (coff != 0 or cstride != C) is not served")
                    o = plan.new_buf(v.C, v.H, v.W)
                    plan.steps.append(Step("drop", o, [v], dict(p=float(args[1]), draw=n_drop)))
                    n_drop += 1
                    vals[id(out[0] if isinstance(out, tuple) else out)] = o
                    continue
            vals[id(out if not isinstance(out, tuple) else out[0])] = get(src)
        elif op == "convolution":
            xin, w, b, stride, padding, dilation, transposed, _, groups = args[:9]
            _need(not transposed and tuple(dilation) == (1, 1), "dilated / transposed conv2d not lowered")
            s, p_ = _pair(stride), _pair(padding)
            _need(s[0] == s[1] and p_[0] == p_[1], "anisotropic stride / padding not lowered")
            v = get(xin)
            o = plan.new_buf(out.shape[1], out.shape[2], out.shape[3])
            plan.steps.append(Step("conv", o, [v], dict(w=w.detach().float(), b=None if b is None else b.detach().float(),
                                                        stride=s[0], pad=p_[0], groups=groups, relu=False, res=None,
                                                        kh=w.shape[2], kw=w.shape[3], wsrc=w, bsrc=b)))
            vals[id(out)] = o
        elif train and op in ("_native_batch_norm_legit_no_training", "native_batch_norm", "cudnn_batch_norm", "_native_batch_norm_legit",
                              "_native_batch_norm_legit_functional"):
            xin, w, b, mean, var = args[:5]
            _need(isinstance(mean, torch.Tensor) and id(mean) in bn_of, "BatchNorm without tracked running statistics is not served in train() mode")
            _need(w is not None and b is not None and id(w) in names and id(b) in names, "BatchNorm(affine=False) is not served in train() mode")
            mod = bn_of[id(mean)]
            _need(mod.training, "a BatchNorm layer in eval() mode inside a train() module is not served")
            v = get(xin)
            _need(isinstance(v, Val), "shape / argument pattern not lowered")
            o = plan.new_buf(v.C, v.H, v.W)
            rm = names[id(mean)]
            _need(all(s_.kind != "bn" or s_.p["rmname"] != rm for s_ in plan.steps),
                  "a BatchNorm layer applied twice in one forward is not served in train() mode")   # (its d gamma / d beta would have to add up)
            plan.steps.append(Step("bn", o, [v], dict(wname=names[id(w)], bname=names[id(b)], rmname=rm, rvname=names[id(var)],
                                                      nbtname=rm[:-len("running_mean")] + "num_batches_tracked",
                                                      eps=float(mod.eps), momentum=None if mod.momentum is None else float(mod.momentum),
                                                      relu=False)))
            vals[id(out[0])] = o
        elif op in ("_native_batch_norm_legit_no_training", "native_batch_norm", "cudnn_batch_norm",
                    "_native_batch_norm_legit"):
            xin, w, b, mean, var = args[:5]
            eps = args[-1] if op != "cudnn_batch_norm" else args[7]
            v = get(xin)
            scale = (w if w is not None else torch.ones_like(mean)).detach().double() / torch.sqrt(var.detach().double() + eps)
            shift = (b if b is not None else torch.zeros_like(mean)).detach().double() - mean.detach().double() * scale
            o = plan.new_buf(v.C, v.H, v.W)
            plan.steps.append(Step("affine", o, [v], dict(scale=scale.float(), shift=shift.float(), relu=False)))
            vals[id(out[0])] = o
        elif op in ("relu", "relu_"):
            v = get(args[0])
            o = plan.new_buf(v.C, v.H, v.W)
            plan.steps.append(Step("affine", o, [v], dict(scale=None, shift=None, relu=True)))
            vals[id(out)] = o                       # relu_ returns its (mutated) input: later uses see the new value
        elif op in ("add", "add_"):
            a, b = get(args[0]), get(args[1])
            _need(kwargs.get("alpha", 1) == 1 and isinstance(a, Val) and isinstance(b, Val), "shape / argument pattern not lowered")
            _need((a.C, a.H, a.W) == (b.C, b.H, b.W), "shape / argument pattern not lowered")
            o = plan.new_buf(a.C, a.H, a.W)
            plan.steps.append(Step("add", o, [a, b], dict(relu=False)))
            vals[id(out)] = o
        elif op == "cat":
            ts, dim = args[0], (args[1] if len(args) > 1 else 0)
            _need(dim == 1, "only channel concatenation is lowered")
            vs = [get(t) for t in ts]
            o = plan.new_buf(sum(v.C for v in vs), vs[0].H, vs[0].W)
            off = 0
            for v in vs:
                plan.steps.append(Step("copy", Val(o.buf, v.C, v.H, v.W, o.cstride, off), [v]))
                off += v.C
            vals[id(out)] = o
        elif op == "slice":
            xin, dim = args[0], args[1] if len(args) > 1 else 0
            start = args[2] if len(args) > 2 and args[2] is not None else 0
            end = args[3] if len(args) > 3 and args[3] is not None else xin.shape[dim]
            step = args[4] if len(args) > 4 else 1
            v = get(xin)
            end = min(end, xin.shape[dim])
            if dim == 0 or (start == 0 and end >= xin.shape[dim]):
                vals[id(out)] = v
            else:
                _need(dim == 1 and step == 1 and isinstance(v, Val), "only channel slices are lowered")
                vals[id(out)] = Val(v.buf, end - start, v.H, v.W, v.cstride, v.coff + start)
        elif op in ("max_pool2d_with_indices", "max_pool2d", "avg_pool2d"):
            xin, k = args[0], _pair(args[1])
            stride = _pair(args[2]) if len(args) > 2 and args[2] else k
            pad = _pair(args[3]) if len(args) > 3 else (0, 0)
            _need(k[0] == k[1] and stride[0] == stride[1] and pad[0] == pad[1], "shape / argument pattern not lowered")
            # ap_pool2d computes the floor shape of an undilated window: what it cannot run is refused, never traced at torch's shape
            if op == "avg_pool2d":        # (self, kernel_size, stride, padding, ceil_mode, count_include_pad, divisor_override)
                _need(not (len(args) > 4 and args[4]) and not kwargs.get("ceil_mode", False), "pooling with ceil_mode=True not lowered")
                _need(pad[0] == 0 or (len(args) <= 5 or args[5]), "count_include_pad=False not lowered")
                _need(len(args) <= 6 or args[6] is None, "avg_pool2d with divisor_override not lowered")
            else:                         # (self, kernel_size, stride, padding, dilation, ceil_mode)
                dil = _pair(args[4]) if len(args) > 4 else _pair(kwargs.get("dilation", 1))
                _need(tuple(dil) == (1, 1), "dilated max_pool2d not lowered")
                _need(not (len(args) > 5 and args[5]) and not kwargs.get("ceil_mode", False), "pooling with ceil_mode=True not lowered")
            v = get(xin)
            if not v.full:
                c = plan.new_buf(v.C, v.H, v.W)
                plan.steps.append(Step("copy", c, [v]))
                v = c
            o_t = out[0] if isinstance(out, tuple) else out
            o = plan.new_buf(v.C, o_t.shape[2], o_t.shape[3])
            plan.steps.append(Step("pool", o, [v], dict(k=k[0], stride=stride[0], pad=pad[0], is_max=op != "avg_pool2d")))
            vals[id(o_t)] = o
        elif op in ("mean", "adaptive_avg_pool2d", "_adaptive_avg_pool2d"):
            v = get(args[0])
            if op == "mean":
                dims = sorted(d % 4 for d in args[1])
                _need(dims == [2, 3], "only spatial means are lowered")
            else:
                _need(_pair(args[1]) == (1, 1), "shape / argument pattern not lowered")
            _need(v.H == v.W, "shape / argument pattern not lowered")
            if not v.full:
                c = plan.new_buf(v.C, v.H, v.W)
                plan.steps.append(Step("copy", c, [v]))
                v = c
            o = plan.new_buf(v.C, 1, 1)
            plan.steps.append(Step("pool", o, [v], dict(k=v.H, stride=v.H, pad=0, is_max=False)))
            vals[id(out)] = o
        elif op in ("view", "_unsafe_view", "reshape", "flatten", "squeeze", "unsqueeze"):
            v = get(args[0])
            if isinstance(v, tuple):
                vals[id(out)] = v
                continue
            n_el = v.C * v.H * v.W
            _need(out.numel() == 2 * n_el, "views that mix the batch axis are not lowered")
            if not v.full:
                c = plan.new_buf(v.C, v.H, v.W)
                plan.steps.append(Step("copy", c, [v]))
                v = c
            if out.dim() == 2:
                vals[id(out)] = Val(v.buf, n_el, 1, 1, n_el, 0)      # [B, C*H*W]: same memory
            else:
                vals[id(out)] = Val(v.buf, out.shape[1], out.shape[2], out.shape[3], out.shape[1], 0)
        elif op == "t":
            vals[id(out)] = ("paramT", args[0])
        elif op in ("addmm", "mm", "linear"):
            if op == "addmm":
                b, xin, wt = args[0], args[1], args[2]
                kind, w = get(wt)
                _need(kind == "paramT", "shape / argument pattern not lowered")
            elif op == "mm":
                b, xin = None, args[0]
                kind, w = get(args[1])
                _need(kind == "paramT", "shape / argument pattern not lowered")
            else:
                xin, w, b = args[0], args[1], (args[2] if len(args) > 2 else None)
            v = get(xin)
            _need(v.H == 1 and v.W == 1 and v.full, "shape / argument pattern not lowered")
            o = plan.new_buf(w.shape[0], 1, 1)
            plan.steps.append(Step("conv", o, [v], dict(w=w.detach().float().reshape(w.shape[0], w.shape[1], 1, 1),
                                                        b=None if b is None else b.detach().float(), stride=1, pad=0,
                                                        groups=1, relu=False, res=None, kh=1, kw=1, wsrc=w, bsrc=b)))
            vals[id(out)] = o
        elif op in ("size", "sym_size", "empty", "zeros", "ones", "zeros_like", "empty_like", "fill_", "copy_") or \
                (train and op in ("_local_scalar_dense", "item")):   # (BatchNorm(momentum=None) reads num_batches_tracked)
            continue
        else:
            raise NotImplementedError(f"convnet lowering: ATen op '{op}' is not supported")
    plan.output = get(y)
    _need(isinstance(plan.output, Val), "shape / argument pattern not lowered")
    _fuse(plan, train)
    for st in plan.steps:
        if st.kind == "conv":
            wsrc, bsrc = st.p.pop("wsrc"), st.p.pop("bsrc")
            if train:                               # the module's live tensors, by name: nothing to go stale after optimizer.step()
                _need(id(wsrc) in names and (bsrc is None or id(bsrc) in names), "a convolution whose weight is not a parameter of the module")
                st.p.pop("w"), st.p.pop("b")
                st.p["wname"], st.p["bname"] = names[id(wsrc)], None if bsrc is None else names[id(bsrc)]
                st.p["wshape"] = (wsrc.shape[0], wsrc.shape[1], st.p["kh"], st.p["kw"])
                continue
            st.p["wk"] = add_weight(st.p.pop("w"))
            b = st.p.pop("b")
            st.p["bk"] = None if b is None else add_weight(b)
            sc = st.p.pop("scale", None)
            st.p["sk"] = None if sc is None else add_weight(sc)
        elif st.kind == "affine" and st.p["scale"] is not None:
            st.p["sk"], st.p["hk"] = add_weight(st.p.pop("scale")), add_weight(st.p.pop("shift"))
        elif st.kind == "affine":
            st.p.pop("scale"), st.p.pop("shift")
            st.p["sk"] = st.p["hk"] = None
    return plan


def _fuse(plan: Plan, train: bool = False):
    """conv -> BN (fold) -> ReLU, BN -> ReLU, add -> ReLU, conv (+ residual add) peepholes.  A producer is merged into
    its consumer only when that consumer is the ONLY reader of the producer's buffer.  A train plan folds nothing: BN -> ReLU sets
    the ``bn`` step's flag, add -> ReLU and conv + residual add (a BatchNorm between them is a step of its own, so they are
    not adjacent) stay, a ReLU straight after a conv stays a step."""
    def readers(buf):
        r = sum(1 for s in plan.steps for v in s.ins if v.buf == buf)
        return r + (1 if plan.output.buf == buf else 0)

    changed = True
    while changed:
        changed = False
        for i, st in enumerate(plan.steps):
            if st.kind not in ("affine", "add"):
                continue
            src = st.ins[0]
            prod = next((s for s in plan.steps[:i] if s.out is not None and s.out.buf == src.buf and s.out.full), None)
            if st.kind == "affine" and prod is not None and src.full and readers(src.buf) == 1:
                has_aff = st.p["scale"] is not None
                if prod.kind == "conv" and not train and not prod.p["relu"] and (prod.p["res"] is None or not has_aff):
                    if has_aff:        # fold BN: w' = w * s, b' = b * s + t
                        s_, t_ = st.p["scale"], st.p["shift"]
                        prod.p["scale"] = s_ if prod.p.get("scale") is None else prod.p["scale"] * s_
                        b0 = prod.p["b"] if prod.p["b"] is not None else torch.zeros_like(t_)
                        prod.p["b"] = b0 * s_ + t_
                    prod.p["relu"] = st.p["relu"]
                elif prod.kind in ("affine", "add", "bn") and not has_aff and not prod.p["relu"]:
                    prod.p["relu"] = True
                else:
                    continue
                prod.out = st.out
                plan.steps.pop(i)
                changed = True
                break
            if st.kind == "add" and not st.p["relu"]:
                # conv + residual: the conv output is read only by this add -> let the conv epilogue add the other operand
                for a_i in (0, 1):
                    cv, other = st.ins[a_i], st.ins[1 - a_i]
                    prod = next((s for s in plan.steps[:i] if s.kind == "conv" and s.out.buf == cv.buf), None)
                    if (prod is not None and cv.full and other.full and readers(cv.buf) == 1 and not prod.p["relu"]
                            and prod.p["res"] is None
                            and all(s2.out.buf != other.buf for s2 in plan.steps[plan.steps.index(prod):i])):
                        prod.p["res"] = other
                        prod.ins.append(other)
                        prod.out = st.out
                        plan.steps.pop(i)
                        changed = True
                        break
                if changed:
                    break


# ---------------------------------------------------------------------------------------------------------
# 3. executor
# ---------------------------------------------------------------------------------------------------------
class _ConvNetInputGrad(torch.autograd.Function):
    """Scores with the gradient w.r.t. the input spectrogram formed by the HIP library (white_box_attack.py:392,437-439)."""

    @staticmethod
    def forward(ctx, x, net):
        with torch.no_grad():
            out, bufs = net._run(x.detach())
        ctx.net, ctx.bufs = net, bufs
        return out

    @staticmethod
    def backward(ctx, g):
        with torch.no_grad():
            dx = ctx.net._input_grad(ctx.bufs, g.detach().float().contiguous())
        ctx.bufs = None
        return dx, None


class _ConvNetTrainFn(torch.autograd.Function):
    """Train-mode scores over (x, the module's parameters): the forward keeps every activation and each BatchNorm's batch
    statistics, the backward runs the reverse sweep with ``bn`` steps and, per conv step, ap_conv2d_wgrad + ap_rowsum."""

    @staticmethod
    def forward(ctx, x, net, tplan, names, *params):
        out, saved = net._run_train(x, tplan, keep=True, drop=net._drop_now)
        ctx.net, ctx.tplan, ctx.names, ctx.saved = net, tplan, names, saved
        ctx.save_for_backward(x, *params)                        # (an in-place change of x or a parameter before backward is torch's error;
                                                                 #  the kept input activation may alias x)
        return out

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():                              # create_graph=True reached this node
            raise NotImplementedError("audiopure_amd NativeConvNet: no double backward through the train-mode step (create_graph=True)")
        if ctx.saved is None:
            raise RuntimeError("audiopure_amd NativeConvNet: the train-mode step was already back-propagated (its activations are freed)")
        params = dict(zip(ctx.names, ctx.saved_tensors[1:]))
        want = {n for n, need in zip(ctx.names, ctx.needs_input_grad[4:]) if need}
        bufs, stats, drop = ctx.saved                            # (the dropout stream is kept with the activations: seed and offset)
        tr = _TrainSweep(ctx.tplan, params, stats, want, ctx.needs_input_grad[0], drop)
        with torch.no_grad():
            dx = ctx.net._input_grad(bufs, g.detach().float().contiguous(), train=tr)
        ctx.saved = None
        return (dx if ctx.needs_input_grad[0] else None, None, None, None) + tuple(tr.grads.get(n) for n in ctx.names)


class _TrainSweep:
    """What the reverse sweep needs beyond the activations when it runs a train plan: the live parameters by name, each ``bn``
    step's [2][C] batch statistics, which parameters want a gradient, and where those gradients go."""

    def __init__(self, plan, params, stats, want, want_dx, drop=None):
        self.plan, self.params, self.stats, self.want, self.want_dx = plan, params, stats, want, want_dx
        self.drop = drop                                         # the forward's dropout stream: dict(seed, offset) or None
        self.grads = {}

    def grad_of(self, name):
        """-> (gradient tensor shaped like the parameter, accumulate flag): a parameter two steps share adds up."""
        if name in self.grads:
            return self.grads[name], 1
        self.grads[name] = torch.empty_like(self.params[name], dtype=torch.float32)
        return self.grads[name], 0


class _TrainRun:
    """What the step loop needs to run a train plan: the module's live parameters and buffers by name and the per-plan device images
    (``_train_images``); it leaves each ``bn`` step's [2][C] batch statistics and the counters of the layers that ran."""

    def __init__(self, live, img, drop=None):
        self.live, self.img, self.drop = live, img, drop         # drop: this forward's dropout stream, dict(seed, offset) or None
        self.stats, self.counters = {}, []


def strict() -> bool:
    """``AUDIOPURE_STRICT=1``: the off-native routes of ``NativeConvNet.forward`` raise instead of running PyTorch operators."""
    import os
    return os.environ.get("AUDIOPURE_STRICT", "0") not in ("", "0")


# The reference's six 2-D classifier families (audio_models/ConvNets_SpeechCommands/models/{vgg,resnet,wideresnet,resnext,dpn,
# densenet}.py: the classes create_model() can return).  All of them are known to lower (tests/test_gpu_convnets.py), so for THEM a
# trace that meets an operator without a kernel is a bug of this library, never a reason to run the module on PyTorch operators:
# it raises whatever AUDIOPURE_STRICT says.  The warning route is for genuinely foreign modules only.
KNOWN_FAMILIES = frozenset({"VGG", "ResNet", "WideResNet", "CifarResNeXt", "DPN", "DenseNet"})


class NativeConvNet(nn.Module):
    """``NativeConvNet(module)(x)`` == ``module.eval()(x)`` for the reference's 2-D classifiers, computed by the HIP
    library.  The wrapped module keeps owning the parameters (``.module``); call ``refresh()`` after changing them.
    In ``train()`` mode, with parameters and input on the device, ``forward`` is the module's train-mode forward (batch
    statistics, running statistics updated in place) and its ``backward`` fills the parameters' gradients, both on the HIP library."""

    # class-level defaults: an instance restored without __init__ (copy / pickle of an older object) still works
    plan = None
    input_chw = None
    _dev_weights = None
    _dev = None
    _conv_flags = 0
    _bwd_packed = None
    _bwd_key = None

    def __init__(self, module: nn.Module, input_chw=(1, 32, 32)):
        """``input_chw=None`` defers the lowering to the first forward (the plan is then traced for that input's
        [C, H, W]; the scripts' mel32 / mel40 front-ends give 1x32x32 / 1x40x32)."""
        super().__init__()
        self.module = module
        self.input_chw = tuple(input_chw) if input_chw is not None else None
        self.plan = lower(module, self.input_chw) if input_chw is not None else None

    def __getstate__(self):                    # device images / packed weights are rebuilt on demand, never pickled
        d = dict(self.__dict__)
        for k in ("_dev_weights", "_packed", "_dev", "_bwd_packed", "_bwd_key", "_zero_vec", "_train_plan", "_train_chw", "_train_bufs", "_train_drop", "_drop_now"):
            d.pop(k, None)
        return d

    def set_precision(self, mode: str):
        """"f32": fp32 MFMA (default).  "f32s": eligible conv layers on the bf16 MFMA with exactly 3-way-split fp32
        operands (AP_CONV_SPLIT) -- fp32-class results, faster.  "f16x2": the same layers with operands as two fp16 parts on the
        fp16 MFMA (AP_CONV_SPLIT_F16; NOT fp32-class: weights and activations must stay below 3750 in magnitude and within
        fp16's exponent range of each other -- the UNet's normalised activations do; "f32h" is the round-3/4 name of this flag)."""
        self._conv_flags = {"f32": 0, "fp32": 0, "f32s": 0x100, "f32_split": 0x100, "f16x2": 0x400, "f32h": 0x400}[mode]
        return self

    def _get_name(self):                       # the scripts print / branch on the classifier's class name
        return self.module._get_name()

    def refresh(self):
        """Re-lower after the wrapped module changed.  Also drops the train plan, which holds each BatchNorm's eps and momentum and
        the decision that no dropout is live as they were when it was traced: change those on the module, then call this."""
        self.plan = lower(self.module, self.input_chw)
        self._dev_weights = None
        self._train_plan, self._train_chw, self._train_bufs = None, None, None

    def _prepare(self, dev):
        lib = N.lib()
        W = {k: v.to(dev) for k, v in self.plan.weights.items()}
        packed = {}
        for i, st in enumerate(self.plan.steps):
            if st.kind != "conv":
                continue
            w = W[st.p["wk"]]
            Cout, Cg, kh, kw = w.shape
            wT = torch.empty(lib.ap_conv2d_packed_elems(Cout, Cg, kh, kw, st.p["groups"]), device=dev, dtype=torch.float32)
            sc = W[st.p["sk"]].contiguous() if st.p["sk"] else None
            N.check(lib.ap_conv2d_pack(N.ptr(w.contiguous()), N.ptr(sc), N.ptr(wT), Cout, Cg, kh, kw, st.p["groups"], N.stream()),
                    "ap_conv2d_pack")
            packed[i] = wT
        torch.cuda.synchronize(dev)
        self._dev_weights, self._packed, self._dev = W, packed, dev

    _foreign = False                           # set when a lazily lowered module turns out not to be a ConvNet this library knows

    def _off_native(self, x, why: str):
        """The ONLY place a caller's module runs on PyTorch operators.  ``AUDIOPURE_STRICT=1`` (set by tests/conftest.py, bench.py and
        tools/run_cfg4_step.py) turns every such route into an error, so a lowering bug can never pass for the native path; for the
        reference's own six families a failed lowering raises even without it (``KNOWN_FAMILIES``)."""
        if strict():
            raise N.NativeError(f"{type(self.module).__name__}: {why}; AUDIOPURE_STRICT=1 forbids running the caller's module "
                                "on PyTorch operators")
        return self.module(x)

    def forward(self, x):
        """A module that ``lower_classifier`` wrapped on sight (``input_chw=None``) is only KNOWN to contain Conv2d layers.
        What the reference's scripts would have done with it stays possible in three named cases -- ``train()`` mode where the
        train plan has no kernel (live dropout without ``set_dropout``, ``affine=False``, ...) or the module is not on the device, a CPU module fed CPU tensors, and a trace that meets an operator the library has no
        kernel for (``lower`` raises ``NotImplementedError``; any other failure of the lowering propagates) -- each said once with
        a ``RuntimeWarning`` and each an error under ``AUDIOPURE_STRICT=1``.  An explicitly constructed
        ``NativeConvNet(module, chw)`` lowers in ``__init__`` and raises there instead."""
        if self.training and not self._foreign:
            self.plan, self._dev_weights = None, None            # the eval plan holds weights folded at lowering: stale after a training step
            if x.is_cuda and all(p.is_cuda for p in self.module.parameters()):
                try:
                    tplan = self._train_plan_for(x)
                except NotImplementedError as e:                 # live dropout, affine=False, ...: no kernel -- today's announced route
                    if strict():
                        hint = ("; set_dropout('philox') opts in to the library's own Philox masks" if ("dropout" in str(e) or "bernoulli_" in str(e))
                                and self._dropout is None else "")   # (F.dropout traces as empty_like, bernoulli_, div_, mul)
                        raise N.NativeError(f"{type(self.module).__name__}: train() mode not lowered ({e}{hint}); AUDIOPURE_STRICT=1 forbids "
                                            "running the caller's module on PyTorch operators") from e
                else:
                    return self._forward_train(x, tplan)         # batch-statistics BatchNorm and parameter gradients on the HIP library
            if not getattr(self, "_warned_train", False):
                import warnings
                warnings.warn(f"{type(self.module).__name__}: train() mode -- the caller's module runs on PyTorch operators; the "
                              "native plan is re-lowered from the parameters at the next eval() forward", RuntimeWarning, stacklevel=2)
                self._warned_train = True
            return self._off_native(x, "train() mode")
        if self._foreign:
            return self._off_native(x, "not lowered (an operator without a kernel)")
        if not x.is_cuda and self.plan is None and all(not p.is_cuda for p in self.module.parameters()):
            return self._off_native(x, "CPU module and CPU input")
        return self._forward_native(x)

    @N.on_device
    def _forward_native(self, x):
        if self.plan is None and x.is_cuda and x.dim() == 4:     # deferred lowering (input_chw=None)
            try:
                self.input_chw = tuple(x.shape[1:])
                self.plan = lower(self.module, self.input_chw)
                self._dev_weights = None
            except NotImplementedError as e:                     # "no kernel for this operator" -- nothing else is caught: an OOM, a
                import warnings                                  # NativeError or a bug in the lowering must not latch a silent fallback
                self.plan, self.input_chw = None, None
                if strict() or type(self.module).__name__ in KNOWN_FAMILIES:
                    raise                                        # (a known family that does not lower is a bug here, not a foreign module)
                warnings.warn(f"{type(self.module).__name__}: not lowered onto the HIP library ({e}); the module runs as "
                              "the caller built it (PyTorch operators)", RuntimeWarning, stacklevel=3)
                self._foreign = True
                return self._off_native(x, f"not lowered ({e})")
        if torch.is_grad_enabled() and x.requires_grad:
            return _ConvNetInputGrad.apply(x, self)              # white-box attack: dL/dx (parameters frozen)
        self.native_calls = getattr(self, "native_calls", 0) + 1
        return self._run(x)[0]

    def _run(self, x):
        """-> (output, every buffer of the plan) -- the backward pass needs the intermediate activations."""
        if not x.is_cuda:
            raise N.NativeError("NativeConvNet needs a HIP device tensor; there is no CPU path")
        if self.plan is None and x.dim() == 4:                   # deferred lowering (input_chw=None)
            self.input_chw = tuple(x.shape[1:])
            self.plan = lower(self.module, self.input_chw)
            self._dev_weights = None
        if x.dim() != 4 or tuple(x.shape[1:]) != self.input_chw:
            raise ValueError(f"expected [B, {self.input_chw}], got {tuple(x.shape)}")
        dev = x.device
        if self._dev_weights is None or self._dev != dev:
            self._prepare(dev)
        N.use_conv_workspace(dev)
        return self._execute(x, self.plan)

    def _execute(self, x, plan, tr=None):
        """The one step loop of both plans -> (output, every buffer of the plan).  Two step kinds depend on the mode.  ``conv``: the
        eval plan reads the image ``_prepare`` packed (BatchNorm folded in, ReLU and the precision flags in the launch); with ``tr``
        (a ``_TrainRun``) the image is packed from the module's live weight before every launch and the launch carries no flag.
        ``bn`` exists in train plans only: batch statistics into ``tr.stats``, the layer's counter into ``tr.counters``."""
        lib, W, B, dev, st_ = N.lib(), self._dev_weights, x.shape[0], x.device, N.stream()
        bufs = {plan.input.buf: x.detach().float().contiguous()}

        def buf(v):
            if v.buf not in bufs:
                C_, H_, W_ = plan.buf_shape[v.buf]
                bufs[v.buf] = torch.empty((B, C_, H_, W_), device=dev, dtype=torch.float32)
            return bufs[v.buf]

        for i, s in enumerate(plan.steps):
            o, p = s.out, s.p
            ob = buf(o)
            if s.kind == "conv":
                v = s.ins[0]
                assert o.full
                if tr is None:
                    wimg, bias, flags = self._packed[i], (W[p["bk"]] if p["bk"] else None), int(p["relu"]) | self._conv_flags
                else:
                    assert not p["relu"]
                    Cout, Cg, kh, kw = p["wshape"]
                    wimg, bias, flags = tr.img["fwd"][i], (tr.live[p["bname"]].detach() if p["bname"] else None), 0
                    N.check(lib.ap_conv2d_pack(N.ptr(tr.live[p["wname"]].detach()), None, N.ptr(wimg), Cout, Cg, kh, kw, p["groups"], st_),
                            "ap_conv2d_pack")
                res = N.ptr(buf(p["res"])) if p["res"] is not None else None
                N.check(lib.ap_conv2d_fwd(N.ptr(buf(v)), N.ptr(wimg), N.ptr(bias), res, N.ptr(ob), B, v.C, v.H, v.W, o.C, p["kh"], p["kw"],
                                          p["stride"], p["pad"], p["groups"], flags, v.cstride, v.coff, st_), "ap_conv2d_fwd")
            elif s.kind == "bn":
                v = s.ins[0]
                assert o.full
                live, ws = tr.live, tr.img["bn_ws"]
                nbt = live.get(p["nbtname"])
                mom = p["momentum"] if p["momentum"] is not None else 1.0 / (int(nbt) + 1)   # momentum=None: the cumulative average
                stat = torch.empty((2, o.C), device=dev, dtype=torch.float32)
                N.check(lib.ap_bn2d_train_fwd(N.ptr(buf(v)), N.ptr(live[p["wname"]].detach()), N.ptr(live[p["bname"]].detach()),
                                              N.ptr(live[p["rmname"]]), N.ptr(live[p["rvname"]]), N.ptr(ob), N.ptr(stat), ws.data_ptr(),
                                              ws.numel(), B, o.C, o.H * o.W, v.cstride, v.coff, p["eps"], mom, int(p["relu"]), st_),
                        "ap_bn2d_train_fwd")
                if nbt is not None:
                    tr.counters.append(nbt)
                tr.stats[i] = stat
            elif s.kind == "drop":                               # the mask is a function of (seed, draw, sample, element): nothing is kept
                v = s.ins[0]
                assert o.full and v.full and tr.drop is not None
                N.check(lib.ap_dropout(N.ptr(buf(v)), N.ptr(ob), B, v.C * v.H * v.W, p["p"], tr.drop["seed"], p["draw"], tr.drop["offset"],
                                       st_), "ap_dropout")
            elif s.kind == "affine":
                v = s.ins[0]
                assert o.full and (tr is None or p["sk"] is None)    # a train plan's affine steps are bare ReLUs (lower())
                N.check(lib.ap_affine_nchw(N.ptr(buf(v)), N.ptr(W[p["sk"]]) if p["sk"] else None,
                                           N.ptr(W[p["hk"]]) if p["hk"] else None, N.ptr(ob), B, v.C, v.H * v.W, v.cstride,
                                           v.coff, int(p["relu"]), st_), "ap_affine_nchw")
            elif s.kind == "add":
                a, b = s.ins
                assert o.full
                N.check(lib.ap_add_nchw(N.ptr(buf(a)), N.ptr(buf(b)), N.ptr(ob), B, a.C, a.H * a.W, a.cstride, a.coff,
                                        b.cstride, b.coff, int(p["relu"]), st_), "ap_add_nchw")
            elif s.kind == "copy":
                v = s.ins[0]
                N.check(lib.ap_copy_channels(N.ptr(buf(v)), N.ptr(ob), B, v.C, v.H * v.W, v.cstride, v.coff, o.cstride,
                                             o.coff, st_), "ap_copy_channels")
            elif s.kind == "pool":
                v = s.ins[0]
                N.check(lib.ap_pool2d(N.ptr(buf(v)), N.ptr(ob), B * v.C, v.H, v.W, p["k"], p["stride"], p["pad"],
                                      int(p["is_max"]), st_), "ap_pool2d")
        o = plan.output
        out = buf(o)
        assert o.full
        return (out.view(B, -1) if (o.H == 1 and o.W == 1) else out), bufs

    # ---- train() mode: batch-statistics BatchNorm, parameter gradients (train_speech_commands.py:122-153) ---------
    _train_plan = None
    _train_chw = None
    _train_bufs = None                         # per conv step: the packed forward / backward weight images, written anew every step

    _dropout = None                            # set_dropout's spec
    _train_drop = False                        # whether the cached train plan was lowered with dropout=True
    _drop_now = None                           # the dropout stream of the train forward that is running

    def set_dropout(self, spec):
        """How a live nn.Dropout / F.dropout of the wrapped module runs in ``train()`` mode.
        ``None`` (default): it does not -- the train plan refuses it (an error under AUDIOPURE_STRICT=1, else the announced PyTorch route).
        ``"philox"``: the library's counter-based Philox masks (``ap_dropout``; NOT torch's generator stream); every train-mode forward
        draws a 64-bit seed from torch's CPU generator, so ``torch.manual_seed`` reproduces a run; sample offset 0.
        ``("philox", seed, sample_offset)``: a fixed stream; ``sample_offset`` is the global index of the batch's first sample (a
        sharded batch).  Eval mode is unaffected: dropout is inert there."""
        if spec is not None and spec != "philox":
            if not (isinstance(spec, (tuple, list)) and len(spec) == 3 and spec[0] == "philox"):
                raise ValueError('set_dropout: None, "philox" or ("philox", seed, sample_offset)')
            spec = ("philox", int(spec[1]) & ((1 << 64) - 1), int(spec[2]))
            if spec[2] < 0:
                raise ValueError("set_dropout: sample_offset must not be negative")
        self._dropout = spec
        return self

    def _dropout_stream(self):
        """-> dict(seed, offset) of one train-mode forward, or None where dropout is not opted in."""
        if self._dropout is None:
            return None
        if self._dropout == "philox":
            w = torch.randint(0, 1 << 32, (2,), dtype=torch.int64)   # torch's CPU generator: torch.manual_seed reproduces a step
            return dict(seed=(int(w[0]) << 32) | int(w[1]), offset=0)
        return dict(seed=self._dropout[1], offset=self._dropout[2])

    def _train_plan_for(self, x):
        if x.dim() != 4:
            raise ValueError(f"expected [B, C, H, W], got {tuple(x.shape)}")
        chw = tuple(x.shape[1:])
        drop = self._dropout is not None
        if self._train_plan is None or self._train_chw != chw or self._train_drop != drop:     # cached per setting: toggling re-lowers
            self._train_plan = None
            self._train_plan, self._train_chw, self._train_drop, self._train_bufs = lower(self.module, chw, train=True, dropout=drop), chw, drop, None
        return self._train_plan

    def _live_tensors(self):
        d = dict(self.module.named_parameters())
        d.update(self.module.named_buffers())
        return d

    @N.on_device
    def _forward_train(self, x, tplan):
        if self._conv_flags:
            raise N.NativeError("NativeConvNet: train() mode runs in 'f32' only; set_precision('f32') before training")
        live = self._live_tensors()
        pnames = tuple(n for n, _ in self.module.named_parameters())
        if any(live[n].dtype != torch.float32 or not live[n].is_contiguous() for n in pnames):
            raise N.NativeError("NativeConvNet: train() mode needs contiguous float32 parameters")
        self._drop_now = self._dropout_stream() if any(s.kind == "drop" for s in tplan.steps) else None
        if torch.is_grad_enabled() and (x.requires_grad or any(live[n].requires_grad for n in pnames)):
            return _ConvNetTrainFn.apply(x, self, tplan, pnames, *[live[n] for n in pnames])
        return self._run_train(x, tplan, keep=False, drop=self._drop_now)[0]   # no_grad: the statistics move (and the same masks apply), nothing is kept

    def _train_images(self, tplan, dev):
        """Device buffers for the packed weight images of every conv step (forward and transposed), the flip scratch and the
        BatchNorm workspace: allocated once per train plan, rewritten from the live weights at every step."""
        if self._train_bufs is not None and self._train_bufs["dev"] == dev:
            return self._train_bufs
        lib = N.lib()
        f32 = dict(device=dev, dtype=torch.float32)
        fwd, bwd, wmax, cmax = {}, {}, 1, 1
        for i, st in enumerate(tplan.steps):
            if st.kind == "conv":
                Cout, Cg, kh, kw = st.p["wshape"]
                g = st.p["groups"]
                fwd[i] = torch.empty(lib.ap_conv2d_packed_elems(Cout, Cg, kh, kw, g), **f32)
                bwd[i] = torch.empty(lib.ap_conv2d_packed_elems(g * Cg, Cout // g, kh, kw, g), **f32)
                wmax = max(wmax, Cout * Cg * kh * kw)
            elif st.kind == "bn":
                cmax = max(cmax, st.out.C)
        self._train_bufs = dict(dev=dev, fwd=fwd, bwd=bwd, flip=torch.empty(wmax, **f32),
                                bn_ws=torch.empty(lib.ap_bn2d_train_workspace_bytes(cmax), device=dev, dtype=torch.uint8))
        return self._train_bufs

    def _run_train(self, x, tplan, keep, drop=None):
        """-> (scores, (every buffer of the plan, {bn step: its [2][C] batch statistics}, the dropout stream) or None).  Updates running_mean /
        running_var in place (the kernels do) and increments num_batches_tracked, as nn.BatchNorm2d does (also under no_grad).  The
        counters are int64 bookkeeping and move by one fused torch call per step, the only torch operator in it; a
        BatchNorm(momentum=None) additionally reads its counter on the host (one device-to-host copy per such layer and step), as
        torch's own module does."""
        if tuple(x.shape[1:]) != self._train_chw:
            raise ValueError(f"expected [B, {self._train_chw}], got {tuple(x.shape)}")
        dev = x.device
        N.use_conv_workspace(dev)
        tr = _TrainRun(self._live_tensors(), self._train_images(tplan, dev), drop)
        out, bufs = self._execute(x, tplan, tr)
        if tr.counters:                                          # num_batches_tracked += 1, every BatchNorm's int64 counter in one
            torch._foreach_add_(tr.counters, 1)                  # fused torch call: the step's only torch operator
        return out, ((bufs, tr.stats, drop) if keep else None)

    # ---- input gradient (SURVEY section 8 f-1 for the spectrogram classifiers) ------------------------------------
    def _prepare_backward(self):
        """Per conv step: the flipped, transposed weights (BatchNorm scale folded in) packed for ap_conv2d_fwd."""
        lib, W, dev = N.lib(), self._dev_weights, self._dev
        packs = {}
        for i, st in enumerate(self.plan.steps):
            if st.kind != "conv":
                continue
            w = W[st.p["wk"]]
            if st.p["sk"]:
                w = w * W[st.p["sk"]].reshape(-1, 1, 1, 1)
            Cout, Cg, kh, kw = w.shape
            g = st.p["groups"]
            # [g][Cout/g][Cin/g][kh][kw] -> [g][Cin/g][Cout/g][kh][kw], taps flipped: conv from Cout to Cin, same groups
            wt = w.reshape(g, Cout // g, Cg, kh, kw).permute(0, 2, 1, 3, 4).flip(3, 4).reshape(g * Cg, Cout // g, kh, kw).contiguous()
            out = torch.empty(lib.ap_conv2d_packed_elems(g * Cg, Cout // g, kh, kw, g), device=dev, dtype=torch.float32)
            N.check(lib.ap_conv2d_pack(N.ptr(wt), None, N.ptr(out), g * Cg, Cout // g, kh, kw, g, N.stream()), "ap_conv2d_pack")
            packs[i] = out
        torch.cuda.synchronize(dev)
        self._bwd_packed = packs

    def _input_grad(self, bufs, dout, keep=None, train=None):
        """Reverse sweep over the plan: every step adds its contribution into the gradient buffers of its inputs.
        ``keep``: a dict that receives every gradient buffer of the sweep ({buf id: [B, C, H, W]}, the layout of ``bufs``) -- for
        tests that check the sweep step by step; the arithmetic does not depend on it.
        ``train`` (a ``_TrainSweep``): the sweep runs that train plan instead -- ``bn`` steps go through ap_bn2d_train_bwd, every conv
        step packs its transposed image from the live weight (ap_conv2d_pack_bwd) and leaves dW (ap_conv2d_wgrad) and db (ap_rowsum) in
        ``train.grads`` for the parameters that want one."""
        if train is None and (getattr(self, "_bwd_packed", None) is None or self._bwd_key is not self._dev_weights):
            self._prepare_backward()
            self._bwd_key = self._dev_weights
        lib, W, st_ = N.lib(), self._dev_weights, N.stream()
        plan = self.plan if train is None else train.plan
        B, dev = dout.shape[0], dout.device
        grads = {}
        if train is not None:
            img = self._train_images(plan, dev)
            wg_bytes = max([lib.ap_conv2d_wgrad_workspace_bytes(B, s.ins[0].C, s.ins[0].H, s.ins[0].W, s.out.C, s.p["kh"], s.p["kw"],
                                                                s.p["stride"], s.p["pad"], s.p["groups"])
                            for s in plan.steps if s.kind == "conv" and s.p["wname"] in train.want] + [0])
            wg_ws = torch.empty(max(wg_bytes, 4), device=dev, dtype=torch.uint8)

        def gbuf(b):
            if b not in grads:
                C_, H_, W_ = plan.buf_shape[b]
                grads[b] = torch.zeros((B, C_, H_, W_), device=dev, dtype=torch.float32)
            return grads[b]

        def acc(src, C_, HW, s_cs, s_co, v):                      # g[v] += src[:, s_co : s_co + C]
            N.check(lib.ap_acc_channels(N.ptr(src), N.ptr(gbuf(v.buf)), B, C_, HW, s_cs, s_co, v.cstride, v.coff, st_),
                    "ap_acc_channels")

        def masked(o, relu):                                     # incoming gradient of a full output, through its ReLU
            dy = gbuf(o.buf)
            if not relu:
                return dy
            out = torch.empty_like(dy)
            N.check(lib.ap_relu_mask(N.ptr(dy), N.ptr(bufs[o.buf]), N.ptr(out), dy.numel(), st_), "ap_relu_mask")
            return out

        o = plan.output
        gbuf(o.buf).copy_(dout.reshape(B, o.C, o.H, o.W))
        for i in range(len(plan.steps) - 1, -1, -1):
            s = plan.steps[i]
            o, p = s.out, s.p
            if o.buf not in grads:                               # nothing downstream used this value
                continue
            if s.kind == "conv":
                v = s.ins[0]
                dy = masked(o, p["relu"])
                if p["res"] is not None:
                    acc(dy, o.C, o.H * o.W, o.C, 0, p["res"])
                k, sd, pad = p["kh"], p["stride"], p["pad"]
                assert p["kh"] == p["kw"] and pad <= k - 1
                packed = None if train is not None else self._bwd_packed[i]
                if train is not None:
                    if p["wname"] in train.want:
                        dW, accum = train.grad_of(p["wname"])
                        N.check(lib.ap_conv2d_wgrad(N.ptr(dy), N.ptr(bufs[v.buf]), N.ptr(dW), wg_ws.data_ptr(), wg_ws.numel(), B, v.C, v.H,
                                                    v.W, o.C, k, k, sd, pad, p["groups"], v.cstride, v.coff, accum, st_), "ap_conv2d_wgrad")
                    if p["bname"] in train.want:
                        db, accum = train.grad_of(p["bname"])
                        N.check(lib.ap_rowsum(N.ptr(dy), None, None, N.ptr(db), B, o.C, o.H * o.W, 0, 1.0, accum, st_), "ap_rowsum")
                    if v.buf == plan.input.buf and not train.want_dx:
                        continue                                 # the first layer: nobody asked for dx
                    Cout, Cg, _, _ = p["wshape"]
                    packed = img["bwd"][i]
                    N.check(lib.ap_conv2d_pack_bwd(N.ptr(train.params[p["wname"]].detach()), N.ptr(packed), N.ptr(img["flip"]), Cout, Cg, k,
                                                   k, p["groups"], st_), "ap_conv2d_pack_bwd")
                src, Hs, Ws = dy, o.H, o.W
                if sd > 1:
                    Hs = (o.H - 1) * sd + 1 + (v.H + 2 * pad - k) % sd
                    Ws = (o.W - 1) * sd + 1 + (v.W + 2 * pad - k) % sd
                    src = torch.empty((B, o.C, Hs, Ws), device=dev, dtype=torch.float32)
                    N.check(lib.ap_zero_insert2d(N.ptr(dy), N.ptr(src), B * o.C, o.H, o.W, Hs, Ws, sd, st_), "ap_zero_insert2d")
                tmp = torch.empty((B, v.C, v.H, v.W), device=dev, dtype=torch.float32)
                assert Hs + 2 * (k - 1 - pad) - k + 1 == v.H and Ws + 2 * (k - 1 - pad) - k + 1 == v.W
                N.check(lib.ap_conv2d_fwd(N.ptr(src), N.ptr(packed), None, None, N.ptr(tmp), B, o.C, Hs, Ws, v.C, k, k,
                                          1, k - 1 - pad, p["groups"], self._conv_flags, o.C, 0, st_), "ap_conv2d_fwd")
                acc(tmp, v.C, v.H * v.W, v.C, 0, v)
            elif s.kind == "bn":
                v = s.ins[0]
                assert o.full
                dg = train.grad_of(p["wname"])[0] if p["wname"] in train.want else None
                db = train.grad_of(p["bname"])[0] if p["bname"] in train.want else None
                want = v.buf != plan.input.buf or train.want_dx  # a BatchNorm on the input itself: dx only if somebody asked
                tmp = torch.empty((B, o.C, o.H, o.W), device=dev, dtype=torch.float32) if want else None
                N.check(lib.ap_bn2d_train_bwd(N.ptr(bufs[v.buf]), N.ptr(bufs[o.buf]), N.ptr(gbuf(o.buf)), N.ptr(train.params[p["wname"]].detach()),
                                              N.ptr(train.stats[i]), N.ptr(tmp), N.ptr(dg), N.ptr(db), img["bn_ws"].data_ptr(),
                                              img["bn_ws"].numel(), B, o.C, o.H * o.W, v.cstride, v.coff, int(p["relu"]), st_),
                        "ap_bn2d_train_bwd")
                if want:
                    acc(tmp, o.C, o.H * o.W, o.C, 0, v)
            elif s.kind == "drop":                               # the forward's call on the cotangent: the same mask, the same scale
                v = s.ins[0]
                tmp = torch.empty((B, o.C, o.H, o.W), device=dev, dtype=torch.float32)
                N.check(lib.ap_dropout(N.ptr(gbuf(o.buf)), N.ptr(tmp), B, o.C * o.H * o.W, p["p"], train.drop["seed"], p["draw"],
                                       train.drop["offset"], st_), "ap_dropout")
                acc(tmp, o.C, o.H * o.W, o.C, 0, v)
            elif s.kind == "affine":
                v = s.ins[0]
                dy = masked(o, p["relu"])
                if p["sk"]:
                    tmp = torch.empty_like(dy)
                    zero = self._zeros(o.C, dev)
                    N.check(lib.ap_affine_nchw(N.ptr(dy), N.ptr(W[p["sk"]]), N.ptr(zero), N.ptr(tmp), B, o.C, o.H * o.W, o.C, 0, 0,
                                               st_), "ap_affine_nchw")
                    dy = tmp
                acc(dy, o.C, o.H * o.W, o.C, 0, v)
            elif s.kind == "add":
                dy = masked(o, p["relu"])
                for v in s.ins:
                    acc(dy, o.C, o.H * o.W, o.C, 0, v)
            elif s.kind == "copy":
                v = s.ins[0]
                acc(gbuf(o.buf), v.C, v.H * v.W, o.cstride, o.coff, v)
            elif s.kind == "pool":
                v = s.ins[0]
                assert v.full and o.full
                tmp = torch.empty((B, v.C, v.H, v.W), device=dev, dtype=torch.float32)
                N.check(lib.ap_pool2d_bwd(N.ptr(bufs[v.buf]), N.ptr(gbuf(o.buf)), N.ptr(tmp), B * v.C, v.H, v.W, p["k"], p["stride"],
                                          p["pad"], int(p["is_max"]), st_), "ap_pool2d_bwd")
                acc(tmp, v.C, v.H * v.W, v.C, 0, v)
        dx = gbuf(plan.input.buf)
        if keep is not None:
            keep.update(grads)
        return dx

    def _zeros(self, n, dev):
        z = getattr(self, "_zero_vec", None)
        if z is None or z.numel() < n or z.device != dev:
            self._zero_vec = z = torch.zeros(max(n, 4096), device=dev)
        return z
