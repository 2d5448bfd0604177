"""Native optimizer step: ``Adam``, ``AdamW`` and ``SGD`` as drop-in namesakes of ``torch.optim``'s, the EMA of the parameters fused
into the same pass, and the gradient norm as one device double (``csrc/ap_optim.hip``).

The reference's trainers build ``torch.optim.Adam(net.parameters(), lr=..., weight_decay=...)`` (DiffWave_Unconditional/train.py:79,
M5/train.py:51, RCNN_KWS/train.py:80, train_speech_commands.py:99), ``SGD(momentum=0.9, weight_decay=...)``
(train_speech_commands.py:97) and ``AdamW`` (improved_diffusion/train_util.py:82); the one-line change in each is the import.

Only ``step()`` is native.  ``param_groups``, ``state`` (torch's keys: ``step`` as torch's CPU float32 scalar tensor, ``exp_avg``,
``exp_avg_sq``, ``momentum_buffer``), ``state_dict()`` / ``load_state_dict()`` and ``zero_grad()`` are ``torch.optim.Optimizer``'s, so
lr schedulers work unchanged (``lr`` is read at every step) and a ``state_dict`` moves both ways between a native optimizer and its
torch namesake.  One launch set per param group; a step copies nothing to the device, allocates nothing after the first one and
never synchronises.  There is no CPU path and no fall-back: what the kernel does not serve is refused with a message that says so.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
from torch.optim import Optimizer

from . import _native as N

__all__ = ["Adam", "AdamW", "SGD", "update_ema"]

_REFUSED = "audiopure_amd.optim.{}: {} is not served by the native step (use torch.optim.{} for it)"


def _check_param(p, who):
    ok = isinstance(p, torch.Tensor) and not p.is_sparse and p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()
    if not ok:
        raise N.NativeError(f"{who}: every parameter must be a contiguous float32 tensor on a HIP device (there is no CPU path); got "
                            f"{getattr(p, 'dtype', type(p))} on {getattr(p, 'device', '?')}, layout {getattr(p, 'layout', '?')}")


def _check_grad(g, p, who):
    if g.is_sparse:
        raise N.NativeError(f"{who}: sparse gradients are not served by the native step")
    if not g.is_contiguous() or g.dtype != torch.float32 or g.device != p.device or g.numel() != p.numel():
        raise N.NativeError(f"{who}: a gradient must be a contiguous float32 tensor on its parameter's device; got {g.dtype} on "
                            f"{g.device}, contiguous={g.is_contiguous()}")


_DESC = np.dtype([("param", "<u8"), ("grad", "<u8"), ("state1", "<u8"), ("state2", "<u8"), ("ema", "<u8", (N.AP_OPTIM_MAX_EMA,)),
                  ("n", "<u8"), ("step_size", "<f4"), ("sqrt_bc2", "<f4")])
assert _DESC.itemsize == C.sizeof(N.ApOptimTensor)
_DESC_P = C.POINTER(N.ApOptimTensor)


class _Table:
    """The descriptor array of one launch set (the layout of ApOptimTensor, written by columns): the pointer columns are rewritten
    only when one of them changes -- zero_grad(set_to_none=True) followed by a backward that gets the same blocks back from the
    caching allocator changes none -- the two per-tensor scalars at every step."""

    def __init__(self):
        self.key = None
        self.arr = None

    def fill(self, rows, step_size=None, sqrt_bc2=None):
        """rows: (param, grad, state1, state2, (ema, ...), n) with device pointers (0 for none) -> the ctypes pointer of the table"""
        if rows != self.key:
            arr = np.zeros(len(rows), _DESC)
            cols = list(zip(*rows))
            for name, col in zip(("param", "grad", "state1", "state2"), cols):
                arr[name] = col
            arr["n"] = cols[5]
            if cols[4][0]:
                arr["ema"][:, :len(cols[4][0])] = cols[4]
            self.key, self.arr = rows, arr
        if step_size is not None:
            self.arr["step_size"] = step_size
            self.arr["sqrt_bc2"] = sqrt_bc2
        return self.arr.ctypes.data_as(_DESC_P)


class _Native(Optimizer):
    _NAME = ""

    def __init__(self, params, defaults):
        self._ema_rates = []
        self._ema_of = {}                        # parameter -> its EMA copies, one per tracked rate
        self._tables = {}
        self._slots = {}                         # parameter -> its validated state tensors
        self._step_rows = {}                     # Adam: group index -> the row its parameters' `step` tensors are views of
        self._norm_ws = None
        super().__init__(params, defaults)

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_ema_rates", [])
        self.__dict__.setdefault("_ema_of", {})
        self.__dict__["_tables"] = {}
        self.__dict__["_slots"] = {}             # load_state_dict comes through here: the state tensors are new ones
        self.__dict__["_step_rows"] = {}
        self.__dict__["_norm_ws"] = None

    def add_param_group(self, param_group):
        if getattr(self, "_ema_rates", None):
            raise N.NativeError(f"audiopure_amd.optim.{self._NAME}: add_param_group after track_ema would leave parameters untracked")
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        self._check_group(group)
        for p in group["params"]:
            _check_param(p, f"audiopure_amd.optim.{self._NAME}")
        devs = {p.device for g in self.param_groups for p in g["params"]}
        if len(devs) > 1:
            raise N.NativeError(f"audiopure_amd.optim.{self._NAME}: parameters on several devices {sorted(map(str, devs))}; use one "
                                "optimizer per device")

    def _refuse(self, what):
        raise NotImplementedError(_REFUSED.format(self._NAME, what, self._NAME))

    def _check_group(self, group):
        if isinstance(group["lr"], torch.Tensor):
            self._refuse("a tensor lr")
        for flag in ("amsgrad", "maximize", "capturable", "differentiable", "nesterov"):
            if group.get(flag):
                self._refuse(f"{flag}=True")
        if group.get("dampening", 0) != 0:
            self._refuse("a non-zero dampening")

    # ---- EMA and gradient norm -------------------------------------------------------------------------------------------------
    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def track_ema(self, rate):
        """-> a list of tensors, copies of the parameters (in param_groups order) that every later ``step()`` moves inside the same
        kernel pass: e = rate e + (1 - rate) p_new (nn.py:55-65; parameters without a grad included, as update_ema walks all)."""
        rate = float(rate)
        if not 0.0 <= rate <= 1.0:
            raise ValueError(f"Invalid EMA rate: {rate}")
        if len(self._ema_rates) >= N.AP_OPTIM_MAX_EMA:
            raise N.NativeError(f"audiopure_amd.optim.{self._NAME}: at most {N.AP_OPTIM_MAX_EMA} EMA rates can be tracked")
        copies = [p.detach().clone() for p in self._params()]
        self._ema_rates.append(rate)
        for p, e in zip(self._params(), copies):
            self._ema_of[p] = self._ema_of.get(p, ()) + (e,)
        return copies

    @torch.no_grad()
    def grad_sqnorm(self):
        """-> sum of g^2 over every parameter that has a grad, as a 1-element float64 device tensor; no host read."""
        who = f"audiopure_amd.optim.{self._NAME}.grad_sqnorm"
        params = self._params()
        grads = [p.grad for p in params if p.grad is not None and p.grad.numel()]
        dev = params[0].device
        out = torch.empty(1, dtype=torch.float64, device=dev)
        if not grads:
            return out.zero_()
        for g, p in ((p.grad, p) for p in params if p.grad is not None and p.grad.numel()):
            _check_grad(g, p, who)
        n = len(grads)
        ptrs = (C.c_void_p * n)(*[g.data_ptr() for g in grads])
        sizes = (C.c_uint64 * n)(*[g.numel() for g in grads])
        lib = N.lib()
        need = lib.ap_optim_sqnorm_workspace_bytes(sizes, n)
        if self._norm_ws is None or self._norm_ws.numel() * 8 < need or self._norm_ws.device != dev:
            self._norm_ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            N.check(lib.ap_optim_sqnorm(ptrs, sizes, n, self._norm_ws.data_ptr(), self._norm_ws.numel() * 8, out.data_ptr(), N.stream()),
                    "ap_optim_sqnorm")
        return out

    def grad_norm(self):
        """The gradient norm of train_util.py:254-258 as a float: one host read instead of one per parameter."""
        return math.sqrt(self.grad_sqnorm().item())

    # ---- the step ----------------------------------------------------------------------------------------------------------------
    def _rows(self, gi, group):
        """-> (rows for _Table.fill, step_size and sqrt_bc2 per row or None, the tensors the launch writes); initialises and
        advances torch's per-parameter state"""
        raise NotImplementedError

    def _hyper(self, group):
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            if not group["params"]:
                continue
            with torch.cuda.device(group["params"][0].device):
                rows, step_size, sqrt_bc2, written = self._rows(gi, group)
                hyper = self._hyper(group)
                hyper.n_ema = len(self._ema_rates)
                for k, r in enumerate(self._ema_rates):
                    hyper.ema_rate[k] = r
                if rows:
                    table = self._tables.setdefault(gi, _Table()).fill(rows, step_size, sqrt_bc2)
                    N.check(N.lib().ap_optim_step(table, len(rows), C.byref(hyper), N.stream()), "ap_optim_step")
            if written:
                # the models key their device images on (_version, data_ptr): a raw-pointer write must count as a write
                torch._C._increment_version(written)
        return loss


def _adam_init(self, params, lr, betas, eps, weight_decay, amsgrad, foreach, maximize, capturable, differentiable, fused, decoupled):
    if not isinstance(lr, torch.Tensor) and not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
    if not 0.0 <= weight_decay:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")
    if isinstance(betas[0], torch.Tensor) or isinstance(betas[1], torch.Tensor):
        raise NotImplementedError(_REFUSED.format(self._NAME, "a tensor beta", self._NAME))
    # foreach / fused choose between torch's own implementations: accepted and ignored (recorded as None, so that a state_dict loaded
    # into this optimizer keeps `step` on the CPU, torch's default layout)
    defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                    capturable=capturable, differentiable=differentiable, fused=None, decoupled_weight_decay=decoupled)
    _Native.__init__(self, params, defaults)


class Adam(_Native):
    """torch.optim.Adam (coupled weight decay unless ``decoupled_weight_decay``), the step on ap_optim_step."""
    _NAME = "Adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        _adam_init(self, params, lr, betas, eps, weight_decay, amsgrad, foreach, maximize, capturable, differentiable, fused,
                   decoupled_weight_decay)

    def _hyper(self, group):
        b1, b2 = group["betas"]
        kind = N.AP_OPTIM_ADAMW if group.get("decoupled_weight_decay") else N.AP_OPTIM_ADAM
        return N.ApOptimHyper(kind=kind, lr=group["lr"], beta1=b1, beta2=b2, eps=group["eps"], weight_decay=group["weight_decay"])

    def _state_of(self, p):
        """torch's lazily initialised state of one parameter: `step` a CPU float32 scalar tensor (which the first step() replaces by
        a view of the group's row of counts, `_step_row`), the two moments zeros like p"""
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _step_row(self, gi, group):
        """-> (one CPU float32 row holding the `step` of every parameter of the group, {parameter: its index}).  Each state's `step`
        is a 0-dim view of its entry -- still torch's CPU float32 scalar tensor to every reader -- so a step advances all counts
        with one operator and reads them with one tolist() instead of an add and an item() per parameter."""
        held = self._step_rows.get(gi)
        params = group["params"]
        if held is None or len(held[1]) != len(params):
            held = self._step_rows[gi] = (torch.zeros(len(params), dtype=torch.float32), {p: i for i, p in enumerate(params)}, {})
            for p in params:
                self._slots.pop(p, None)         # re-attached, with the counts they hold now, at their next step
        return held

    def _rows(self, gi, group):
        who = f"audiopure_amd.optim.{self._NAME}.step"
        lr = float(group["lr"])
        b1, b2 = group["betas"]
        f32, state, slots, emas = torch.float32, self.state, self._slots, self._ema_of
        row, pos, masks = self._step_row(gi, group)
        rows, written, live = [], [], []
        for p in group["params"]:
            g = p.grad
            if g is None and not emas:
                continue
            n = p.numel()
            if n == 0:
                continue
            ema = ()
            if emas:
                copies = emas[p]
                ema = tuple(e.data_ptr() for e in copies)
                written.extend(copies)
            if g is None:                        # no grad: `step` and the state stay, the EMA copies move
                rows.append((p.data_ptr(), 0, 0, 0, ema, n))
                live.append(-1)
                continue
            if g.dtype is not f32 or g.is_sparse or not g.is_contiguous() or g.numel() != n or g.device != p.device:
                _check_grad(g, p, who)
            st = state[p]
            slot = slots.get(p)
            if slot is None or st.get("exp_avg") is not slot[0] or st.get("exp_avg_sq") is not slot[1] or st.get("step") is not slot[2]:
                st = self._state_of(p)
                i = pos.get(p)
                if i is None:                    # the group's parameter list was edited in place: start the row over
                    del self._step_rows[gi]
                    return self._rows(gi, group)
                row[i] = float(st["step"])       # a loaded count moves into the row; the state's `step` becomes the view of it
                st["step"] = row[i]
                slot = slots[p] = (st["exp_avg"], st["exp_avg_sq"], st["step"], i)
                N.ptr(slot[0])                   # contiguous fp32 on the current device: checked once per state tensor
                N.ptr(slot[1])
                if slot[0].numel() != n or slot[1].numel() != n:
                    raise N.NativeError(f"{who}: a state tensor's size differs from its parameter's")
            m, v = slot[0], slot[1]
            rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ema, n))
            live.append(slot[3])
            written += (p, m, v)
        stepped = tuple(i for i in live if i >= 0)
        if not stepped:
            return rows, None, None, written
        if len(stepped) == len(pos):
            row += 1
        else:                                    # some parameters have no grad: their counts stay
            mask = masks.get(stepped)
            if mask is None:
                masks.clear()
                mask = masks[stepped] = torch.zeros_like(row)
                mask[list(stepped)] = 1.0
            row += mask
        counts = row.tolist()
        scal = {}                                # step count -> (lr / bc1, sqrt(bc2)) in double; the table rounds them to fp32
        step_size, sqrt_bc2 = [], []
        for i in live:
            if i < 0:
                step_size.append(0.0)
                sqrt_bc2.append(1.0)
                continue
            t = counts[i]
            c = scal.get(t)
            if c is None:
                c = scal[t] = (lr / (1 - b1 ** t), (1 - b2 ** t) ** 0.5)
            step_size.append(c[0])
            sqrt_bc2.append(c[1])
        return rows, step_size, sqrt_bc2, written


class AdamW(Adam):
    """torch.optim.AdamW: Adam with decoupled weight decay (as in torch, where AdamW is Adam with ``decoupled_weight_decay=True``)."""
    _NAME = "AdamW"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None):
        _adam_init(self, params, lr, betas, eps, weight_decay, amsgrad, foreach, maximize, capturable, differentiable, fused, True)


class SGD(_Native):
    """torch.optim.SGD with dampening 0 and no Nesterov momentum, the step on ap_optim_step."""
    _NAME = "SGD"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        if not isinstance(lr, torch.Tensor) and lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if isinstance(weight_decay, torch.Tensor):
            raise NotImplementedError(_REFUSED.format(self._NAME, "a tensor weight_decay", self._NAME))
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize,
                        foreach=None, differentiable=differentiable, fused=None)
        super().__init__(params, defaults)

    def _hyper(self, group):
        return N.ApOptimHyper(kind=N.AP_OPTIM_SGD, lr=group["lr"], weight_decay=group["weight_decay"], momentum=group["momentum"])

    def _state_of(self, p):
        """torch's state of one parameter under momentum: `momentum_buffer` (torch's first step clones the gradient into it; zeros
        and mu 0 + g give the same values)"""
        st = self.state[p]
        if st.get("momentum_buffer") is None:
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _rows(self, gi, group):
        who = "audiopure_amd.optim.SGD.step"
        mu = group["momentum"]
        f32, state, slots, emas = torch.float32, self.state, self._slots, self._ema_of
        rows, written = [], []
        for p in group["params"]:
            g = p.grad
            if g is None and not emas:
                continue
            n = p.numel()
            if n == 0:
                continue
            ema = ()
            if emas:
                copies = emas[p]
                ema = tuple(e.data_ptr() for e in copies)
                written.extend(copies)
            if g is None:
                rows.append((p.data_ptr(), 0, 0, 0, ema, n))
                continue
            if g.dtype is not f32 or g.is_sparse or not g.is_contiguous() or g.numel() != n or g.device != p.device:
                _check_grad(g, p, who)
            buf = 0
            written.append(p)
            if mu != 0:
                b = slots.get(p)
                if b is None or state[p].get("momentum_buffer") is not b:
                    b = slots[p] = self._state_of(p)["momentum_buffer"]
                    N.ptr(b)                     # contiguous fp32 on the current device: checked once per state tensor
                    if b.numel() != n:
                        raise N.NativeError(f"{who}: a momentum buffer's size differs from its parameter's")
                buf = b.data_ptr()
                written.append(b)
            rows.append((p.data_ptr(), g.data_ptr(), buf, 0, ema, n))
        return rows, None, None, written


@torch.no_grad()
def update_ema(target_params, source_params, rate=0.99):
    """The reference's ``update_ema`` (improved_diffusion/nn.py:55-65): targ = rate targ + (1 - rate) src for every pair, as one
    launch set of the EMA-only kind instead of two operators per parameter."""
    pairs = [(t, s) for t, s in zip(target_params, source_params) if t.numel()]
    if not pairs:
        return
    rows = []
    for t, s in pairs:
        if t.numel() != s.numel() or t.device != s.device:
            raise N.NativeError("audiopure_amd.optim.update_ema: a target and its source differ in size or device")
        rows.append((N.ptr(s.detach()), 0, 0, 0, (N.ptr(t.detach()),), t.numel()))
    hyper = N.ApOptimHyper(kind=N.AP_OPTIM_EMA_ONLY, n_ema=1)
    hyper.ema_rate[0] = float(rate)
    with torch.cuda.device(pairs[0][0].device):
        N.check(N.lib().ap_optim_step(_Table().fill(rows), len(rows), C.byref(hyper), N.stream()), "ap_optim_step (update_ema)")
    torch._C._increment_version([t.detach() for t, _ in pairs])
