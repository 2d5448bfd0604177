"""The loss head of the classifiers' training loop on the HIP library (``csrc/ap_loss.hip``): what
``train_speech_commands.py:131-163`` runs between ``model(inputs)`` and ``optimizer.step()``.

``cross_entropy`` / ``CrossEntropyLoss`` (``nn.CrossEntropyLoss()`` with its default arguments), ``nll_loss`` (M5's loop) and
``mixup_cross_entropy_loss`` (``mixup.py:17-29``) are autograd functions: the forward is ONE ``ap_class_loss`` call that also leaves
d loss / d input, the backward multiplies that by the upstream cotangent, read on the device (``ap_scale_by_scalar``).  With
``return_stats=True`` the same call also returns the predictions and the count of correct ones as device tensors; nothing here
synchronises with the host.  ``mixup`` has the reference's signature and host draws (``np.random.beta`` then
``np.random.permutation``) and mixes on the device.  There is no CPU path: CPU tensors raise ``NativeError``.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _native as N

__all__ = ["cross_entropy", "CrossEntropyLoss", "nll_loss", "mixup_cross_entropy_loss", "mixup", "mixup_with"]

MAX_CLASSES, MAX_BATCH = 4096, 65535


def _scores(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise N.NativeError(f"audiopure_amd.losses: {what} must be a HIP device tensor; there is no CPU path")
    if t.dim() != 2 or t.dtype != torch.float32:
        raise ValueError(f"audiopure_amd.losses: {what} must be float32 [B, K], got {t.dtype} {tuple(t.shape)}")
    return t


def _labels(t, B, dev, what="target"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise N.NativeError(f"audiopure_amd.losses: {what} must be a HIP device tensor; there is no CPU path")
    if t.dtype != torch.int64 or t.dim() != 1 or t.shape[0] != B or t.device != dev:
        raise ValueError(f"audiopure_amd.losses: {what} must be int64 [{B}] on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t.contiguous()


def _iptr(t):
    return None if t is None else t.data_ptr()


def _device(dev):
    """the tensor's device current for the launch (streams and allocations bind to it); nothing to enter where it already is"""
    import contextlib
    return contextlib.nullcontext() if dev.index == torch.cuda.current_device() else torch.cuda.device(dev)


class _ClassLoss(torch.autograd.Function):
    """loss (and pred, n_correct) of one ``ap_class_loss`` launch pair; din is kept for the backward."""

    @staticmethod
    def forward(ctx, scores, mode, labels, soft, stats, factor):
        B, K = scores.shape
        dev = scores.device
        x = scores.detach().contiguous()
        with _device(dev):
            fbuf = torch.empty(B + 1, device=dev, dtype=torch.float32)           # the row losses, then the loss
            din = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            ibuf = torch.empty(B + 1, device=dev, dtype=torch.int64) if stats else None      # pred, then n_correct
            count = stats and labels is not None
            lib, st = N.lib(), N.stream()
            N.check(lib.ap_class_loss(x.data_ptr(), _iptr(labels), _iptr(soft), mode, fbuf.data_ptr(), fbuf.data_ptr() + 4 * B, _iptr(din),
                                      _iptr(ibuf), ibuf.data_ptr() + 8 * B if count else None, B, K, st), "ap_class_loss")
            loss = fbuf[B]
            if factor != 1.0:                                    # size_average=False: the sum over the batch
                N.check(lib.ap_scale_by_scalar(loss.data_ptr(), None, factor, loss.data_ptr(), 1, st), "ap_scale_by_scalar")
        ctx.din, ctx.factor = din, factor
        if not stats:
            return loss
        pred = ibuf[:B]
        ctx.mark_non_differentiable(pred)
        if not count:
            return loss, pred
        n_correct = ibuf[B]
        ctx.mark_non_differentiable(n_correct)
        return loss, pred, n_correct

    @staticmethod
    def backward(ctx, g, *unused):
        if torch.is_grad_enabled():
            raise NotImplementedError("audiopure_amd.losses: no double backward through the native loss (create_graph=True)")
        din = ctx.din
        g = g.detach()
        if g.dtype != torch.float32 or not g.is_cuda:
            raise N.NativeError("audiopure_amd.losses: the loss's cotangent must be a float32 device scalar")
        with _device(din.device):
            out = torch.empty_like(din)
            N.check(N.lib().ap_scale_by_scalar(din.data_ptr(), g.data_ptr(), ctx.factor, out.data_ptr(), din.numel(), N.stream()),
                    "ap_scale_by_scalar")
        return out, None, None, None, None, None


def _check_shape(B, K):
    if not (1 <= K <= MAX_CLASSES and 1 <= B <= MAX_BATCH):
        raise ValueError(f"audiopure_amd.losses: [B, K] = [{B}, {K}] outside [1..{MAX_BATCH}, 1..{MAX_CLASSES}]")


def cross_entropy(logits, target, return_stats=False):
    """``F.cross_entropy(logits, target)`` with its default arguments (mean over the batch; no ignore_index, weights or label
    smoothing).  ``return_stats=True`` -> (loss, pred int64 [B], n_correct int64 scalar), all on the device."""
    x = _scores(logits, "logits")
    _check_shape(*x.shape)
    return _ClassLoss.apply(x, 0, _labels(target, x.shape[0], x.device), None, bool(return_stats), 1.0)


def nll_loss(logprobs, target, return_stats=False):
    """``F.nll_loss(logprobs, target)`` with its default arguments, on log-probabilities [B, K] (M5's loop)."""
    x = _scores(logprobs, "logprobs")
    _check_shape(*x.shape)
    return _ClassLoss.apply(x, 2, _labels(target, x.shape[0], x.device), None, bool(return_stats), 1.0)


def mixup_cross_entropy_loss(input, target, size_average=True, labels=None, return_stats=False):
    """``mixup.py:17-29``: -sum(log(softmax(input).clamp(1e-5, 1)) * target), divided by the batch size unless ``size_average=False``.
    ``labels`` (int64 [B], optional) are the un-mixed targets the loop counts the correct predictions against
    (``train_speech_commands.py:160-163``); with ``return_stats=True`` -> (loss, pred[, n_correct when labels are given])."""
    x = _scores(input, "input")
    q = _scores(target, "target")
    if x.shape != q.shape or x.device != q.device:
        raise ValueError(f"audiopure_amd.losses: input {tuple(x.shape)} and target {tuple(q.shape)} differ")
    _check_shape(*x.shape)
    lab = None if labels is None else _labels(labels, x.shape[0], x.device, "labels")
    return _ClassLoss.apply(x, 1, lab, q.detach().contiguous(), bool(return_stats), 1.0 if size_average else float(x.shape[0]))


class CrossEntropyLoss(nn.Module):
    """Namesake of ``nn.CrossEntropyLoss()`` for the loop's ``criterion``: the default arguments only."""

    def __init__(self, weight=None, size_average=None, ignore_index=-100, reduce=None, reduction="mean", label_smoothing=0.0):
        super().__init__()
        if (weight is not None or size_average is not None or ignore_index != -100 or reduce is not None or reduction != "mean"
                or label_smoothing != 0.0):
            raise ValueError("audiopure_amd.losses.CrossEntropyLoss serves nn.CrossEntropyLoss()'s default arguments only "
                             "(no weight, ignore_index, reduction other than 'mean' or label smoothing)")

    def forward(self, input, target):
        return cross_entropy(input, target)


def mixup_with(inputs, targets, num_classes, weight, index):
    """The device half of ``mixup``: inputs [B, ...] float32 and targets int64 [B] on the device, ``weight`` float32 [B] and ``index``
    int64 [B] (a permutation of the batch) as host arrays -> (mixed inputs, soft targets [B, num_classes])."""
    if not (isinstance(inputs, torch.Tensor) and inputs.is_cuda and isinstance(targets, torch.Tensor) and targets.is_cuda):
        raise N.NativeError("audiopure_amd.losses.mixup: inputs and targets must be HIP device tensors; there is no CPU path")
    B = inputs.shape[0]
    weight = np.ascontiguousarray(weight, dtype=np.float32).reshape(-1)
    index = np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
    if weight.shape[0] != B or index.shape[0] != B:
        raise ValueError(f"audiopure_amd.losses.mixup: {B} samples, {weight.shape[0]} weights, {index.shape[0]} indices")
    if B < 1 or B > MAX_BATCH or not 1 <= num_classes <= MAX_CLASSES or inputs.numel() == 0:
        raise ValueError(f"audiopure_amd.losses.mixup: B = {B}, num_classes = {num_classes} or an empty sample")
    if index.min() < 0 or index.max() >= B:
        raise ValueError("audiopure_amd.losses.mixup: index outside [0, B)")
    if inputs.dtype != torch.float32:
        raise ValueError(f"audiopure_amd.losses.mixup: inputs must be float32, got {inputs.dtype}")
    dev = inputs.device
    y = _labels(targets, B, dev, "targets")
    x = inputs.detach().contiguous()
    with _device(dev):
        w = torch.from_numpy(weight).to(dev)
        idx = torch.from_numpy(index).to(dev)
        out = torch.empty_like(x)
        soft = torch.empty((B, num_classes), device=dev, dtype=torch.float32)
        lib = N.lib()
        N.check(lib.ap_mixup_rows(N.ptr(x), idx.data_ptr(), N.ptr(w), N.ptr(out), B, x.numel() // B, N.stream()), "ap_mixup_rows")
        N.check(lib.ap_mixup_targets(y.data_ptr(), idx.data_ptr(), N.ptr(w), N.ptr(soft), B, num_classes, N.stream()), "ap_mixup_targets")
    return out, soft


def mixup(inputs, targets, num_classes, alpha=2):
    """``mixup.py:40-52`` on device tensors.  The draws are the reference's, on the host and in its order -- ``np.random.beta(alpha,
    alpha, B)`` then ``np.random.permutation(B)`` -- so ``np.random.seed`` reproduces its batches; the weights are rounded to float32
    as ``torch.Tensor(...)`` rounds them.  A label outside [0, num_classes) leaves its row of soft targets NaN (the kernel reads
    nothing out of bounds; checking would be a host read)."""
    if not (isinstance(inputs, torch.Tensor) and inputs.is_cuda and isinstance(targets, torch.Tensor) and targets.is_cuda):
        raise N.NativeError("audiopure_amd.losses.mixup: inputs and targets must be HIP device tensors; there is no CPU path")
    s = inputs.shape[0]
    weight = np.random.beta(alpha, alpha, s).astype(np.float32)
    index = np.random.permutation(s)
    return mixup_with(inputs, targets, num_classes, weight, index)
