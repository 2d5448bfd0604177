"""The PGD loop of the reference's adversarial-training scripts on the HIP library (``csrc/ap_attack.hip``): ``pgd`` of
``audio_models/RCNN_KWS/train.py:84-121`` and of ``audio_models/ConvNets_SpeechCommands/adv_train_speech_commands.py:139-183``.

The scripts define ``pgd`` in their own body; they use this one by replacing that definition with
``from audiopure_amd.attacks import pgd`` (the KWS script passes ``transform`` and ``criterion`` by keyword or in its own order
through a two-line wrapper; the ConvNet script passes ``transform=Wave2Spect``).  The loop has no early exit -- it always runs n + 1
forwards and n backwards -- so it is enqueued without a host read: the random start is one ``ap_pgd_init`` launch, and an iteration's
per-sample test, copy, update, projection and box step are one ``ap_pgd_step_linf`` launch (three for ``ap_pgd_step_l2``), where the
scripts index, compare and block on the host once per sample and iteration.  The linf results are the bits of the scripts' loops.

The one documented difference from the scripts: the model's parameters are frozen for the duration (``requires_grad`` off, restored
in a ``finally``), so the backward forms the input gradient only -- ``KWSModel`` takes its input-gradient node, a ``NativeConvNet``
in ``train()`` its train-mode node with no parameter wanting a gradient (no ``ap_conv2d_wgrad``, no ``ap_rowsum``) -- and no
parameter's ``.grad`` is touched, where the scripts' ``pgd`` fills every ``.grad`` and the caller zeroes it.  The model runs in the
mode it is in: in ``train()`` each of the n + 1 forwards moves the BatchNorm running statistics, as in the scripts.

``PgdRun`` holds one run's device buffers and the kernel calls on them.  ``stage_1`` is stage 1 of the white-box attack
(``robustness_eval/white_box_attack.py:362-471``) on it, with the checkout's own model, EOT and criterion calls
(``dropin/robustness_eval/white_box_attack.py``: ``NativeStage1AudioAttack``).  There is no CPU path.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn as nn

from . import _native as N
from . import losses as L

__all__ = ["pgd", "PgdRun", "stage_1", "stage_1_served"]

MAX_CLASSES, MAX_BATCH = 4096, 65535


class PgdRun:
    """The buffers of one PGD run over rows ``x`` [B, ...] float32 -- ``delta``, ``x_pert``, ``x_adv`` shaped like ``x``, ``found``
    uint8 [B] -- and the kernel calls on them.  Every call is enqueued on the current stream; nothing is read on the host."""

    def __init__(self, x, y, who="audiopure_amd.attacks.pgd"):
        if not (isinstance(x, torch.Tensor) and x.is_cuda and isinstance(y, torch.Tensor) and y.is_cuda):
            raise N.NativeError(f"{who}: x and y must be HIP device tensors; there is no CPU path")
        if x.dtype != torch.float32 or x.dim() < 2 or x.numel() == 0:
            raise ValueError(f"{who}: x must be a non-empty float32 [B, ...], got {x.dtype} {tuple(x.shape)}")
        B = x.shape[0]
        if B > MAX_BATCH or y.dim() != 1 or y.shape[0] != B or y.device != x.device or y.dtype.is_floating_point:
            raise ValueError(f"{who}: y must be an integer [{B}] on {x.device} (B <= {MAX_BATCH}), got {y.dtype} {tuple(y.shape)} on {y.device}")
        self.who, self.B, self.n = who, B, x.numel() // B
        self.x = x.detach().contiguous()
        self.y = y.detach().to(torch.int64).contiguous()
        self.delta, self.x_pert, self.x_adv = (torch.empty_like(self.x) for _ in range(3))
        self.found = torch.zeros(B, device=x.device, dtype=torch.uint8)
        self._ws = None

    def start(self, u=None, eps=0.0):
        """the random start from the uniform draws ``u`` (shaped like x), or with ``u=None`` stage 1's zero start"""
        if u is not None:
            if not (isinstance(u, torch.Tensor) and u.is_cuda):
                raise N.NativeError(f"{self.who}: noise must be a HIP device tensor; there is no CPU path")
            if u.shape != self.x.shape or u.dtype != torch.float32 or u.device != self.x.device:
                raise ValueError(f"{self.who}: noise must be float32 {tuple(self.x.shape)} on {self.x.device}")
            u = u.detach().contiguous()
        N.check(N.lib().ap_pgd_init(N.ptr(self.x), N.ptr(u), N.ptr(self.delta), N.ptr(self.x_pert), float(eps), self.B, self.n, N.stream()),
                "ap_pgd_init")

    def _scores(self, scores):
        s = scores.detach()
        if not s.is_cuda or s.dim() != 2 or s.shape[0] != self.B or not 1 <= s.shape[1] <= MAX_CLASSES or s.dtype != torch.float32:
            raise ValueError(f"{self.who}: the model must give float32 device scores [{self.B}, K <= {MAX_CLASSES}], got {s.dtype} "
                             f"{tuple(s.shape)} on {s.device}")
        return s.contiguous()

    def step(self, scores, g, step, eps, p="linf", targeted=False, last=False):
        """One iteration after the model call: rows that are adversarial now (the argmax of ``scores`` [B, K] against y, taken by the
        kernel) copy the current iterate into ``x_adv``; then the update by ``g`` (the gradient at ``x_pert``) with the signed
        ``step``, projected to ``eps`` (a float, or a float32 device tensor [B] of per-row bounds).  ``last``: no update, and the
        rows never hit take the current iterate."""
        s = self._scores(scores)
        if not last:
            if g.shape != self.x.shape or g.dtype != torch.float32 or g.device != self.x.device:
                raise ValueError(f"{self.who}: the gradient must be float32 {tuple(self.x.shape)} on {self.x.device}, got {g.dtype} "
                                 f"{tuple(g.shape)} on {g.device}")
            g = g.detach().contiguous()
        rows = None
        if isinstance(eps, torch.Tensor):                        # a bound per row
            if not eps.is_cuda:
                raise N.NativeError(f"{self.who}: a per-row eps must be a HIP device tensor; there is no CPU path")
            if eps.dtype != torch.float32 or eps.shape != (self.B,) or eps.device != self.x.device:
                raise ValueError(f"{self.who}: a per-row eps must be float32 [{self.B}] on {self.x.device}, got {eps.dtype} "
                                 f"{tuple(eps.shape)} on {eps.device}")
            rows = eps.detach().contiguous()
        args = (N.ptr(self.x), None if last else N.ptr(g), N.ptr(self.delta), N.ptr(self.x_pert), N.ptr(self.x_adv), self.found.data_ptr(),
                None, N.ptr(s), s.shape[1], self.y.data_ptr(), float(step), N.ptr(rows), 0.0 if rows is not None else float(eps),
                int(bool(targeted)), int(bool(last)))
        lib = N.lib()
        if p == "linf":
            N.check(lib.ap_pgd_step_linf(*args, self.B, self.n, N.stream()), "ap_pgd_step_linf")
        else:
            if self._ws is None:
                self._ws = torch.empty(max(lib.ap_pgd_l2_workspace_bytes(self.B, self.n) // 8, 1), device=self.x.device, dtype=torch.float64)
            N.check(lib.ap_pgd_step_l2(*args, self._ws.data_ptr(), self._ws.numel() * 8, self.B, self.n, N.stream()), "ap_pgd_step_l2")


@contextlib.contextmanager
def _frozen(model):
    """the module's parameters with requires_grad off; every flag is put back on the way out, also when the body raises"""
    params = list(model.parameters()) if isinstance(model, nn.Module) else []
    flags = [q.requires_grad for q in params]
    try:
        for q in params:
            q.requires_grad_(False)
        yield
    finally:
        for q, f in zip(params, flags):
            q.requires_grad_(f)


def _is_default_cross_entropy(criterion):
    if criterion is None or isinstance(criterion, L.CrossEntropyLoss) or criterion is L.cross_entropy:
        return True
    return (type(criterion) is nn.CrossEntropyLoss and criterion.weight is None and criterion.ignore_index == -100
            and criterion.reduction == "mean" and criterion.label_smoothing == 0.0)


def pgd(model, x, y, eps=0.002, alpha=0.0004, n=10, p="linf", *, transform=None, criterion=None, targeted=False, noise=None,
        accumulate=False, return_found=False, check_range=True):
    """``pgd`` of both adversarial-training scripts -> ``x_adv`` shaped like ``x`` ([B, 1, L]); with ``return_found=True`` also the
    bool [B] of the rows that were adversarial at some iteration (the others hold the last iterate).

    ``transform`` is the waveform front-end (``None``: the model takes waveforms).  ``criterion=None``, ``nn.CrossEntropyLoss()`` with
    its default arguments and this package's namesakes run on ``ap_class_loss``; any other callable is called as it is.  ``noise`` are
    the uniform draws of the random start (default ``torch.rand_like(x)``, the scripts' own draw).  ``targeted``: descend the loss
    towards ``y`` and count a row as hit when it is predicted ``y``.  ``accumulate=True`` is RCNN_KWS/train.py's loop to the bit: it
    never zeroes ``delta.grad``, so its update takes the sign of the running sum of the gradients so far (one fp32 add per iteration,
    as autograd's accumulation does); adv_train_speech_commands.py zeroes it (the default).  The scripts' range assertion on ``x`` is the call's ONE host read,
    before the loop; ``check_range=False`` leaves it out."""
    if p not in ("linf", "l2"):
        raise NotImplementedError(f'Unsupported norm: {p}!')
    n = int(n)
    if n < 0:
        raise ValueError(f"audiopure_amd.attacks.pgd: n = {n} < 0")
    run = PgdRun(x, y)                                           # (CPU tensors raise here)
    dev = run.x.device
    with L._device(dev):
        if check_range:
            lo, hi = torch.aminmax(run.x)
            if not bool((hi <= 1) & (lo >= -1)):                 # (a NaN fails it too, as it fails the scripts' assert)
                raise AssertionError("audiopure_amd.attacks.pgd: x must lie in [-1, 1]")
        run.start(torch.rand_like(run.x) if noise is None else noise, eps)
        native_ce = _is_default_cross_entropy(criterion)
        step = -float(alpha) if targeted else float(alpha)
        acc = None
        with _frozen(model):
            for i in range(n + 1):
                xp = run.x_pert.detach().requires_grad_(True)    # a fresh leaf on the iterate's memory: its gradient is d loss / d delta
                scores = model(xp if transform is None else transform(xp))
                if i == n:
                    run.step(scores, None, step, eps, p, targeted, last=True)
                    break
                loss = L.cross_entropy(scores, run.y) if native_ce else criterion(scores, run.y)
                g, = torch.autograd.grad(loss, xp)
                del loss
                acc = g if acc is None or not accumulate else acc.add_(g)
                run.step(scores, acc, step, eps, p, targeted)
    x_adv = run.x_adv.view(x.shape)
    return (x_adv, run.found.bool()) if return_found else x_adv


# what ``stage_1`` reads of an ``AudioAttack`` (white_box_attack.py:280-341; ``eot_model`` only where an EOT size is above 1, and
# ``_targeted`` as ``generate`` leaves it)
STAGE_1_READS = ("model", "criterion", "eps", "norm", "learning_rate_1", "max_iter_1", "_targeted", "eot_attack_size", "eot_defense_size",
                 "eot_model", "verbose")


def stage_1_served(attack, x, y):
    """whether ``stage_1`` serves this call of an ``AudioAttack``: a float32 device batch [B, 1, L] under the linf norm"""
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[1] == 1
            and x.numel() > 0 and isinstance(y, torch.Tensor) and y.is_cuda and attack.norm == 'linf')


def stage_1(attack, x, y):
    """``AudioAttack.stage_1`` (white_box_attack.py:362-471) for the calls ``stage_1_served`` accepts -> (x_adv [B, 1, L], the list
    of per-sample successes).  The calls of ``attack.model``, ``attack.eot_model`` (both EOT branches) and ``attack.criterion`` are the
    checkout's; the per-sample loops, the update, the projection and the final gather are ``ap_pgd_step_linf``: the zero start, the step
    ``-lr`` targeted / ``+lr`` untargeted, a bound per row (the checkout keeps a per-sample list).  The success list is the one host
    read, after the loop.  The results are the checkout's bits."""
    if not stage_1_served(attack, x, y):
        raise N.NativeError("audiopure_amd.attacks.stage_1: needs a float32 HIP device batch [B, 1, L] and norm 'linf'; there is no CPU path")
    batch_size = x.shape[0]
    run = PgdRun(x, y, who="audiopure_amd.attacks.stage_1")
    with L._device(x.device):
        run.start(None)                                          # delta = zeros_like(x)
        epsilon = torch.full((batch_size,), attack.eps, device=x.device, dtype=torch.float32)
        step = -attack.learning_rate_1 if attack._targeted else attack.learning_rate_1
        for i in range(0, attack.max_iter_1 + 1):
            x_pert = run.x_pert.detach().requires_grad_(True)    # a leaf on the iterate: its gradient is delta's
            if attack.eot_defense_size > 1:
                attack.eot_model.EOT_size = attack.eot_defense_size
                attack.eot_model.use_grad = False
                y_pert, _, _, _ = attack.eot_model(x_pert, y)
            else:
                y_pert = attack.model(x_pert)
            if i == attack.max_iter_1:
                run.step(y_pert, None, step, epsilon, 'linf', attack._targeted, last=True)
                break
            if attack.eot_attack_size > 1:
                attack.eot_model.EOT_size = attack.eot_attack_size
                attack.eot_model.use_grad = True
                _, _, grad, _ = attack.eot_model(x_pert, y)
            else:
                loss = attack.criterion(y_pert, y)
                loss.backward()
                grad = x_pert.grad
            run.step(y_pert, grad.data, step, epsilon, 'linf', attack._targeted)
        success_stage_1 = run.found.bool().tolist()              # the one host read
    if attack.verbose:
        for j in range(batch_size):
            if not success_stage_1[j]:
                print("Adversarial attack stage 1 for x_{} was not successful".format(j))
    return run.x_adv, success_stage_1
