"""float64 restatement of the loss head (audiopure_amd/csrc/ap_loss.hip, audiopure_amd/losses.py): the three modes of ``ap_class_loss``
with their gradients, ``pred`` and ``n_correct``, and the two mixup expressions.  Test infrastructure only: test_loss_restate_cpu.py
pins it to torch's own ``F.cross_entropy`` / ``F.nll_loss`` + autograd and to the reference's ``mixup_cross_entropy_loss`` / ``mixup``
(tests/golden/golden_loss_v1.npz, written by tests/golden/make_golden_loss.py) and asserts the conditions the bounds rest on;
test_gpu_loss.py pins the kernels to it.

    python tests/loss_restate.py        # re-measure the float32 errors of every case (CPU, seconds)

Cases: B in {1, 5, 257} x K in {1, 2, 12, 64, 65, 200} x logits uniform in +-4 and in +-100 (a softmax without the maximum subtracted
overflows there, and the clamp of mode 1 is live).  Where B >= 2 and K >= 2, row 1 holds a deliberate exact tie of its two largest
scores (the lowest index wins); the extra case "bad" (B = 5, K = 12) has one label outside [0, K).  The seed of a case is the first of
0, 1, ... at which the float64 restatement alone meets the conditions: every non-tie row's two largest scores are more than 1e-4 of the
row's largest magnitude apart, and in mode 1 no p_i lies within a relative 1e-3 of the clamp's 1e-5.  No case is set aside.

Bounds (the convention of 3.12): 4 x the error of float32 torch on the CPU against this restatement, per tensor as
max |d| / max |ref|, maximised over modes and cases:
    loss            LOSS_F32_ERR
    d loss / d in   DIN_F32_ERR
"""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from audiopure_amd import synth  # noqa: E402

BATCHES, CLASSES, RANGES = (1, 5, 257), (1, 2, 12, 64, 65, 200), (4.0, 100.0)
CASES = [(B, K, r, False) for B in BATCHES for K in CLASSES for r in RANGES] + [(5, 12, 4.0, True)]
MODES = (0, 1, 2)                                   # nn.CrossEntropyLoss(), mixup_cross_entropy_loss, F.nll_loss
TIE_ROW = 1
CLAMP = 1e-5

LOSS_F32_ERR = 1.9e-7
DIN_F32_ERR = 3.4e-7
LOSS_BOUND = 4 * LOSS_F32_ERR
DIN_BOUND = 4 * DIN_F32_ERR


def case_id(c):
    B, K, r, bad = c
    return f"B{B}-K{K}-r{int(r)}" + ("-bad" if bad else "")


def _draw(c, seed):
    """-> (logits float32 [B, K], labels int64 [B], soft targets float32 [B, K]) of one case at one seed"""
    B, K, r, bad = c
    z = synth.uniform("loss/z/" + case_id(c), (B, K), seed, -r, r).astype(np.float32)
    if B > TIE_ROW and K >= 2:                       # an exact tie of the row's two largest scores, the lower index second in memory order
        j = np.argsort(z[TIE_ROW])[-2:]
        z[TIE_ROW, j] = z[TIE_ROW, j].max()
    # labels: an odd row's is its own prediction (row 1's: the tie's lower index), an even row's the class after it -- every case has
    # right and wrong predictions, and row 0 is wrong: at +-100 a rightly predicted row's loss and din row underflow in float32, and
    # with nothing else in the batch (B = 1) the rounding of a 1e-21 would be measured against itself
    y = (z.argmax(1).astype(np.int64) + (np.arange(B) % 2 == 0)) % K
    if bad:
        y[2] = K
    w = synth.uniform("loss/w/" + case_id(c), (B,), seed, 0.0, 1.0).astype(np.float32)
    y_ok = np.where((y >= 0) & (y < K), y, 0)
    soft = mixup_targets(y_ok, np.roll(np.arange(B), 1), w, K)
    return z, y, soft


def softmax64(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def conditions(c, seed):
    """-> (smallest top-two gap of a non-tie row over the row's largest magnitude, smallest relative distance of a p_i from the clamp)"""
    z, _, _ = _draw(c, seed)
    B, K = z.shape
    gap = float("inf")
    if K >= 2:
        top = np.sort(z.astype(np.float64), 1)[:, -2:]
        g = (top[:, 1] - top[:, 0]) / np.abs(z).max(1)
        rows = [b for b in range(B) if not (b == TIE_ROW and B > TIE_ROW)]
        gap = float(g[rows].min()) if rows else float("inf")
    p = softmax64(z)
    return gap, float(np.abs(p / CLAMP - 1.0).min())


@functools.lru_cache(maxsize=None)
def seed_of(c):
    for seed in range(64):
        gap, clamp = conditions(c, seed)
        if gap > 1e-4 and clamp > 1e-3:
            return seed
    raise AssertionError(f"no seed below 64 meets the conditions of {case_id(c)}")


@functools.lru_cache(maxsize=None)
def case(c):
    """-> (logits float32 [B, K], labels int64 [B], soft float32 [B, K]) as numpy arrays.  Shared by the tests: do not modify."""
    return _draw(c, seed_of(c))


def mode_input(c, mode):
    """what mode `mode` reads: the logits, or (mode 2) their log-softmax rounded to float32"""
    z = case(c)[0]
    if mode != 2:
        return z
    z64 = z.astype(np.float64)
    m = z64.max(1, keepdims=True)
    return (z64 - m - np.log(np.exp(z64 - m).sum(1, keepdims=True))).astype(np.float32)


def class_loss(x, labels, soft, mode):
    """The float64 restatement of ap_class_loss -> dict(rows [B], loss, din [B, K], pred int64 [B], n_correct).  A label outside [0, K)
    makes its row's loss and din row NaN (and the loss with it)."""
    x = np.asarray(x, np.float64)
    B, K = x.shape
    pred = x.argmax(1).astype(np.int64)              # numpy's argmax is the first maximum
    rows, din = np.empty(B), np.empty((B, K))
    ok = None
    if mode != 1 or labels is not None:
        ok = (labels >= 0) & (labels < K)
    if mode == 1:
        p = softmax64(x)
        q = np.asarray(soft, np.float64)
        live = (p >= CLAMP) & (p <= 1.0)
        rows = -(q * np.log(np.clip(p, CLAMP, 1.0))).sum(1)
        din = (-q * live + p * (q * live).sum(1, keepdims=True)) / B
    else:
        ys = np.where(ok, labels, 0)
        onehot = np.zeros((B, K))
        onehot[np.arange(B), ys] = 1.0
        if mode == 0:
            m = x.max(1)
            rows = m + np.log(np.exp(x - m[:, None]).sum(1)) - x[np.arange(B), ys]
            din = (softmax64(x) - onehot) / B
        else:
            rows = -x[np.arange(B), ys]
            din = -onehot / B
        rows = np.where(ok, rows, np.nan)
        din = np.where(ok[:, None], din, np.nan)
    n_correct = None if labels is None else int((pred == labels).sum())
    return dict(rows=rows, loss=rows.sum() / B, din=din, pred=pred, n_correct=n_correct)


@functools.lru_cache(maxsize=None)
def reference(c, mode):
    """The restatement of one case in one mode.  Computed once, shared by the tests, never modified."""
    z, y, soft = case(c)
    return class_loss(mode_input(c, mode), y, soft if mode == 1 else None, mode)


def torch_loss(x, labels, soft, mode, dtype=torch.float32):
    """torch's own operators (mode 1: the expression of mixup.py:17-29) in `dtype` on the CPU with autograd -> dict(loss, din, pred)"""
    xs = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_(True)
    if mode == 0:
        loss = F.cross_entropy(xs, torch.from_numpy(labels))
    elif mode == 2:
        loss = F.nll_loss(xs, torch.from_numpy(labels))
    else:
        lp = torch.log(F.softmax(xs, dim=1).clamp(1e-5, 1))
        loss = -torch.sum(lp * torch.from_numpy(np.asarray(soft)).to(dtype)) / xs.shape[0]
    din, = torch.autograd.grad(loss, xs)
    return dict(loss=loss.detach().numpy(), din=din.numpy(), pred=xs.detach().max(1)[1].numpy())


def rel(a, ref):
    """max |a - ref| / max |ref| in float64 (an exact-zero reference: the absolute figure)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    if a.size == 0:
        return 0.0
    d, s = float(np.abs(a - ref).max()), float(np.abs(ref).max())
    return d / s if s > 0 else d


def mixup_rows(x, index, weight):
    """mixup.py:46-49 as float32 torch computes it on the CPU: fl(fl(w x1) + fl(fl(1 - w) x2)), rows of any shape"""
    x = np.asarray(x, np.float32)
    w = np.asarray(weight, np.float32).reshape((-1,) + (1,) * (x.ndim - 1))
    omw = (np.float32(1.0) - w).astype(np.float32)
    return ((w * x).astype(np.float32) + (omw * x[np.asarray(index)]).astype(np.float32)).astype(np.float32)


def onehot(y, K):
    out = np.zeros((len(y), K), np.float32)
    out[np.arange(len(y)), y] = 1.0
    return out


def mixup_targets(labels, index, weight, K):
    """mixup.py:47,50-51: weight * onehot(y) + (1 - weight) * onehot(y[index]), the same rounding sequence"""
    labels = np.asarray(labels)
    return mixup_rows(onehot(labels, K), index, weight)


def mixup_draws(seed, B, alpha=2):
    """the host draws of mixup.py:43-44 after np.random.seed(seed): (weight as torch.Tensor rounds it, index)"""
    np.random.seed(seed)
    w = np.random.beta(alpha, alpha, B).astype(np.float32)
    return w, np.random.permutation(B)


MIXUP_GOLDEN = [(1, 3), (2, 12), (5, 12)]            # (B, num_classes) of the golden's mixup() runs, inputs [B, 1, 4, 8], seed = B


def mixup_inputs(B, K):
    x = synth.uniform(f"loss/mixup/x/{B}", (B, 1, 4, 8), 0, -3.0, 3.0).astype(np.float32)
    return x, (np.arange(B, dtype=np.int64) * 5 + 1) % K


GOLDEN_FULL = 4096                                   # the golden holds the first this many elements of a gradient


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_loss_v1.npz")))


def measure_f32():
    """float32 torch on the CPU against the restatement -> (loss error, din error), the largest over modes and cases"""
    worst_l = worst_d = 0.0
    for c in CASES:
        if c[3]:
            continue                                 # (torch refuses an out-of-range label)
        z, y, soft = case(c)
        for mode in MODES:
            ref = reference(c, mode)
            got = torch_loss(mode_input(c, mode), y, soft, mode)
            worst_l, worst_d = max(worst_l, rel(got["loss"], ref["loss"])), max(worst_d, rel(got["din"], ref["din"]))
    return worst_l, worst_d


if __name__ == "__main__":
    for c in CASES:
        gap, clamp = conditions(c, seed_of(c))
        print(f"{case_id(c):18s} seed {seed_of(c)}  top-two gap {gap:.3g}  distance from the clamp {clamp:.3g}")
    l, d = measure_f32()
    print(f"LOSS_F32_ERR {l:.2e} (recorded {LOSS_F32_ERR:.2e})   DIN_F32_ERR {d:.2e} (recorded {DIN_F32_ERR:.2e})")
