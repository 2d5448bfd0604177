"""Restatement of the PGD loops behind audiopure_amd/csrc/ap_attack.hip and audiopure_amd/attacks.py in torch operators, in float32
and float64: the arithmetic of the three kernels (``init``, ``step_linf``, ``step_l2``), and on top of it the three loops -- ``pgd`` of
RCNN_KWS/train.py:84-121, ``pgd`` of adv_train_speech_commands.py:139-183, stage 1 of white_box_attack.py:362-471 -- with the
per-sample Python loops written as ``torch.where``.  Test infrastructure only: test_pgd_restate_cpu.py pins the float32 restatement,
bit for bit, to what the reference's own functions returned (tests/golden/golden_pgd_v1.npz, written by tests/golden/make_golden_pgd.py);
test_gpu_pgd.py pins the kernels and ``attacks.pgd`` to the restatement.

The loops are driven by a SCRIPTED model: its i-th forward returns recorded scores [B, K] and its backward returns a recorded
gradient G_i whatever the cotangent, so the expected outputs depend on no model numerics and are the same bits on any device.

One difference between the two scripts that the restatement keeps: RCNN_KWS/train.py never zeroes ``delta.grad``, so its update takes
the sign of the running SUM of the gradients so far (``accumulate=True``); adv_train_speech_commands.py zeroes it every iteration.
"""
import functools
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_pgd_v1.npz")

EPS, ALPHA, LR = 0.002, 0.0008, 0.0008           # alpha = lr = 0.4 eps: the third step in one direction leaves the ball
K = 6
CASES = {"b1": (1, 1, 2), "b3": (3, 7, 3), "b5": (5, 1031, 4)}       # name -> (B, L, n)


# ---------------------------------------------------------------------------------------------------------
# 1. the scripted model
# ---------------------------------------------------------------------------------------------------------
class _Scripted(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scores, grad):
        ctx.grad = grad
        return scores.clone()

    @staticmethod
    def backward(ctx, g):
        if ctx.grad is None:
            raise RuntimeError("the scripted model has no gradient recorded for this forward")
        return ctx.grad.clone(), None, None


class ScriptedModel(torch.nn.Module):
    """i-th forward -> scores[i] [B, K]; its backward -> grads[i] shaped like the input, whatever the cotangent."""

    def __init__(self, scores, grads):
        super().__init__()
        self.scores, self.grads, self.calls = list(scores), list(grads), 0

    def forward(self, x):
        i = self.calls
        self.calls += 1
        g = self.grads[i].to(device=x.device, dtype=x.dtype).reshape(x.shape) if i < len(self.grads) else None
        return _Scripted.apply(x, self.scores[i].to(device=x.device, dtype=x.dtype), g)


# ---------------------------------------------------------------------------------------------------------
# 2. the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------
def _rows(v, like):
    """a float, or per-row values [B], against rows shaped like `like`"""
    if isinstance(v, torch.Tensor):
        return v.to(like.dtype).reshape((-1,) + (1,) * (like.dim() - 1))
    return v


def box(x, d):
    delta = (x + d).clamp(-1, 1) - x
    return delta, x + delta


def init(x, u, eps):
    """ap_pgd_init -> (delta, x_pert); u None: the zero start"""
    if u is None:
        delta = torch.zeros_like(x)
        return delta, x + delta
    return box(x, eps * (2 * u - 1))


def argmax_rows(scores):
    """Tensor.max's index: the lowest index of the row maximum, a NaN counting as the maximum"""
    return scores.max(1)[1]


def _bookkeep(x_pert, x_adv, found, pred, y, targeted, last):
    hit = (pred == y) if targeted else (pred != y)
    found = found | hit
    copy = (hit | ~found) if last else hit
    shape = (-1,) + (1,) * (x_pert.dim() - 1)
    return torch.where(copy.reshape(shape), x_pert, x_adv), found


def clamp_rows(v, eps):
    """torch.clamp(v, -eps, eps) with a bound per row where eps is a tensor"""
    if isinstance(eps, torch.Tensor):
        e = _rows(eps, v)
        return torch.minimum(torch.maximum(v, -e), e)
    return v.clamp(-eps, eps)


def step_linf(x, g, delta, x_pert, x_adv, found, pred, y, step, eps, targeted=False, last=False):
    """ap_pgd_step_linf -> (delta, x_pert, x_adv, found)"""
    x_adv, found = _bookkeep(x_pert, x_adv, found, pred, y, targeted, last)
    if last:
        return delta, x_pert, x_adv, found
    delta, x_pert = box(x, clamp_rows(delta + step * g.sign(), eps))
    return delta, x_pert, x_adv, found


def _l2_project(v, eps):
    """project_to_norm_ball(v, 'l2', eps) (adv_train_speech_commands.py:112-123), norms per row"""
    norm = torch.norm(v.reshape(v.shape[0], -1), dim=1).reshape((-1,) + (1,) * (v.dim() - 1))
    return v * torch.min(torch.ones_like(norm), _rows(eps, v) / norm)


def step_l2(x, g, delta, x_pert, x_adv, found, pred, y, step, eps, targeted=False, last=False):
    """ap_pgd_step_l2 -> (delta, x_pert, x_adv, found)"""
    x_adv, found = _bookkeep(x_pert, x_adv, found, pred, y, targeted, last)
    if last:
        return delta, x_pert, x_adv, found
    delta, x_pert = box(x, _l2_project(delta + step * _l2_project(g, 1), eps))
    return delta, x_pert, x_adv, found


# ---------------------------------------------------------------------------------------------------------
# 3. the loops
# ---------------------------------------------------------------------------------------------------------
def pgd_loop(model, x, y, eps, alpha, n, p="linf", transform=None, criterion=None, u=None, accumulate=False, dtype=None):
    """Both scripts' ``pgd`` -> (x_adv, found).  ``u``: the draws of torch.rand_like.  ``accumulate``: the KWS script's never-zeroed
    delta.grad.  ``dtype``: run in that precision (the float64 reference)."""
    x = x.detach() if dtype is None else x.detach().to(dtype)
    u = u if dtype is None else u.to(dtype)
    criterion = criterion if criterion is not None else torch.nn.CrossEntropyLoss()
    delta, x_pert = init(x, u, eps)
    x_adv, found = torch.zeros_like(x), torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
    acc = None
    step = step_linf if p == "linf" else step_l2
    for i in range(n + 1):
        d = delta.detach().requires_grad_(True)
        xp = x + d
        y_pert = model(xp if transform is None else transform(xp))
        pred = argmax_rows(y_pert.detach())
        if i == n:
            delta, x_pert, x_adv, found = step(x, None, delta, xp.detach(), x_adv, found, pred, y, alpha, eps, last=True)
            break
        g, = torch.autograd.grad(criterion(y_pert, y), d)
        acc = g if acc is None or not accumulate else acc + g
        delta, x_pert, x_adv, found = step(x, acc, delta, xp.detach(), x_adv, found, pred, y, alpha, eps)
    return x_adv, found


def stage_1_loop(model, criterion, x, y, eps, lr, n, targeted):
    """AudioAttack.stage_1 (linf, no EOT) -> (x_adv, found)"""
    x = x.detach()
    delta, x_pert = init(x, None, 0.0)
    x_adv, found = torch.zeros_like(x), torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
    eps_rows = torch.full((x.shape[0],), eps, dtype=x.dtype, device=x.device)
    for i in range(n + 1):
        d = delta.detach().requires_grad_(True)
        xp = x + d
        y_pert = model(xp)
        pred = argmax_rows(y_pert.detach())
        if i == n:
            delta, x_pert, x_adv, found = step_linf(x, None, delta, xp.detach(), x_adv, found, pred, y, 0.0, eps_rows, targeted, last=True)
            break
        g, = torch.autograd.grad(criterion(y_pert, y), d)
        delta, x_pert, x_adv, found = step_linf(x, g, delta, xp.detach(), x_adv, found, pred, y, -lr if targeted else lr, eps_rows, targeted)
    return x_adv, found


# ---------------------------------------------------------------------------------------------------------
# 4. the fixture's cases
# ---------------------------------------------------------------------------------------------------------
def special_values(g, it):
    """+0, -0, NaN and denormals into a gradient [B, 1, L] (L = 1: one of them per iteration)"""
    sp = [0.0, -0.0, float("nan"), 1e-42, -1e-42]
    B, _, L = g.shape
    if L == 1:
        g[0, 0, 0] = sp[(it + 2) % len(sp)] if it % 2 else g[0, 0, 0]
        return g
    for b in range(B):
        for j, v in enumerate(sp):
            g[b, 0, (b + 2 * j + it) % L] = v
    return g


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict of numpy arrays: x [B,1,L], scores [n+1,B,K], G [n,B,1,L] (special values in), G_l2 (none), y and y_t (the untargeted
    and targeted labels), pred [n+1,B] (what the score rows were built for).  Shared by the tests: do not modify.

    Row 0's prediction goes a, b, a, a..: with y = b it is hit, missed, hit (the last hit wins), with the targeted y_t = a the same.
    Row 1's prediction never moves: y = it (never hit), y_t = another class (never hit).  Row 2 holds a tied maximum at iteration 0
    (the lowest index is the prediction, y the other index) and is hit there alone; row 3 holds a NaN at iteration 1 beside a larger
    finite score, which y names, and that is its last hit (targeted: its only one); with B = 3 row 2 takes the NaN too.  x holds exact +-1 and values within eps of +-1; the first half of
    each gradient row keeps its sign over the iterations, so delta + step leaves the eps ball there."""
    B, L, n = CASES[name]
    r = np.random.default_rng(sum(map(ord, name)))
    x = r.uniform(-0.9, 0.9, (B, 1, L)).astype(np.float32)
    edge = [1.0, -1.0, 1.0 - EPS / 2, -1.0 + EPS / 3, 1.0 - EPS * 0.9, -1.0 + EPS * 0.99]
    for b in range(B):
        for j, v in enumerate(edge):
            if L > 1 or j == 2:
                x[b, 0, (3 * b + j) % L] = v
    y = np.array([3, 2, 4, 5, 1][:B], np.int64)
    y_t = np.array([0, 5, 1, 2, 1][:B], np.int64)
    it = np.arange(n + 1)
    pred = np.empty((n + 1, B), np.int64)
    pred[:, 0] = np.where(it == 1, 3, 0)
    if B > 1:
        pred[:, 1] = 2
    if B > 2:
        pred[:, 2] = np.where(it == 0, 1, 4)                     # hit at the tie alone
    if B > 3:
        pred[:, 3] = np.where(it == 0, 0, np.where(it == 1, 2, 5))       # the NaN iteration is the last hit
    if B > 4:
        pred[:, 4] = (it + 4) % K
    scores = r.uniform(-3.0, 3.0, (n + 1, B, K)).astype(np.float32)
    for i in range(n + 1):
        for b in range(B):
            scores[i, b, pred[i, b]] = 4.0 + 0.25 * i
    if B > 2:
        scores[0, 2, 1] = scores[0, 2, 4] = 5.0                  # the tie: indices 1 and 4 share the maximum, the prediction is 1
        nan_row = 3 if B > 3 else 2
        scores[1, nan_row, 2] = np.nan                           # the NaN is the maximum; index 5 holds a larger finite score than any
        scores[1, nan_row, 5] = 9.0
        pred[1, nan_row] = 2
    base = r.standard_normal((B, 1, L)).astype(np.float32)
    G = np.empty((n, B, 1, L), np.float32)
    for i in range(n):
        gi = (base * r.uniform(0.5, 1.5, (B, 1, L))).astype(np.float32)
        flip = r.random((B, 1, L)) < 0.5
        flip[..., :(L + 1) // 2] = False
        G[i] = np.where(flip, -gi, gi)
    G_l2 = G.copy()
    if B > 1:
        G_l2[0, 1] = 0.0                                         # a zero-gradient row
        G_l2[1:, 0] *= 1e-3                                      # ... and rows whose norm is below 1 (the factor is exactly 1)
    for i in range(n):
        G[i] = special_values(torch.from_numpy(G[i].copy()), i).numpy()
    return dict(x=x, scores=scores, G=G, G_l2=G_l2, y=y, y_t=y_t, pred=pred)


def model_of(c, which="G"):
    return ScriptedModel([torch.from_numpy(s) for s in c["scores"]], [torch.from_numpy(g) for g in c[which]])


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def restated(name, form, device="cpu"):
    """the float32 restatement of one recorded run -> (x_adv, found); form: 'kws', 'convnet', 'convnet_l2', 'stage1_t', 'stage1_u'"""
    c, g = case(name), golden()
    B, L, n = CASES[name]
    t = lambda a: torch.from_numpy(np.asarray(a)).to(device)    # noqa: E731
    x, u = t(c["x"]), t(g[f"{name}/u"])
    if form == "kws":
        return pgd_loop(model_of(c), x, t(c["y"]), EPS, ALPHA, n, u=u, accumulate=True)
    if form == "convnet":
        return pgd_loop(model_of(c), x, t(c["y"]), EPS, ALPHA, n, u=u)
    if form == "convnet_l2":
        return pgd_loop(model_of(c, "G_l2"), x, t(c["y"]), EPS, ALPHA, n, p="l2", u=u)
    targeted = form == "stage1_t"
    return stage_1_loop(model_of(c), torch.nn.CrossEntropyLoss(), x, t(c["y_t"] if targeted else c["y"]), EPS, LR, n, targeted)


FORMS = ("kws", "convnet", "convnet_l2", "stage1_t", "stage1_u")


# ---------------------------------------------------------------------------------------------------------
# 5. inputs of the kernel tests
# ---------------------------------------------------------------------------------------------------------
KERNEL_SHAPES = [(1, 1), (3, 7), (2, 1023), (5, 4099), (2, 16000)]      # (B, n): one element; tails only; one quad short of a chunk's
                                                                        # quarter; a second chunk of 3 elements; four chunks


@functools.lru_cache(maxsize=None)
def kernel_inputs(B, n, l2=False):
    """-> dict of numpy arrays for one kernel call at (B, n): x, u, g, delta, x_pert (a consistent iterate), x_adv (what an earlier hit
    left), found, pred, scores (whose argmax is pred; a tie and a NaN row where B allows), y, eps_rows.  Shared: do not modify."""
    r = np.random.default_rng(1000 * B + n + (7 if l2 else 0))
    x = r.uniform(-0.95, 0.95, (B, n)).astype(np.float32)
    edge = [1.0, -1.0, 1.0 - EPS / 2, -1.0 + EPS / 3]
    for b in range(B):
        for j, v in enumerate(edge):
            if n > len(edge) or j == (b % len(edge)):
                x[b, (5 * b + j) % n] = v
    u = r.random((B, n)).astype(np.float32)
    d0 = (np.float32(EPS) * (2 * u - 1).astype(np.float32)).astype(np.float32)
    delta = (np.clip((x + d0).astype(np.float32), -1, 1) - x).astype(np.float32)
    g = r.standard_normal((B, n)).astype(np.float32)
    if l2:
        g[0] *= 50.0                                             # |g| > 1: the gradient is scaled, the step leaves the ball
        if B > 1:
            g[1] = 0.0                                           # the zero-gradient row
        if B > 2:
            g[2] *= 1e-6                                         # stays inside: both factors exactly 1 ...
            delta[2] *= 1e-3                                     # ... from a small perturbation
    else:
        g = special_values(torch.from_numpy(g.reshape(B, 1, n).copy()), 0).numpy().reshape(B, n)
    x_pert = (x + delta).astype(np.float32)
    scores = r.uniform(-3, 3, (B, K)).astype(np.float32)
    if B > 1:
        scores[1, 1] = scores[1, 4] = 5.0
    if B > 2:
        scores[2, 3], scores[2, 5] = np.nan, 9.0
    pred = torch.from_numpy(scores).max(1)[1].numpy()
    y = pred.copy()
    y[::2] = (y[::2] + 1) % K                                    # even rows are predicted wrongly
    found = (np.arange(B) % 3 == 1).astype(np.uint8)
    x_adv = r.uniform(-1, 1, (B, n)).astype(np.float32)
    eps_rows = (EPS * (1.0 + 0.25 * np.arange(B))).astype(np.float32)
    return dict(x=x, u=u, g=g, delta=delta, x_pert=x_pert, x_adv=x_adv, found=found, pred=pred, scores=scores, y=y, eps_rows=eps_rows)


def rel(a, ref):
    """max |a - ref| / max |ref| in float64 (an exact-zero reference: the absolute figure)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    d, s = float(np.abs(a - ref).max()), float(np.abs(ref).max())
    return d / s if s > 0 else d


# ---------------------------------------------------------------------------------------------------------
# 6. a stand-in checkout for the drop-in's stage 1
# ---------------------------------------------------------------------------------------------------------
# robustness_eval/white_box_attack.py of a stand-in checkout: an AudioAttack with the constructor arguments and attribute names of the
# reference's (the fixture records those names: golden "audio_attack/attributes"), a generate() that leaves `targeted` in `_targeted` and
# calls stage_1, and a stage_1 that only says it ran.  None of the reference's text.
STANDIN_CHECKOUT = """
from ._EOT import EOT


class PsychoacousticMasker:
    pass


class AudioAttack:
    def __init__(self, model, masker=None, criterion=None, eps=2000.0, norm='linf', learning_rate_1=100.0, max_iter_1=1000,
                 max_iter_2=4000, eot_attack_size=15, eot_defense_size=15, verbose=1, **more):
        self.model, self.masker, self.criterion, self.eps, self.norm = model, masker, criterion, eps, norm
        self.learning_rate_1, self.max_iter_1, self.max_iter_2 = learning_rate_1, max_iter_1, max_iter_2
        self.eot_attack_size, self.eot_defense_size, self.verbose = eot_attack_size, eot_defense_size, verbose
        self._targeted = True
        self.ran = []

    def generate(self, x, y, targeted=True):
        self._targeted = targeted
        return self.stage_1(x, y)

    def stage_1(self, x, y):
        self.ran.append(self.norm)
        return "stage_1 of the checkout"

    def _loss_gradient_masking_threshold(self, *a):
        raise RuntimeError("unused")

    def _stabilized_threshold_and_psd_maximum(self, x):
        raise RuntimeError("unused")
"""


class ScriptedEOT:
    """what stage 1 asks of ``attack.eot_model``: with use_grad off the i-th recorded scores, with it on the i-th recorded gradient
    (and on to i + 1) -- the scripted model's run through both EOT branches"""

    def __init__(self, c):
        self.c, self.i, self.asked = c, 0, []
        self.EOT_size, self.use_grad = None, None

    def __call__(self, x, y):
        self.asked.append((self.EOT_size, self.use_grad))
        if not self.use_grad:
            return torch.from_numpy(self.c["scores"][self.i]).to(x.device), None, None, None
        g = torch.from_numpy(self.c["G"][self.i]).to(x.device).reshape(x.shape)
        self.i += 1
        return None, None, g, None
