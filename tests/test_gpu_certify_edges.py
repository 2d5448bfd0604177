"""The certification loop's own kernels where they branch: ``ap_argmax_hist`` (ap_backward.hip) against numpy -- ties, signed
zeros, non-finite rows at the first, a middle and the last column, a running histogram, B around the 256-thread block --
``ap_affine_noise`` alone (ap_kernels.hip: the quad tail, explicit and Philox noise at a 64-bit utterance offset, ``cs == 0``
without noise, no ``x``), and ``RobustCertificate`` with ``denoiser=None`` on a stub classifier that records what it is given:
row i of any device batch is global sample i of one Philox stream, the votes are the arg-maxes of the scores the classifier
returned, and a non-finite score row is refused.

One-line defects these cases catch and tests/test_gpu_certify.py (two flipped votes allowed, finite scores only) does not:
``>=`` for ``>`` in the arg-max (ties); ``counts + am`` for a non-finite row, or a finiteness test that misses -inf or the
last column; a 32-bit add into the histogram; ``first_sample`` not passed on, so that every device batch draws samples
0 .. 127 again; the kernel's Philox draw made for ``cs == 0`` or skipped for ``x == NULL``."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audiopure_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, -77.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _hist(dev, scores, counts=None):
    """ap_argmax_hist of scores [B, K] (numpy fp32) into counts (int64 [K + 1] device tensor; fresh zeros if None)."""
    B, K = scores.shape
    if counts is None:
        counts = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    s = torch.from_numpy(np.ascontiguousarray(scores)).to(dev)
    N.check(N.lib().ap_argmax_hist(N.ptr(s), counts.data_ptr(), B, K, N.stream()), "ap_argmax_hist")
    torch.cuda.synchronize()
    return counts


def _want(scores):
    K = scores.shape[1]
    return np.append(np.bincount(np.argmax(scores, axis=1), minlength=K), 0)   # numpy's argmax is first-maximum too


@pytest.mark.parametrize("K", (1, 2, 10, 35))
@pytest.mark.parametrize("B", (1, 255, 256, 257, 1000))
def test_argmax_hist_first_maximum_against_numpy(dev, B, K):
    rng = np.random.default_rng([B, K])
    cont = rng.normal(size=(B, K)).astype(np.float32)
    assert np.array_equal(_hist(dev, cont).cpu().numpy(), _want(cont))
    # three levels, the top one likely: most rows have their maximum more than once, and the first one must win
    quant = rng.choice(np.array([-1.5, 0.25, 2.0], dtype=np.float32), size=(B, K), p=(0.1, 0.1, 0.8))
    quant[0] = 0.25                                                           # (a whole row of one value: vote for class 0)
    tied = (quant == quant.max(axis=1, keepdims=True)).sum(axis=1) > 1
    if K > 1:
        assert tied.mean() >= 0.5
        last = np.bincount(K - 1 - np.argmax(quant[:, ::-1], axis=1), minlength=K)      # what a last-maximum rule would count
        assert not np.array_equal(last, _want(quant)[:K])
    assert np.array_equal(_hist(dev, quant).cpu().numpy(), _want(quant))
    # 0.0 against -0.0 compare equal: every row votes for class 0
    zeros = rng.choice(np.array([0.0, -0.0], dtype=np.float32), size=(B, K))
    zeros[0, 0], zeros[0, -1] = -0.0, 0.0
    got = _hist(dev, zeros).cpu().numpy()
    assert np.array_equal(got, _want(zeros)) and got[0] == B


@pytest.mark.parametrize("K", (1, 2, 10, 35))
def test_non_finite_rows_count_once_in_slot_k_and_nowhere_else(dev, K):
    rng = np.random.default_rng(K)
    cols = (0, K // 2, K - 1)
    specials = [(v, c) for v in (np.nan, np.inf, -np.inf) for c in cols]
    for v, c in specials:                                                     # each alone, in a large finite row
        row = (100 * rng.normal(size=(1, K))).astype(np.float32)
        row[0, c] = v
        want = np.zeros(K + 1, dtype=np.int64)
        want[K] = 1
        assert np.array_equal(_hist(dev, row).cpu().numpy(), want), (v, c)
    B = 300
    scores = rng.normal(size=(B, K)).astype(np.float32)
    where = (0, 1, 100, 254, 255, 256, 257, 298, 299)                         # both sides of the block edge, first and last row
    for r, (v, c) in zip(where, specials):
        scores[r, c] = v
    finite = np.delete(scores, where, axis=0)
    want = _want(finite)
    want[K] = len(where)
    assert np.array_equal(_hist(dev, scores).cpu().numpy(), want)


def test_histogram_accumulates_across_calls_and_above_2_to_32(dev):
    rng = np.random.default_rng(3)
    K = 10
    a, b = rng.normal(size=(257, K)).astype(np.float32), rng.normal(size=(1000, K)).astype(np.float32)
    b[7, 3] = np.nan
    start = (1 << 32) + 7 + np.arange(K + 1, dtype=np.int64) * ((1 << 31) + 1)
    counts = torch.from_numpy(start.copy()).to(dev)
    _hist(dev, a, counts)
    assert np.array_equal(counts.cpu().numpy(), start + _want(a))
    _hist(dev, b, counts)
    wb = _want(np.delete(b, 7, axis=0))
    wb[K] = 1
    assert np.array_equal(counts.cpu().numpy(), start + _want(a) + wb)


def test_argmax_hist_refusals(dev):
    lib = N.lib()
    s = torch.zeros(4, 3, device=dev)
    counts = torch.full((4,), 5, dtype=torch.int64, device=dev)
    for args in ((None, counts.data_ptr(), 4, 3), (N.ptr(s), None, 4, 3), (N.ptr(s), counts.data_ptr(), 0, 3),
                 (N.ptr(s), counts.data_ptr(), 4, 0), (N.ptr(s), counts.data_ptr(), -1, 3)):
        assert lib.ap_argmax_hist(*args, N.stream()) == -22
        assert b"ap_argmax_hist" in lib.ap_last_error()
    torch.cuda.synchronize()
    assert counts.tolist() == [5, 5, 5, 5]


# ---- ap_affine_noise alone ------------------------------------------------------------------------------------------
CA, CS = float(np.float32(0.75003)), float(np.float32(0.30001))
SEED, DRAW, OFFSET = 0x0FEDCBA987654321, 2, (1 << 33) + 5


def _affine(dev, x, ca, cs, z, B, L, seed=SEED, draw=DRAW, off=OFFSET):
    out = torch.full((B * L + GUARD,), SENTINEL, device=dev)
    N.check(N.lib().ap_affine_noise(N.ptr(x), N.ptr(out), ca, cs, N.ptr(z), seed, draw, off, B, L, N.stream()),
            "ap_affine_noise")
    torch.cuda.synchronize()
    assert bool((out[B * L:] == SENTINEL).all())                              # the quad tail stops at L
    got = out[:B * L].cpu().numpy().reshape(B, L)
    assert not (got == SENTINEL).any()
    return got


def _philox(dev, B, L, seed=SEED, draw=DRAW, off=OFFSET):
    z = torch.empty(B, L, device=dev)
    N.check(N.lib().ap_philox_normal(N.ptr(z), seed, draw, off, B, L, N.stream()), "ap_philox_normal")
    return z


@pytest.mark.parametrize("L", (1, 3, 4, 5, 1023, 1025))
def test_affine_noise_alone(dev, L):
    """Tolerance 2^-23 (|ca x| + |cs z|) per element: two product roundings and an add, or one fma."""
    B = 3
    rng = np.random.default_rng(L)
    xh = rng.uniform(-1, 1, (B, L)).astype(np.float32)
    x = torch.from_numpy(xh).to(dev)
    explicit = torch.from_numpy(rng.normal(size=(B, L)).astype(np.float32)).to(dev)
    filled = _philox(dev, B, L)
    assert not torch.equal(filled[0], filled[1])
    for z_arg, z in ((explicit, explicit), (None, filled)):                   # None: the kernel draws utterance OFFSET + b
        zh = z.cpu().numpy().astype(np.float64)
        got = _affine(dev, x, CA, CS, z_arg, B, L)
        want = CA * xh.astype(np.float64) + CS * zh
        tol = 2.0 ** -23 * (np.abs(CA * xh) + np.abs(CS * zh))
        assert np.all(np.abs(got - want) <= tol)
        # no x: cs z exactly (ca must be 0, see the refusals)
        got = _affine(dev, None, 0.0, CS, z_arg, B, L)
        assert np.array_equal(got, (CS * zh).astype(np.float32))
    # cs == 0 and no z: fl32(ca x) exactly, and finite (no draw is made, nothing uninitialised is multiplied by 0)
    got = _affine(dev, x, CA, 0.0, None, B, L)
    assert np.isfinite(got).all() and np.array_equal(got, (CA * xh.astype(np.float64)).astype(np.float32))
    # the low word of the offset alone is another stream
    assert not torch.equal(_philox(dev, B, L, off=5), filled)


def test_affine_noise_refusals(dev):
    lib = N.lib()
    x = torch.zeros(2, 8, device=dev)
    out = torch.full((2, 8), SENTINEL, device=dev)
    st = N.stream()
    assert lib.ap_affine_noise(N.ptr(x), None, 1.0, 0.5, None, 1, 0, 0, 2, 8, st) == -22
    assert lib.ap_affine_noise(N.ptr(x), N.ptr(out), 1.0, 0.5, None, 1, 0, 0, 0, 8, st) == -22
    assert lib.ap_affine_noise(N.ptr(x), N.ptr(out), 1.0, 0.5, None, 1, 0, 0, 2, 0, st) == -22
    assert lib.ap_affine_noise(None, N.ptr(out), 1.0, 0.5, None, 1, 0, 0, 2, 8, st) == -22       # x == NULL needs ca == 0
    assert b"x is NULL" in lib.ap_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- RobustCertificate without a denoiser ------------------------------------------------------------------------------
class Recorder(torch.nn.Module):
    """Fixed-weight linear scores; keeps every input and every returned score row."""

    def __init__(self, L, K, dev, nan_at=None):
        super().__init__()
        w = torch.from_numpy(np.random.default_rng(11).normal(size=(K, L)).astype(np.float32))
        self.w = torch.nn.Parameter(w.to(dev), requires_grad=False)
        self.nan_at = nan_at                                                  # (call, row) whose scores become NaN
        self.inputs, self.scores = [], []

    def forward(self, x):
        s = x[:, 0, :] @ self.w.t()
        if self.nan_at is not None and len(self.inputs) == self.nan_at[0]:
            s[self.nan_at[1], 4] = float("nan")
        self.inputs.append(x.detach().clone())
        self.scores.append(s.detach().clone())
        return s


def test_randomised_smoothing_batches_continue_one_philox_stream(dev):
    from audiopure_amd.robustness_eval.certified_robust import RobustCertificate
    L, K, n, sigma = 4001, 10, 300, 0.25
    clf = Recorder(L, K, dev)
    rc = RobustCertificate(classifier=clf, transform=None, denoiser=None)
    assert rc.classifier is clf
    rc.seed, rc.native_batch = 77, 128
    xh = np.random.default_rng(12).uniform(-0.1, 0.1, (1, 1, L)).astype(np.float32)
    counts = rc.smooth_predict(torch.from_numpy(xh).to(dev), num_sampling=n, sigma=sigma, batch_size=64)
    assert [t.shape[0] for t in clf.inputs] == [128, 128, 44]
    seen = torch.cat(clf.inputs)[:, 0].cpu().numpy()
    z = _philox(dev, n, L, seed=77, draw=0, off=0).cpu().numpy().astype(np.float64)
    s32 = float(np.float32(sigma))
    want = xh[0].astype(np.float64) + s32 * z                                 # row i of any batch is global sample i
    assert np.all(np.abs(seen - want) <= 2.0 ** -23 * (np.abs(xh[0]) + np.abs(s32 * z)))
    # had the second batch started the stream again, its rows would be the first batch's
    assert np.abs(seen[128:256] - seen[:128]).max() > sigma
    scores = torch.cat(clf.scores).cpu().numpy()
    assert np.isfinite(scores).all()
    votes = np.bincount(scores.argmax(axis=1), minlength=K)
    assert counts.dtype == torch.int64 and counts.tolist() == votes.tolist() and int(counts.sum()) == n
    assert (votes > 0).sum() >= 3                                             # a histogram with something to get wrong


def test_smooth_predict_refuses_a_non_finite_score_row(dev):
    from audiopure_amd.robustness_eval.certified_robust import RobustCertificate
    L = 4001
    clf = Recorder(L, 10, dev, nan_at=(1, 17))
    rc = RobustCertificate(classifier=clf, transform=None, denoiser=None)
    rc.seed, rc.native_batch = 77, 128
    x = torch.from_numpy(np.random.default_rng(12).uniform(-0.1, 0.1, (1, 1, L)).astype(np.float32)).to(dev)
    with pytest.raises(FloatingPointError, match="1 of 300 score rows are not finite"):
        rc.smooth_predict(x, num_sampling=300, sigma=0.25, batch_size=64)
    assert len(clf.inputs) == 3                                               # counted on the device, read once at the end
