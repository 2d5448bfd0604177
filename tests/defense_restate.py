"""numpy restatements of the baseline defenses (transforms/time_defense.py, transforms/frequency_defense.py) that the
defense tests compare the HIP kernels with.  float64 arithmetic on the fp32 coefficients the reference uses; no scipy,
no torch, nothing read from the reference checkout."""
from __future__ import annotations

import numpy as np

from audiopure_amd.transforms import defense_design as D


def as_fwd(x, k=3):
    """AS: zero-padded moving average with w = float32(1 / k), as float64 sums."""
    x = np.asarray(x, np.float64)
    r = (k - 1) // 2
    w = float(np.float32(1.0 / k))
    xp = np.pad(x, ((0, 0), (r, r)))
    return sum(w * xp[:, j:j + x.shape[1]] for j in range(k))


def ms_fwd(x, k=3):
    """MS: (values, argmedian offsets) under the library's tie rule (rank r in the order (value, position))."""
    x = np.asarray(x, np.float32)
    r = (k - 1) // 2
    B, L = x.shape
    xp = np.pad(x, ((0, 0), (r, r)))
    win = np.stack([xp[:, j:j + L] for j in range(k)], axis=-1)          # [B, L, k]
    order = np.argsort(win, axis=-1, kind="stable")
    pick = order[..., r]
    vals = np.take_along_axis(win, pick[..., None], axis=-1)[..., 0]
    return vals, (pick - r).astype(np.int8)


def ms_bwd(g, off):
    """MS adjoint: dx[m] = sum over n with n + off[n] == m of g[n] (targets in the padding dropped)."""
    g = np.asarray(g, np.float64)
    B, L = g.shape
    dx = np.zeros((B, L))
    n = np.arange(L)
    for b in range(B):
        t = n + off[b].astype(np.int64)
        ok = (t >= 0) & (t < L)
        np.add.at(dx[b], t[ok], g[b][ok])
    return dx


def at_fwd(x, z, param=25):
    x, z = np.asarray(x, np.float64), np.asarray(z, np.float64)
    snr = 10 ** (param / 10)
    s = np.sqrt(np.sum(x * x, axis=1, keepdims=True) / x.shape[1] / snr)
    return x + z * s


def at_bwd(x, z, g, param=25):
    x, z, g = (np.asarray(t, np.float64) for t in (x, z, g))
    snr = 10 ** (param / 10)
    N = x.shape[1]
    s = np.sqrt(np.sum(x * x, axis=1, keepdims=True) / N / snr)
    return g + np.sum(g * z, axis=1, keepdims=True) * x / (N * snr * s)


def ds_fwd(x, same_size=True):
    """DS(param=0.5): torchaudio 0.11's two sinc_interpolation resamplers with the fp32 kernels, float64 sums."""
    kd, ku = (np.asarray(t, np.float64) for t in D.ds_taps())
    x = np.asarray(x, np.float64)
    B, L = x.shape
    M = (L + 1) // 2
    xp = np.pad(x, ((0, 0), (13, 13 + 2)))
    d = np.stack([xp[:, 2 * m:2 * m + 28] @ kd for m in range(M)], axis=1)            # [B, M]
    dp = np.pad(d, ((0, 0), (7, 7 + 1)))
    y = np.zeros((B, 2 * M))
    for p in range(2):
        y[:, p::2] = np.stack([dp[:, n:n + 15] @ ku[p] for n in range(M)], axis=1)
    return y[:, :L] if same_size else y


def ds_matrix(L, same_size=True):
    """The DS operator as a dense [Lout, L] matrix (for the adjoint: ds_matrix.T @ g)."""
    return ds_fwd(np.eye(L), same_size).T


def lfilter(b, a, x, reverse=False):
    """Direct-form-II-transposed IIR filter in float64 along the last axis (zero initial state); ``reverse`` runs it
    backwards in time, which is the adjoint of the forward filter."""
    b = np.asarray(b, np.float64) / float(a[0])
    a = np.asarray(a, np.float64) / float(a[0])
    x = np.asarray(x, np.float64)
    if reverse:
        x = x[..., ::-1]
    n = len(a) - 1
    z = np.zeros(x.shape[:-1] + (n,))
    y = np.empty_like(x)
    for t in range(x.shape[-1]):
        u = x[..., t]
        yt = b[0] * u + z[..., 0]
        for i in range(n - 1):
            z[..., i] = b[i + 1] * u - a[i + 1] * yt + z[..., i + 1]
        z[..., n - 1] = b[n] * u - a[n] * yt
        y[..., t] = yt
    return y[..., ::-1] if reverse else y


def clip_range(x, bits=16):
    """frequency_defense.py:75-80: the batch-global clamp range."""
    x = np.asarray(x, np.float32)
    if np.float32(0.9) * x.max() <= 1 and np.float32(0.9) * x.min() >= -1:
        return -1.0, 1.0
    return -2.0 ** (bits - 1), 2.0 ** (bits - 1) - 1


def filt_fwd(x, b, a, bits=16):
    """(clamped output, pre-clamp output) of LPF / BPF with the given fp32 design."""
    lo, hi = clip_range(x, bits)
    y = lfilter(b, a, x)
    return np.clip(y, lo, hi), y


def filt_bwd(x, g, b, a, bits=16):
    lo, hi = clip_range(x, bits)
    y = lfilter(b, a, x)
    m = (y >= lo) & (y <= hi)
    return lfilter(b, a, np.asarray(g, np.float64) * m, reverse=True)
