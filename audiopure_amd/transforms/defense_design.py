"""Host-side design of the baseline defenses' coefficients, numpy only (no scipy, no torchaudio at run time).

* ``buttord`` / ``butter``: the digital low-pass and band-pass Butterworth design the reference calls through
  ``scipy.signal`` (frequency_defense.py:82-87,122-127): pre-warp with tan(pi w / 2), the order formula, the W0
  back-conversion to the 3 dB edge(s), the analog prototype, lowpass -> lowpass / bandpass, the bilinear transform and
  zpk -> ba.  ``lpf_design`` / ``bpf_design`` then cast b and a to fp32 as the reference does (:89-90,129-130).
* ``resample_kernel``: torchaudio 0.11's ``sinc_interpolation`` kernel (lowpass_filter_width 6, rolloff 0.99, Hann^2
  window), built in float64 and rounded once to fp32; ``ds_taps`` gives the two kernels of DS (16 k -> 8 k -> 16 k).
* ``chunk_operators``: A^C and the zero-input output basis H[k] = e_0' A^k of the direct-form-II-transposed state
  recurrence, the host half of the parallel-in-time scan of ap_iir_fwd / ap_iir_bwd.

The one deliberate departure from the reference: a design whose fp32-cast denominator has a pole on or outside the unit
circle (e.g. ``LPF(wp=20, param=40)``: order 7, largest pole |1.12| after the cast) is refused with ``ValueError`` naming
the pole radius, where the reference filters anyway and returns NaN / overflow.
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

IIR_CHUNK = 128            # AP_IIR_CHUNK of include/audiopure.h
IIR_MAX_COEF = 16          # AP_IIR_MAX_COEF


def buttord(wp, ws, gpass, gstop):
    """Digital Butterworth order selection (``scipy.signal.buttord(wp, ws, gpass, gstop, analog=False)``) for the
    low-pass (scalar edges, wp < ws) and band-pass (two edges, ws outside wp) cases.  Returns (N, Wn)."""
    wp = np.atleast_1d(np.asarray(wp, dtype=np.float64))
    ws = np.atleast_1d(np.asarray(ws, dtype=np.float64))
    if wp.shape != ws.shape or wp.size not in (1, 2):
        raise ValueError("wp and ws must both be scalars (low-pass) or both pairs (band-pass)")
    ftype = 2 * (wp.size - 1) + 1 + (1 if wp[0] >= ws[0] else 0)
    if ftype not in (1, 4):
        raise NotImplementedError("only the low-pass and band-pass designs of LPF / BPF are restated")
    with np.errstate(divide="ignore", over="ignore"):
        passb = np.tan(np.pi * wp / 2.0)
        stopb = np.tan(np.pi * ws / 2.0)
    if ftype == 1:
        nat = stopb / passb
    else:
        nat = (stopb ** 2 - passb[0] * passb[1]) / (stopb * (passb[0] - passb[1]))
    nat = np.min(np.abs(nat))
    GSTOP = 10 ** (0.1 * abs(gstop))
    GPASS = 10 ** (0.1 * abs(gpass))
    order = int(math.ceil(math.log10((GSTOP - 1.0) / (GPASS - 1.0)) / (2 * math.log10(nat))))
    if order < 1:
        raise ValueError(f"buttord: order {order} from wp={wp}, ws={ws}, gpass={gpass}, gstop={gstop}")
    W0 = (GPASS - 1.0) ** (-1.0 / (2.0 * order))
    if ftype == 1:
        WN = W0 * passb
    else:
        W0 = np.array([-W0, W0], float)
        WN = -W0 * (passb[1] - passb[0]) / 2.0 + np.sqrt(W0 ** 2 / 4.0 * (passb[1] - passb[0]) ** 2 + passb[0] * passb[1])
        WN = np.sort(np.abs(WN))
    wn = np.arctan(WN) * 2.0 / np.pi
    return order, (wn[0] if wn.size == 1 else wn)


def _poly_real(roots):
    c = np.poly(roots) if len(roots) else np.array([1.0])
    return np.real(c) if np.iscomplexobj(c) else c


def butter(N, Wn, btype="low"):
    """``scipy.signal.butter(N, Wn, btype, analog=False, output='ba')`` for btype 'low' / 'bandpass' (float64)."""
    Wn = np.asarray(Wn, dtype=np.float64)
    if np.any(Wn <= 0) or np.any(Wn >= 1):
        raise ValueError("Digital filter critical frequencies must be 0 < Wn < 1")
    N = int(N)
    m = np.arange(-N + 1, N, 2)
    p = -np.exp(1j * np.pi * m / (2 * N))           # analog prototype: no zeros, gain 1
    z = np.array([], dtype=complex)
    k = 1.0
    fs = 2.0
    warped = 2 * fs * np.tan(np.pi * Wn / fs)
    if btype in ("low", "lowpass"):
        if Wn.size != 1:
            raise ValueError("a low-pass design takes one critical frequency")
        wo = float(warped)
        degree = len(p) - len(z)
        z, p, k = wo * z, wo * p, k * wo ** degree
    elif btype in ("band", "bandpass"):
        if Wn.size != 2:
            raise ValueError("a band-pass design takes two critical frequencies")
        bw = float(warped[1] - warped[0])
        wo = float(np.sqrt(warped[0] * warped[1]))
        degree = len(p) - len(z)
        z_lp, p_lp = (z * bw / 2).astype(complex), (p * bw / 2).astype(complex)
        z = np.concatenate((z_lp + np.sqrt(z_lp ** 2 - wo ** 2), z_lp - np.sqrt(z_lp ** 2 - wo ** 2)))
        p = np.concatenate((p_lp + np.sqrt(p_lp ** 2 - wo ** 2), p_lp - np.sqrt(p_lp ** 2 - wo ** 2)))
        z = np.append(z, np.zeros(degree))
        k = k * bw ** degree
    else:
        raise NotImplementedError(f"btype {btype!r}: only 'low' and 'bandpass' are restated")
    fs2 = 2.0 * fs                                   # bilinear transform
    degree = len(p) - len(z)
    k = k * np.real(np.prod(fs2 - z) / np.prod(fs2 - p))
    z = np.append((fs2 + z) / (fs2 - z), -np.ones(degree))
    p = (fs2 + p) / (fs2 - p)
    b = k * _poly_real(z)
    a = _poly_real(p)
    return np.real(b).astype(np.float64), np.real(a).astype(np.float64)


def pole_radius(a) -> float:
    """Largest |pole| of the denominator ``a`` (float64 roots of the given coefficients)."""
    a = np.asarray(a, dtype=np.float64)
    return float(np.max(np.abs(np.roots(a)))) if a.size > 1 else 0.0


def _checked(N, Wn, b, a, what):
    b32, a32 = b.astype(np.float32), a.astype(np.float32)
    if b32.size > IIR_MAX_COEF:
        raise ValueError(f"{what}: order {N} needs {b32.size} coefficients; the native filter takes at most {IIR_MAX_COEF}")
    r = pole_radius(a32)
    if not r < 1.0:
        raise ValueError(f"{what}: the fp32-cast design (order {N}, Wn={Wn}) has a pole of radius {r:.6g} >= 1; "
                         "the filter is unstable and is refused (the reference would return NaN / overflow)")
    return N, Wn, b32, a32


@lru_cache(maxsize=64)
def lpf_design(fs=16000, wp=4000, param=8000, gpass=3, gstop=40):
    """(N, Wn, b fp32, a fp32) of LPF (frequency_defense.py:82-90)."""
    N, Wn = buttord(2 * wp / fs, 2 * param / fs, gpass, gstop)
    b, a = butter(N, Wn, "low")
    return _checked(N, Wn, b, a, f"LPF(fs={fs}, wp={wp}, param={param})")


@lru_cache(maxsize=64)
def bpf_design(fs=16000, wp=(300, 4000), param=(50, 8000), gpass=3, gstop=40):
    """(N, Wn, b fp32, a fp32) of BPF (frequency_defense.py:122-130); N is buttord's order (the filter's is 2N)."""
    N, Wn = buttord([2 * w / fs for w in wp], [2 * w / fs for w in param], gpass, gstop)
    b, a = butter(N, Wn, "bandpass")
    return _checked(N, Wn, b, a, f"BPF(fs={fs}, wp={list(wp)}, param={list(param)})")


def state_matrix(a) -> np.ndarray:
    """A of the DF2T state recurrence s' = A s + B u for the (a[0]-normalised) denominator a: A[i][0] = -a[i+1],
    A[i][i+1] = 1 (float64 of the given coefficients)."""
    a = np.asarray(a, dtype=np.float64)
    a = a / a[0]
    N = a.size - 1
    A = np.zeros((N, N))
    A[:, 0] = -a[1:]
    A[np.arange(N - 1), np.arange(1, N)] = 1.0
    return A


@lru_cache(maxsize=64)
def _chunk_ops_cached(a_bytes, C):
    a = np.frombuffer(a_bytes, dtype=np.float32)
    A = state_matrix(a)
    N = A.shape[0]
    H = np.empty((C, N))
    row = np.zeros(N)
    row[0] = 1.0
    for k in range(C):
        H[k] = row
        row = row @ A
    return np.linalg.matrix_power(A, C), H


def chunk_operators(a, C=IIR_CHUNK):
    """(A^C [N][N], H [C][N]) in float64 for the fp32 denominator ``a``: H[k] = e_0' A^k is the output k samples into a
    chunk due to the state entering it, A^C carries that state over the chunk."""
    AC, H = _chunk_ops_cached(np.ascontiguousarray(a, dtype=np.float32).tobytes(), int(C))
    return AC.copy(), H.copy()


def resample_kernel(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """torchaudio 0.11 ``_get_sinc_resample_kernel(..., 'sinc_interpolation')`` for the gcd-reduced rates: float64
    [new][2 width + orig] and width; the caller rounds once to fp32 (torchaudio's default dtype)."""
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = np.arange(-width, width + orig, dtype=np.float64)
    kernels = []
    for i in range(new):
        t = (-i / new + idx / orig) * base
        t = np.clip(t, -lowpass_filter_width, lowpass_filter_width)
        window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
        t = t * math.pi
        with np.errstate(invalid="ignore", divide="ignore"):
            kern = np.where(t == 0, 1.0, np.sin(t) / t)
        kernels.append(kern * window)
    return np.stack(kernels) * (base / orig), width


@lru_cache(maxsize=1)
def ds_taps():
    """(kd [28], ku [2][15]) fp32: the 2:1 down and the 1:2 up kernel of DS(param=0.5)."""
    kd, wd = resample_kernel(2, 1)
    ku, wu = resample_kernel(1, 2)
    assert kd.shape == (1, 28) and wd == 13 and ku.shape == (2, 15) and wu == 7
    return kd[0].astype(np.float32), ku.astype(np.float32)
