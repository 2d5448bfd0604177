"""Native baseline defenses: the reference's ``TimeDomainDefense`` (AT / AS / MS, transforms/time_defense.py) and
``FreqDomainDefense`` (DS / LPF / BPF, transforms/frequency_defense.py) on the HIP kernels of ap_defense.hip.

Same call signatures, defaults, shapes ([T], [B, T], [B, 1, T] in -> same shape out), ``_get_name()`` strings and
``NotImplementedError`` messages as the reference.  Every op is a ``torch.autograd.Function`` whose backward is the HIP
adjoint, so the white-box attack (robustness_eval/white_box_attack.py:378-439) differentiates through the defender
without a PyTorch-operator path.  CPU tensors raise (there is no CPU path).

Departures, all documented in INTEGRATION.md: ``AT`` takes ``noise=`` (an injected z) and otherwise draws the library's
Philox stream keyed on (seed, draw, utterance offset); a silent clip's AT gradient drops the term through its zero power
(the reference's autograd gives NaN there); LPF / BPF refuse a design whose fp32 denominator is unstable
(``defense_design``); DS has a kernel for the 2:1 ratio (``param=0.5``) only.
"""
from __future__ import annotations

import ctypes
import functools
import itertools
import math

import numpy as np
import torch

from .. import _native as N
from . import defense_design as D


def _on_device(fn):
    """``_native.on_device`` for a module-level function: the device of the first CUDA tensor argument is made current."""
    inner = N.on_device(lambda _self, *a, **k: fn(*a, **k))

    @functools.wraps(fn)
    def wrapper(*a, **k):
        return inner(None, *a, **k)
    return wrapper


def _flat(audio):
    """(x [B, T] float32 contiguous, original shape) with the reference's shape rules."""
    if not isinstance(audio, torch.Tensor):
        raise AssertionError(f"expected a torch.Tensor, got {type(audio).__name__}")   # the reference asserts here
    shape = audio.shape
    if audio.dim() == 1:
        x = audio.unsqueeze(0)
    elif audio.dim() == 2:
        x = audio
    elif audio.dim() == 3 and audio.shape[1] == 1:
        x = audio.squeeze(1)
    else:
        raise NotImplementedError('Audio Shape Error')
    if not x.is_cuda:
        raise N.NativeError("audiopure_amd defenses need device (cuda/HIP) tensors; got a CPU tensor and there is no CPU path")
    if x.dtype != torch.float32:
        x = x.float()
    return x.contiguous(), shape


def _host(a):
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    return (ctypes.c_float * a.size)(*a.tolist())


# ---------------------------------------------------------------------------------------------------------------- AS
class _ASFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        y = torch.empty_like(x)
        N.check(N.lib().ap_avg_smooth(N.ptr(x), N.ptr(y), k, x.shape[0], x.shape[1], N.stream()), "ap_avg_smooth")
        ctx.k = k
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        dx = torch.empty_like(g)                     # symmetric Toeplitz operator: the adjoint is the forward launch
        N.check(N.lib().ap_avg_smooth(N.ptr(g), N.ptr(dx), ctx.k, g.shape[0], g.shape[1], N.stream()), "ap_avg_smooth")
        return dx, None


@_on_device
def AS(audio, param=3, same_size=True):
    """Average smoothing over an odd window ``param`` (time_defense.py:102-124)."""
    x, shape = _flat(audio)
    if param % 2 != 1:
        raise AssertionError(f"AS: the window {param} must be odd")                # as time_defense.py:118 refuses it
    return _ASFn.apply(x, int(param)).view(shape)


# ---------------------------------------------------------------------------------------------------------------- MS
class _MSFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        y = torch.empty_like(x)
        off = torch.empty(x.shape, dtype=torch.int8, device=x.device)
        N.check(N.lib().ap_median_smooth(N.ptr(x), N.ptr(y), off.data_ptr(), k, x.shape[0], x.shape[1], N.stream()),
                "ap_median_smooth")
        ctx.k = k
        ctx.save_for_backward(off)
        ctx.mark_non_differentiable(off)
        return y, off

    @staticmethod
    def backward(ctx, g, _goff):
        (off,) = ctx.saved_tensors
        g = g.contiguous()
        dx = torch.empty_like(g)
        N.check(N.lib().ap_median_smooth_bwd(N.ptr(g), off.data_ptr(), N.ptr(dx), ctx.k, g.shape[0], g.shape[1], N.stream()),
                "ap_median_smooth_bwd")
        return dx, None


def median_smooth(audio, param=3):
    """(MS output, argmedian offsets int8) on the [B, T] view: the offsets say which window element each output took."""
    x, shape = _flat(audio)
    y, off = _MSFn.apply(x, int(param))
    return y.view(shape), off


@_on_device
def MS(audio, param=3, same_size=True):
    """Median smoothing over an odd window ``param`` <= 63 with zero padding (time_defense.py:127-156)."""
    return median_smooth(audio, param)[0]


# ---------------------------------------------------------------------------------------------------------------- AT
class _ATFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, z, snr):
        y = torch.empty_like(x)
        N.check(N.lib().ap_at_fwd(N.ptr(x), N.ptr(z), N.ptr(y), snr, x.shape[0], x.shape[1], N.stream()), "ap_at_fwd")
        ctx.snr = snr
        ctx.save_for_backward(x, z)
        return y

    @staticmethod
    def backward(ctx, g):
        x, z = ctx.saved_tensors
        g = g.contiguous()
        dx = torch.empty_like(g)
        N.check(N.lib().ap_at_bwd(N.ptr(x), N.ptr(z), N.ptr(g), N.ptr(dx), ctx.snr, x.shape[0], x.shape[1], N.stream()),
                "ap_at_bwd")
        return dx, None, None


_AT_DRAWS = itertools.count()


@_on_device
def AT(audio, param=25, same_size=True, noise=None, seed=None, draw=None, utt_offset=0):
    """Additive noise at ``param`` dB SNR per clip (time_defense.py:84-100).  ``noise`` ([B, T] or the input's shape)
    is used as z; otherwise z is the library's Philox N(0, 1) stream keyed on (seed, draw, utt_offset + clip) --
    ``seed`` defaults to ``torch.initial_seed()`` and ``draw`` to a per-process counter, so equal keys give equal z."""
    x, shape = _flat(audio)
    B, L = x.shape
    if noise is not None:
        z = noise.detach().to(device=x.device, dtype=torch.float32).reshape(B, L).contiguous()
    else:
        z = torch.empty_like(x)
        seed = torch.initial_seed() if seed is None else int(seed)
        draw = next(_AT_DRAWS) if draw is None else int(draw)
        N.check(N.lib().ap_philox_normal(N.ptr(z), seed & (2 ** 64 - 1), draw & 0xFFFFFFFF, int(utt_offset), B, L,
                                         N.stream()), "ap_philox_normal")
    snr = 10 ** (param / 10)
    return _ATFn.apply(x, z, float(snr)).view(shape)


# ---------------------------------------------------------------------------------------------------------------- DS
class _DSFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Lout):
        kd, ku = _ds_host()
        B, L = x.shape
        y = torch.empty((B, Lout), device=x.device, dtype=torch.float32)
        N.check(N.lib().ap_ds_fwd(N.ptr(x), N.ptr(y), kd, ku, B, L, Lout, N.stream()), "ap_ds_fwd")
        ctx.L = L
        return y

    @staticmethod
    def backward(ctx, g):
        kd, ku = _ds_host()
        g = g.contiguous()
        B, Lout = g.shape
        dx = torch.empty((B, ctx.L), device=g.device, dtype=torch.float32)
        N.check(N.lib().ap_ds_bwd(N.ptr(g), N.ptr(dx), kd, ku, B, ctx.L, Lout, N.stream()), "ap_ds_bwd")
        return dx, None


@functools.lru_cache(maxsize=1)
def _ds_host():
    kd, ku = D.ds_taps()
    return _host(kd), _host(ku)


@_on_device
def DS(audio, param=0.5, fs=16000, same_size=True):
    """Down-sample by ``param`` and back with torchaudio 0.11's sinc interpolation (frequency_defense.py:36-58)."""
    x, shape = _flat(audio)
    new_freq = int(fs * param)
    g = math.gcd(int(fs), new_freq)
    if (int(fs) // g, new_freq // g) != (2, 1):
        raise NotImplementedError(f"DS: the native resampler is built for the 2:1 ratio (param=0.5); got {fs} -> {new_freq}")
    L = x.shape[1]
    M = (L + 1) // 2
    y = _DSFn.apply(x, L if same_size else 2 * M)
    if same_size:
        return y.view(shape)
    return y.view(tuple(shape[:-1]) + (2 * M,))


# ------------------------------------------------------------------------------------------------------- LPF / BPF
class _Filter:
    """One fp32 design on the host (b, a, fp64 A^128) plus its fp64 zero-input basis H on each device."""

    def __init__(self, b32, a32):
        AC, H = D.chunk_operators(a32)
        self.ncoef = int(b32.size)
        self.b, self.a = _host(b32), _host(a32)
        AC = np.ascontiguousarray(AC, dtype=np.float64).ravel()
        self.AC = (ctypes.c_double * AC.size)(*AC.tolist())
        self.H64 = H
        self._H = {}

    def H(self, device):
        """Device pointer of the fp64 zero-input basis [128][N] on ``device`` (uploaded once per device)."""
        t = self._H.get(device)
        if t is None:
            t = self._H[device] = torch.from_numpy(np.ascontiguousarray(self.H64)).to(device)
        return t.data_ptr()


@functools.lru_cache(maxsize=64)
def _filter(kind, *key):
    _, _, b32, a32 = (D.lpf_design if kind == "lpf" else D.bpf_design)(*key)
    return _Filter(b32, a32)


class _IIRFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, filt, bits):
        B, L = x.shape
        y = torch.empty_like(x)
        ypre = torch.empty_like(x)
        mm = torch.empty(2, dtype=torch.int32, device=x.device)
        scratch = torch.empty(N.lib().ap_iir_scratch_elems(filt.ncoef, B, L), dtype=torch.float32, device=x.device)
        H = filt.H(x.device)
        N.check(N.lib().ap_iir_fwd(N.ptr(x), N.ptr(y), N.ptr(ypre), mm.data_ptr(), filt.b, filt.a, filt.ncoef, filt.AC,
                                   H, N.ptr(scratch), bits, B, L, N.stream()), "ap_iir_fwd")
        ctx.filt, ctx.bits = filt, bits
        ctx.save_for_backward(ypre, mm)
        return y

    @staticmethod
    def backward(ctx, g):
        ypre, mm = ctx.saved_tensors
        filt = ctx.filt
        g = g.contiguous()
        B, L = g.shape
        dx = torch.empty_like(g)
        scratch = torch.empty(N.lib().ap_iir_scratch_elems(filt.ncoef, B, L), dtype=torch.float32, device=g.device)
        N.check(N.lib().ap_iir_bwd(N.ptr(g), N.ptr(ypre), mm.data_ptr(), N.ptr(dx), filt.b, filt.a, filt.ncoef, filt.AC,
                                   filt.H(g.device), N.ptr(scratch), ctx.bits, B, L, N.stream()), "ap_iir_bwd")
        return dx, None, None


def iir_filter(x2d, b32, a32, adjoint=False):
    """The LPF / BPF scan without the clamp on a [B, T] device tensor: H x, or H' x with ``adjoint`` (the adjoint
    identity and long-tail tests use it)."""
    filt = _Filter(np.asarray(b32, np.float32), np.asarray(a32, np.float32))
    x = x2d.float().contiguous()
    B, L = x.shape
    out = torch.empty_like(x)
    scratch = torch.empty(N.lib().ap_iir_scratch_elems(filt.ncoef, B, L), dtype=torch.float32, device=x.device)
    H = filt.H(x.device)
    if adjoint:
        rc = N.lib().ap_iir_bwd(N.ptr(x), None, None, N.ptr(out), filt.b, filt.a, filt.ncoef, filt.AC, H,
                                N.ptr(scratch), 16, B, L, N.stream())
    else:
        ypre = torch.empty_like(x)
        mm = torch.empty(2, dtype=torch.int32, device=x.device)
        rc = N.lib().ap_iir_fwd(N.ptr(x), N.ptr(out), N.ptr(ypre), mm.data_ptr(), filt.b, filt.a, filt.ncoef, filt.AC,
                                H, N.ptr(scratch), 16, B, L, N.stream())
        out = ypre
    N.check(rc, "ap_iir_bwd" if adjoint else "ap_iir_fwd")
    return out


@_on_device
def LPF(new, fs=16000, wp=4000, param=8000, gpass=3, gstop=40, same_size=True, bits=16):
    """Butterworth low-pass (frequency_defense.py:60-100), then the batch-global clamp."""
    x, shape = _flat(new)
    filt = _filter("lpf", fs, wp, param, gpass, gstop)
    return _IIRFn.apply(x, filt, int(bits)).view(shape)


@_on_device
def BPF(new, fs=16000, wp=[300, 4000], param=[50, 8000], gpass=3, gstop=40, same_size=True, bits=16):
    """Butterworth band-pass (frequency_defense.py:102-141), then the batch-global clamp."""
    x, shape = _flat(new)
    filt = _filter("bpf", fs, tuple(wp), tuple(param), gpass, gstop)
    return _IIRFn.apply(x, filt, int(bits)).view(shape)


# --------------------------------------------------------------------------------------------------------- dispatch
class _Dispatch:
    """One defense selected by name.  ``_OPS`` maps each accepted ``defense_type`` to (op, display name,
    whether the call's extra positional arguments reach the op); any other type is refused when called or named,
    with the reference's message."""
    _OPS = {}

    def __init__(self, defense_type: str, *_unused) -> None:
        self.defense_type = defense_type

    def _entry(self):
        entry = self._OPS.get(self.defense_type)
        if entry is None:
            raise NotImplementedError(f"Unknown defense type: {self.defense_type}!")
        return entry

    def __call__(self, x, *args):
        op, _, forwards_args = self._entry()
        return op(x, *args) if forwards_args else op(x)

    def _get_name(self, *_unused):
        return self._entry()[1]


class TimeDomainDefense(_Dispatch):
    """The dispatch of time_defense.py:8-37: AT / AS / MS at their defaults (extra call arguments are ignored there)."""
    _OPS = {"AT": (AT, "Audio_Turbulence", False), "AS": (AS, "Average_Smoothing", False),
            "MS": (MS, "Median_Smoothing", False)}


class FreqDomainDefense(_Dispatch):
    """The dispatch of frequency_defense.py:7-34: DS / LPF / BPF, extra call arguments passed on positionally."""
    _OPS = {"DS": (DS, "Down_Sampling", True), "LPF": (LPF, "Low_Pass_Filter", True),
            "BPF": (BPF, "Band_Pass_Filter", True)}
