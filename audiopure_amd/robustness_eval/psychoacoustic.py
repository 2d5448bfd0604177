"""Native psychoacoustic masker and imperceptibility loss of the white-box attack's second stage (Qin et al. 2019).

The reference computes the masking threshold with ``PsychoacousticMasker`` (robustness_eval/white_box_attack.py:36-273),
on the host, one clip and one frame at a time, through librosa, and the stage-2 hinge loss with ``torch.stft``
(:610-710).  Here both run on the HIP kernels of ap_psy.hip: ``ap_psy_threshold`` (maskers, filters, global threshold and
its stabilised form) and ``ap_psy_loss_grad`` (the hinge loss and its gradient).  The device tables the kernels read --
the analysis window, the bark scale and the absolute threshold of hearing -- are built here in float64 with the
reference's formulas.

Departures, documented in INTEGRATION.md 1b: window sizes other than 2048 and clips shorter than one window raise (there is
no kernel for them); where the perturbation's spectrum is exactly 0 the gradient is 0 (the reference's ``sqrt`` backward
gives NaN there).  CPU tensors raise: there is no CPU path.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from .. import _native as N

WINDOW = 2048
NBINS = WINDOW // 2 + 1


def _on_device(fn):
    inner = N.on_device(lambda _self, *a, **k: fn(*a, **k))

    def wrapper(*a, **k):
        return inner(None, *a, **k)
    wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
    return wrapper


def hann_periodic(n: int) -> np.ndarray:
    """``scipy.signal.get_window("hann", n, fftbins=True)`` in float64, with scipy's own operations (a general cosine window
    on ``linspace(-pi, pi, n + 1)``, truncated), so the values are the same bits."""
    fac = np.linspace(-np.pi, np.pi, n + 1)
    w = np.zeros(n + 1)
    w += 0.5 * np.cos(0 * fac)
    w += 0.5 * np.cos(1 * fac)
    return w[:-1]


def _frames(L: int, hop: int) -> int:
    return 1 + (L - WINDOW) // hop


class PsychoacousticMasker:
    """Psychoacoustic model of Lin and Abdulla (2015) with the simplifications of Qin et al. (2019), as the reference's
    ``PsychoacousticMasker``: same constructor, properties and ``calculate_threshold_and_psd_maximum`` contract, computed
    on the device.  Only ``window_size = 2048`` has a kernel; any other size raises here."""

    def __init__(self, window_size: int = 2048, hop_size: int = 512, sample_rate: int = 16000) -> None:
        if window_size != WINDOW:
            raise ValueError(f"PsychoacousticMasker: window_size {window_size} has no native kernel (only {WINDOW})")
        if not 1 <= hop_size <= WINDOW:
            raise ValueError(f"PsychoacousticMasker: hop_size {hop_size} outside [1, {WINDOW}]")
        self._window_size = window_size
        self._hop_size = hop_size
        self._sample_rate = sample_rate
        self._fft_frequencies = None
        self._bark = None
        self._absolute_threshold_hearing = None
        self._tables = {}                                   # device index -> fp64 [AP_PSY_TABLE_ELEMS]

    @property
    def window_size(self) -> int:
        return self._window_size

    @property
    def hop_size(self) -> int:
        return self._hop_size

    @property
    def sample_rate(self) -> int:
        return self._sample_rate

    @property
    def fft_frequencies(self) -> np.ndarray:
        """Frequencies of the 1025 bins in Hz (float64)."""
        if self._fft_frequencies is None:
            self._fft_frequencies = np.linspace(0, self.sample_rate / 2, self.window_size // 2 + 1)
        return self._fft_frequencies

    @property
    def bark(self) -> np.ndarray:
        """Bark scale of the bin frequencies: 13 atan(0.00076 f) + 3.5 atan((f / 7500)^2), float64."""
        if self._bark is None:
            f = self.fft_frequencies
            self._bark = 13 * np.arctan(0.00076 * f) + 3.5 * np.arctan(np.square(f / 7500.0))
        return self._bark

    @property
    def absolute_threshold_hearing(self) -> np.ndarray:
        """Absolute threshold of hearing in dB at the bin frequencies (float64); -inf outside 20 Hz .. 20 kHz, so that every
        masker there passes the ATH filter and the global threshold stays finite."""
        if self._absolute_threshold_hearing is None:
            f = self.fft_frequencies
            inside = (f >= 20) & (f <= 2e4)
            khz = f[inside] * 0.001
            ath = np.full(f.shape, -np.inf)
            ath[inside] = 3.64 * pow(khz, -0.8) - 6.5 * np.exp(-0.6 * np.square(khz - 3.3)) + 0.001 * pow(khz, 4) - 12
            self._absolute_threshold_hearing = ath
        return self._absolute_threshold_hearing

    def tables(self, device) -> torch.Tensor:
        """The kernels' fp64 table on ``device``: analysis window [2048], bark [1025], ATH [1025] (include/audiopure.h)."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        t = self._tables.get(idx)
        if t is None:
            host = np.concatenate([hann_periodic(WINDOW), self.bark, self.absolute_threshold_hearing])
            t = self._tables[idx] = torch.from_numpy(host).to(torch.device("cuda", idx))
        return t

    def _clips(self, audio: torch.Tensor) -> torch.Tensor:
        if audio.dim() == 3 and audio.shape[1] == 1:
            audio = audio[:, 0]
        if audio.dim() != 2:
            raise ValueError(f"PsychoacousticMasker: expected [B, L] or [B, 1, L], got {tuple(audio.shape)}")
        if audio.shape[-1] < WINDOW:
            raise ValueError(f"PsychoacousticMasker: clips of {audio.shape[-1]} samples are shorter than one window ({WINDOW})")
        if not audio.is_cuda:
            raise N.NativeError("PsychoacousticMasker needs device (cuda/HIP) tensors; there is no CPU path")
        return audio.float().contiguous()

    def threshold_and_psd_maximum(self, audio: torch.Tensor, db: bool = False):
        """Batched masking threshold of ``audio`` [B, L] or [B, 1, L] on the device.

        Returns ``(thr_stab [B, 1025, F], psd_max_stab [B])``, the stabilised forms 10^(0.1 threshold) and 10^(0.1 psd_max)
        that ``AudioAttack._stabilized_threshold_and_psd_maximum`` (:692-715) forms; with ``db=True`` also the threshold in
        dB [B, 1025, F] and psd_max in dB [B]."""
        x = self._clips(audio)
        return _threshold(x, self.tables(x.device), self.hop_size, db)

    def calculate_threshold_and_psd_maximum(self, audio: np.ndarray) -> Tuple[np.ndarray, np.float32]:
        """The reference's numpy contract (:61-86): ``audio`` of shape (L,) -> the global masking threshold (1025, F) in
        dB and the clip's PSD maximum, both fp32 as the reference returns them (its PSD is fp32).  Runs on the current HIP
        device."""
        a = np.asarray(audio)
        if a.ndim != 1:
            raise ValueError(f"calculate_threshold_and_psd_maximum: expected shape (L,), got {a.shape}")
        x = torch.from_numpy(a.astype(np.float32)).to(torch.device("cuda", torch.cuda.current_device()))[None]
        _, _, thr, pmax = self.threshold_and_psd_maximum(x, db=True)
        return thr[0].cpu().numpy(), np.float32(pmax[0].item())


@_on_device
def _threshold(x: torch.Tensor, tables: torch.Tensor, hop: int, db: bool):
    B, L = x.shape
    F = _frames(L, hop)
    lib = N.lib()
    scratch = torch.empty(lib.ap_psy_scratch_elems(WINDOW, hop, B, L), dtype=torch.float32, device=x.device)
    thr = torch.empty(B, NBINS, F, dtype=torch.float32, device=x.device)
    pmax = torch.empty(B, dtype=torch.float32, device=x.device)
    thr_db = torch.empty_like(thr) if db else None
    pmax_db = torch.empty_like(pmax) if db else None
    N.check(lib.ap_psy_threshold(N.ptr(x), tables.data_ptr(), N.ptr(thr), N.ptr(thr_db), N.ptr(pmax), N.ptr(pmax_db),
                                 N.ptr(scratch), WINDOW, hop, B, L, N.stream()), "ap_psy_threshold")
    return (thr, pmax, thr_db, pmax_db) if db else (thr, pmax)


@_on_device
def masking_threshold_loss_and_grad(delta: torch.Tensor, thr_stab: torch.Tensor, psd_max_stab: torch.Tensor,
                                    hop_size: int = 512) -> Tuple[torch.Tensor, torch.Tensor]:
    """Hinge loss of the perturbation's PSD against the stabilised masking threshold and its gradient
    (``AudioAttack._loss_gradient_masking_threshold``, :610-690): ``delta`` [B, L] or [B, 1, L], ``thr_stab``
    [B, 1025, F], ``psd_max_stab`` [B] -> ``(grad [B, 1, L], loss [B])``, both fp32 device tensors."""
    if delta.dim() == 3 and delta.shape[1] == 1:
        delta = delta[:, 0]
    if delta.dim() != 2:
        raise ValueError(f"masking_threshold_loss_and_grad: expected [B, L] or [B, 1, L], got {tuple(delta.shape)}")
    B, L = delta.shape
    if L < WINDOW:
        raise ValueError(f"masking_threshold_loss_and_grad: clips of {L} samples are shorter than one window ({WINDOW})")
    F = _frames(L, hop_size)
    if tuple(thr_stab.shape) != (B, NBINS, F) or tuple(psd_max_stab.reshape(-1).shape) != (B,):
        raise ValueError(f"masking_threshold_loss_and_grad: thresholds {tuple(thr_stab.shape)} / {tuple(psd_max_stab.shape)} "
                         f"do not match B = {B}, {NBINS} bins, F = {F}")
    x = delta.detach().float().contiguous()
    thr = thr_stab.detach().float().contiguous()
    pm = psd_max_stab.detach().reshape(-1).float().contiguous()
    lib = N.lib()
    scratch = torch.empty(lib.ap_psy_scratch_elems(WINDOW, hop_size, B, L), dtype=torch.float32, device=x.device)
    grad = torch.empty(B, 1, L, dtype=torch.float32, device=x.device)
    loss = torch.empty(B, dtype=torch.float32, device=x.device)
    N.check(lib.ap_psy_loss_grad(N.ptr(x), N.ptr(thr), N.ptr(pm), N.ptr(grad), N.ptr(loss), N.ptr(scratch), WINDOW,
                                 hop_size, B, L, N.stream()), "ap_psy_loss_grad")
    return grad, loss
