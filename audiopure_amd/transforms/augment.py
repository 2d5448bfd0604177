"""Train-time augmentation and mel features of the speech-commands classifiers, batched on the device.

``SpeechCommandsAugment`` replaces the per-sample numpy / librosa pipeline that ``train_speech_commands.py:60-68`` runs in its
DataLoader workers::

    ChangeAmplitude -> ChangeSpeedAndPitchAudio -> FixAudioLength -> ToSTFT -> StretchAudioOnSTFT -> TimeshiftAudioOnSTFT
    -> FixSTFTDimension -> AddBackgroundNoiseOnSTFT -> ToMelSpectrogramFromSTFT -> DeleteSTFT -> ToTensor

(``transforms/transforms_wav.py:34-78``, ``transforms/transforms_stft.py:14-114``; the background clip goes through the first seven
steps with its own draws).  ``draw_augment`` draws every random number on the host, in the reference's own order, into per-lane
tables; four HIP kernels (``ap_augment.hip``) then take a padded batch of waveforms to ``[B, n_mels, frames]`` mel-dB with no host
round trip between the stages.  A *lane* is one clip or one background clip.

Not built: the wave-domain ``StretchAudio`` / ``TimeshiftAudio`` / ``AddBackgroundNoise`` (not in the training ``Compose``),
``LoadAudio`` (file I/O), ``WeightedRandomSampler``, gradients, and any n_fft but 2048 (hop 512)."""
from __future__ import annotations

import random
from dataclasses import dataclass

import numpy as np
import torch

from .. import _native as N

N_FFT, HOP = 2048, 512
PAD_MODES = {"constant": 0, "reflect": 1}
# the training Compose by class name; LoadAudio may lead it (the dataset keeps that step)
WAVE_STFT_STEPS = ["ChangeAmplitude", "ChangeSpeedAndPitchAudio", "FixAudioLength", "ToSTFT", "StretchAudioOnSTFT", "TimeshiftAudioOnSTFT",
                   "FixSTFTDimension"]
TRAIN_STEPS = WAVE_STFT_STEPS + ["AddBackgroundNoiseOnSTFT", "ToMelSpectrogramFromSTFT", "DeleteSTFT", "ToTensor"]


@dataclass
class AugmentDraws:
    """Per-lane tables of one batch: lanes ``0 .. n-1`` are the clips, the rest the background clips in the order they were drawn.
    ``source``: a clip's own row, a background lane's row of the background table.  ``noise_lane`` / ``p`` are per clip
    (``-1``: no mix)."""
    n: int
    source: np.ndarray
    length: np.ndarray
    amp_applied: np.ndarray
    amp: np.ndarray
    speed_applied: np.ndarray
    speed_fac: np.ndarray
    n_interp: np.ndarray
    stretch_applied: np.ndarray
    rate: np.ndarray
    n_out: np.ndarray
    shift_applied: np.ndarray
    shift: np.ndarray
    noise_applied: np.ndarray
    noise_lane: np.ndarray
    p: np.ndarray

    @property
    def lanes(self) -> int:
        return len(self.source)


def draw_augment(rng, n, n_bg, lengths, amplitude_range=(0.7, 1.1), speed_max_scale=0.2, stretch_max_scale=0.2, max_shift=8,
                 max_percentage=0.45, out_length=16000, bg_length=16000, hop_length=HOP) -> AugmentDraws:
    """The draws of ``n`` consecutive dataset items, from ``rng`` (a ``random.Random`` or the ``random`` module) in the reference's
    order.  Per item, each of the four random transforms calls ``random()`` and, only if that is below 0.5, its ``uniform`` /
    ``randint`` (transforms_wav.py:12-14,57-60,70-76; transforms_stft.py:37-43,55-59); then the noise step calls ``random()`` and, if
    applied, ``random.choice`` on the background dataset -- whose ``__getitem__`` runs the four transforms on the chosen clip, with
    their draws -- and ``uniform(0, max_percentage)`` (transforms_stft.py:78-82).  Every derived count is numpy's own expression."""
    lengths = [int(v) for v in lengths]
    if len(lengths) != n:
        raise ValueError(f"draw_augment: {len(lengths)} lengths for {n} clips")
    n_frames = 1 + out_length // hop_length

    def lane(source, length):
        amp_applied = rng.random() < 0.5
        amp = rng.uniform(*amplitude_range) if amp_applied else 1.0
        speed_applied = rng.random() < 0.5
        speed_fac, n_interp = 1.0, length
        if speed_applied:
            speed_fac = 1.0 / (1 + rng.uniform(-speed_max_scale, speed_max_scale))
            n_interp = len(np.arange(0, length, speed_fac))
        stretch_applied = rng.random() < 0.5
        rate, n_out = 1.0, n_frames
        if stretch_applied:
            rate = 1 + rng.uniform(-stretch_max_scale, stretch_max_scale)
            n_out = len(np.arange(0, n_frames, rate))
        shift_applied = rng.random() < 0.5
        shift = rng.randint(-max_shift, max_shift) if shift_applied else 0
        return (source, length, amp_applied, amp, speed_applied, speed_fac, n_interp, stretch_applied, rate, n_out, shift_applied, shift)

    clips, bgs, noise = [], [], []
    for i in range(n):
        clips.append(lane(i, lengths[i]))
        if rng.random() < 0.5:
            if n_bg < 1:
                raise ValueError("draw_augment: the noise step was drawn but there is no background clip (random.choice on an empty dataset)")
            bgs.append(lane(rng.choice(range(n_bg)), bg_length))        # random.choice's index, then the item's own draws
            noise.append((True, n + len(bgs) - 1, rng.uniform(0, max_percentage)))
        else:
            noise.append((False, -1, 0.0))
    rows = clips + bgs
    col = lambda j, dt: np.asarray([r[j] for r in rows], dtype=dt)
    return AugmentDraws(n=n, source=col(0, np.int64), length=col(1, np.int32), amp_applied=col(2, np.bool_),
                        amp=col(3, np.float64).astype(np.float32),          # float32 samples * python float: a float32 product
                        speed_applied=col(4, np.bool_), speed_fac=col(5, np.float64), n_interp=col(6, np.int32),
                        stretch_applied=col(7, np.bool_), rate=col(8, np.float64), n_out=col(9, np.int32),
                        shift_applied=col(10, np.bool_), shift=col(11, np.int32),
                        noise_applied=np.asarray([v[0] for v in noise], dtype=np.bool_),
                        noise_lane=np.asarray([v[1] for v in noise], dtype=np.int32),
                        p=np.asarray([v[2] for v in noise], dtype=np.float64))


def _flatten(t):
    """the steps of a (nested) Compose, in order"""
    if type(t).__name__ == "Compose" and hasattr(t, "transforms"):
        return [s for u in t.transforms for s in _flatten(u)]
    return [t]


def _match(steps, names, what):
    got = [type(s).__name__ for s in steps]
    for i, want in enumerate(names):
        if i >= len(got) or got[i] != want:
            raise NotImplementedError(f"SpeechCommandsAugment.from_compose: step {i} of {what} is {got[i] if i < len(got) else 'missing'}, "
                                      f"expected {want} (the pipeline of train_speech_commands.py:60-68 is the one built)")
    if len(got) > len(names):
        raise NotImplementedError(f"SpeechCommandsAugment.from_compose: unrecognised step {got[len(names)]} after {names[-1]} in {what}")
    return dict(zip(names, steps))


class SpeechCommandsAugment(torch.nn.Module):
    """``forward(samples [B, L_max], lengths) -> [B, n_mels, 1 + out_length // 512]`` mel-dB (float32, on the device of
    ``samples``), what the training ``Compose`` yields as ``data['input']`` for each of the B clips.  ``bg_samples`` is the
    background table ``[n_bg, bg_length]`` (``BackgroundNoiseDataset.samples``).  Without ``draws`` the module draws from its own
    ``rng`` (``random.Random``; pass a seeded one to reproduce a run).  ``pad_mode``: ``'constant'`` (librosa >= 0.10, what
    ``ToMelSpectrogramDB`` assumes) or ``'reflect'`` (older librosa).  Forward only."""

    def __init__(self, bg_samples, n_mels=32, pad_mode="constant", amplitude_range=(0.7, 1.1), speed_max_scale=0.2,
                 stretch_max_scale=0.2, max_shift=8, max_percentage=0.45, out_length=16000, rng=None):
        super().__init__()
        if pad_mode not in PAD_MODES:
            raise ValueError(f"SpeechCommandsAugment: pad_mode {pad_mode!r}; one of {sorted(PAD_MODES)}")
        bg = torch.as_tensor(np.asarray(bg_samples), dtype=torch.float32)
        if bg.dim() != 2:
            raise ValueError(f"SpeechCommandsAugment: bg_samples must be [n_bg, length], got {tuple(bg.shape)}")
        self.register_buffer("bg_samples", bg.contiguous())
        self.n_mels, self.pad_mode, self.out_length = int(n_mels), pad_mode, int(out_length)
        self.draw_args = dict(amplitude_range=tuple(amplitude_range), speed_max_scale=speed_max_scale, stretch_max_scale=stretch_max_scale,
                              max_shift=max_shift, max_percentage=max_percentage, out_length=self.out_length,
                              bg_length=int(bg.shape[1]), hop_length=HOP)
        self.rng = rng if rng is not None else random.Random()

    @classmethod
    def from_compose(cls, compose, bg_dataset, pad_mode="constant", rng=None):
        """Read the parameters off the reference's transform objects (by class name): ``compose`` is the training ``Compose`` (with
        or without its leading ``LoadAudio``), ``bg_dataset`` the ``BackgroundNoiseDataset`` whose ``transform`` is the first seven
        steps.  A pipeline that is not this one is refused, naming the step."""
        steps = _flatten(compose)
        if steps and type(steps[0]).__name__ == "LoadAudio":
            steps = steps[1:]
        s = _match(steps, TRAIN_STEPS, "the training Compose")
        b = _match(_flatten(bg_dataset.transform), WAVE_STFT_STEPS, "the background dataset's transform")
        for name, attr in (("ChangeAmplitude", "amplitude_range"), ("ChangeSpeedAndPitchAudio", "max_scale"), ("FixAudioLength", "time"),
                           ("ToSTFT", "n_fft"), ("ToSTFT", "hop_length"), ("StretchAudioOnSTFT", "max_scale"), ("TimeshiftAudioOnSTFT", "max_shift")):
            if getattr(s[name], attr) != getattr(b[name], attr):
                raise NotImplementedError(f"SpeechCommandsAugment.from_compose: {name}.{attr} differs between the clips' and the background's transform")
        if (s["ToSTFT"].n_fft, s["ToSTFT"].hop_length) != (N_FFT, HOP):
            raise NotImplementedError(f"SpeechCommandsAugment.from_compose: ToSTFT(n_fft={s['ToSTFT'].n_fft}, hop_length={s['ToSTFT'].hop_length}); "
                                      f"only n_fft={N_FFT}, hop_length={HOP} is built")
        tt = s["ToTensor"]
        if getattr(tt, "normalize", None) is not None or getattr(tt, "np_name", "mel_spectrogram") != "mel_spectrogram":
            raise NotImplementedError("SpeechCommandsAugment.from_compose: ToTensor must take 'mel_spectrogram' without normalize")
        sample_rate = int(getattr(bg_dataset, "sample_rate", 16000))
        if sample_rate != 16000:
            raise NotImplementedError(f"SpeechCommandsAugment.from_compose: sample_rate {sample_rate}; the mel filterbank is built for 16000")
        return cls(bg_dataset.samples, n_mels=s["ToMelSpectrogramFromSTFT"].n_mels, pad_mode=pad_mode,
                   amplitude_range=s["ChangeAmplitude"].amplitude_range, speed_max_scale=s["ChangeSpeedAndPitchAudio"].max_scale,
                   stretch_max_scale=s["StretchAudioOnSTFT"].max_scale, max_shift=s["TimeshiftAudioOnSTFT"].max_shift,
                   max_percentage=s["AddBackgroundNoiseOnSTFT"].max_percentage, out_length=int(s["FixAudioLength"].time * sample_rate), rng=rng)

    def draw(self, lengths) -> AugmentDraws:
        lengths = [int(v) for v in lengths]
        return draw_augment(self.rng, len(lengths), int(self.bg_samples.shape[0]), lengths, **self.draw_args)

    def _check(self, d: AugmentDraws, B, L_max):
        n_bg, nl = int(self.bg_samples.shape[0]), d.lanes
        if d.n != B or nl < B:
            raise ValueError(f"SpeechCommandsAugment: draws for {d.n} clips, batch of {B}")
        if (d.length[:B] < 1).any() or (d.length[:B] > L_max).any():
            raise ValueError(f"SpeechCommandsAugment: a clip length outside [1, {L_max}]")
        if (d.length[B:] != self.bg_samples.shape[1]).any() or (d.source[B:] < 0).any() or (d.source[B:] >= max(n_bg, 1)).any():
            raise ValueError("SpeechCommandsAugment: a background lane outside the background table")
        if (d.n_interp < 0).any() or (d.n_out < 0).any() or not (d.speed_fac > 0).all() or not (d.rate > 0).all():
            raise ValueError("SpeechCommandsAugment: a non-positive factor, rate or count in the draws")
        if ((d.noise_lane != -1) & ((d.noise_lane < B) | (d.noise_lane >= nl))).any():
            raise ValueError("SpeechCommandsAugment: a noise lane that is not a background lane")

    @N.on_device
    def forward(self, samples, lengths, draws=None):
        if samples.dim() != 2:
            raise ValueError(f"SpeechCommandsAugment: samples must be [B, L_max], got {tuple(samples.shape)}")
        if self.bg_samples.device != samples.device:
            raise N.NativeError(f"SpeechCommandsAugment: background table on {self.bg_samples.device}, samples on {samples.device}")
        x = samples.detach().float().contiguous()
        B, L_max = x.shape
        d = draws if draws is not None else self.draw(lengths)
        if [int(v) for v in lengths] != d.length[:B].tolist():
            raise ValueError("SpeechCommandsAugment: the draws were made for other clip lengths")
        self._check(d, B, L_max)
        dev, nl, L_out = x.device, d.lanes, self.out_length
        F = 1 + L_out // HOP
        if nl > B:                                               # the background lanes join the batch, padded to one width
            bg = self.bg_samples.index_select(0, torch.from_numpy(d.source[B:]).to(dev))
            L_in = max(L_max, bg.shape[1])
            lanes = x.new_zeros((nl, L_in))
            lanes[:B, :L_max] = x
            lanes[B:, :bg.shape[1]] = bg
            x, L_max = lanes, L_in
        pad = lambda a, dt: np.concatenate([a.astype(dt), np.zeros(nl - len(a), dtype=dt)])
        ti = torch.from_numpy(np.stack([d.length, d.n_interp, d.speed_applied.astype(np.int32), d.n_out, d.stretch_applied.astype(np.int32),
                                        d.shift, pad(d.noise_lane, np.int32)]).astype(np.int32)).to(dev)
        tf = torch.from_numpy(np.stack([d.amp.astype(np.float32), pad(d.p, np.float32)])).to(dev)
        td = torch.from_numpy(np.stack([d.speed_fac, d.rate]).astype(np.float64)).to(dev)
        wave = torch.empty((nl, L_out), device=dev, dtype=torch.float32)
        stft = torch.empty((2, nl, F, N_FFT // 2 + 1, 2), device=dev, dtype=torch.float32)
        out = torch.empty((B, self.n_mels, F), device=dev, dtype=torch.float32)
        lib, st = N.lib(), N.stream()
        N.check(lib.ap_aug_wave(N.ptr(x), ti[0].data_ptr(), N.ptr(tf[0]), td[0].data_ptr(), ti[1].data_ptr(), ti[2].data_ptr(), N.ptr(wave),
                                nl, L_max, L_out, st), "ap_aug_wave")
        N.check(lib.ap_stft(N.ptr(wave), N.ptr(stft[0]), PAD_MODES[self.pad_mode], nl, L_out, st), "ap_stft")
        N.check(lib.ap_phase_vocoder_shift(N.ptr(stft[0]), N.ptr(stft[1]), td[1].data_ptr(), ti[3].data_ptr(), ti[4].data_ptr(),
                                           ti[5].data_ptr(), nl, F, st), "ap_phase_vocoder_shift")
        N.check(lib.ap_mel_from_stft(N.ptr(stft[1]), ti[6].data_ptr(), N.ptr(tf[1]), N.ptr(out), self.n_mels, B, nl, F, st), "ap_mel_from_stft")
        return out
