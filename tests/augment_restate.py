"""numpy / torch restatements of the speech-commands train pipeline (train_speech_commands.py:60-68; transforms/transforms_wav.py:
34-78, transforms/transforms_stft.py:14-114) behind ap_augment.hip: the four stages and the whole pipeline.  Every function works in
the dtype of its input, so the float64 call is the reference and the float32 call measures what float32 arithmetic alone costs --
the bar of the GPU tests is 4 x that.  librosa is restated, not imported: stft(n_fft=2048, hop_length=512), core.phase_vocoder,
filters.mel and power_to_db(ref=np.max).  The vocoder keeps its phase accumulator wrapped to [-pi, pi] and applies the expected
advance pi k / 2 as k mod 4 quarter turns; ``wrapped=False`` is librosa's own running sum, which in float32 loses 1e-2 of max |D|.
Per-lane STFTs are librosa's [1025 bins, frames]; ``device_layout`` gives the kernels' [lane][frame][bin][re, im].
Test infrastructure only; the input builders live here too, so the CPU and GPU tests see the same numbers."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from audiopure_amd import synth
from audiopure_amd.transforms.augment import draw_augment

import frontend_restate as FR

NFFT, HOP, NBIN = 2048, 512, 1025
# min |D| / max |D| of the inputs' STFTs the GPU tests assume.  A float32 STFT is off by about 1e-7 of max |D|, so the phase of a bin
# at ratio r is off by 1e-7 / r rad; at r >= 1e-5 that stays under 1e-2 rad, far from turning a phase difference across the
# vocoder's wrap at +-pi.  (Typical per clip: 1e-3; the smallest of all the clips used here: 2.5e-5.)
COND_FLOOR = 1e-5
MARGIN = 4.0               # the GPU bar: 4 x the float32 evaluation's own error


def clips(B, L, seed=21):
    """synth.waveforms clips [B, L], float32"""
    return synth.waveforms(B, L, seed=seed)[:, 0].copy()


def background(n_bg, L=16000, seed=22):
    """synth.noise as the background table [n_bg, L], float32"""
    return synth.noise(0, n_bg, L, seed=seed)[:, 0].copy()


def _rt(a):
    return np.zeros(0, dtype=a.dtype).real.dtype.type


# ---- stage 1: ChangeAmplitude, ChangeSpeedAndPitchAudio, FixAudioLength --------------------------------------------------------
def aug_wave(x, length, amp, speed_applied, speed_fac, L_out, ref_casts=False):
    """x: 1-D, at least `length` samples.  np.interp on xp = 0 .. length-1 written out: slope times offset plus the left value, a
    position past length-1 takes the last sample.  ref_casts: round where the reference rounds to float32 (the float32 product
    with the amplitude, transforms_wav.py:60, and .astype(np.float32) after np.interp, :77) -- what the golden file holds."""
    rt = _rt(x)
    s = x[:length]
    if ref_casts:
        s = (s.astype(np.float32) * np.float32(amp)).astype(rt)
    else:
        s = s * rt(amp)
    if speed_applied:
        pos = np.arange(0, length, speed_fac)
        if length < 2:
            v = np.full(len(pos), s[0], dtype=rt)
        else:
            i = np.floor(pos).astype(np.int64)
            i0 = np.minimum(i, length - 2)
            v = (s[i0 + 1] - s[i0]) * (pos - i0).astype(rt) + s[i0]
            v = np.where(i >= length - 1, s[length - 1], v)
        s = v.astype(np.float32).astype(rt) if ref_casts else v.astype(rt)
    out = np.zeros(L_out, dtype=rt)
    n = min(L_out, len(s))
    out[:n] = s[:n]
    return out


# ---- stage 2: ToSTFT -------------------------------------------------------------------------------------------------------------
def stft(x, pad_mode="constant"):
    """librosa.stft(x, n_fft=2048, hop_length=512) of a 1-D array: [1025, 1 + L // 512] complex of x's precision"""
    t = torch.from_numpy(np.ascontiguousarray(x))[None]
    w = F.pad(t[None], (NFFT // 2, NFFT // 2), mode=pad_mode)[0]
    frames = w.unfold(1, NFFT, HOP)
    n = torch.arange(NFFT, dtype=torch.float64)
    win = (0.5 - 0.5 * torch.cos(2 * math.pi * n / NFFT)).to(t.dtype)
    return torch.fft.rfft(frames * win, dim=-1)[0].T.contiguous().numpy()


# ---- stage 3: StretchAudioOnSTFT, TimeshiftAudioOnSTFT, FixSTFTDimension ----------------------------------------------------------
def phase_vocoder(D, rate, wrapped=True):
    """librosa.core.phase_vocoder(D, rate, hop_length=512): D [1025, F] -> [1025, len(np.arange(0, F, rate))]"""
    rt = _rt(D)
    nb, nf = D.shape
    steps = np.arange(0, nf, rate)
    Dp = np.pad(D, ((0, 0), (0, 2)))
    k = np.arange(nb)
    if wrapped:
        phi = (k % 4).astype(rt) * rt(math.pi / 2)
    else:
        phi = np.linspace(0, np.pi * HOP, nb).astype(rt)
    two_pi = rt(2 * math.pi)
    acc = np.angle(Dp[:, 0]).astype(rt)
    out = np.zeros((nb, len(steps)), dtype=D.dtype)
    for t, s in enumerate(steps):
        i = int(math.floor(s))
        alpha = rt(s - i)
        c0, c1 = Dp[:, i], Dp[:, i + 1]
        mag = (rt(1) - alpha) * np.abs(c0) + alpha * np.abs(c1)
        out[:, t].real, out[:, t].imag = mag * np.cos(acc), mag * np.sin(acc)
        d = np.angle(c1) - np.angle(c0) - phi
        d = d - two_pi * np.round(d / two_pi)
        acc = acc + (phi + d)
        if wrapped:
            acc = acc - two_pi * np.round(acc / two_pi)
        assert acc.dtype == rt and mag.dtype == rt
    return out


def shift_fix(S, shift, n_frames):
    """TimeshiftAudioOnSTFT's pad-and-cut (transforms_stft.py:60-67) then FixSTFTDimension to n_frames columns (:89-98)"""
    a, b = -min(0, shift), max(0, shift)
    S = np.pad(S, ((0, 0), (a, b)), "constant")
    S = S[:, b:] if a == 0 else S[:, 0:-a]
    if S.shape[1] > n_frames:
        S = S[:, :n_frames]
    elif S.shape[1] < n_frames:
        S = np.pad(S, ((0, 0), (0, n_frames - S.shape[1])), "constant")
    return S


def vocoder_shift(D, stretch_applied, rate, shift, wrapped=True):
    S = phase_vocoder(D, rate, wrapped) if stretch_applied else D
    return shift_fix(S, int(shift), D.shape[1])


# ---- stage 4: AddBackgroundNoiseOnSTFT, ToMelSpectrogramFromSTFT ------------------------------------------------------------------
def mel_basis(n_mels):
    """librosa.filters.mel(sr=16000, n_fft=2048, n_mels): float64 [n_mels, 1025]"""
    return FR.mel_filterbank(n_mels).T.contiguous().numpy()


def mel_db(D, n_mels, noise=None, p=0.0):
    """D (1 - p) + noise p, |.|^2, the Slaney bank, librosa.power_to_db(ref=np.max): [n_mels, F] of D's precision"""
    rt = _rt(D)
    if noise is not None:
        D = D * rt(1 - p) + noise * rt(p)
    s = mel_basis(n_mels).astype(rt) @ (np.abs(D) ** 2)
    db = rt(10) * np.log10(np.maximum(s, rt(1e-10)))
    return np.maximum(db - db.max(), rt(-80))


# ---- the whole pipeline ----------------------------------------------------------------------------------------------------------
def lane_inputs(samples, bg, d):
    """per lane the source waveform: a clip's row of `samples` [B, L_max], a background lane's row of `bg`"""
    return [samples[i] if i < d.n else bg[d.source[i]] for i in range(d.lanes)]


def pipeline(samples, bg, d, n_mels=32, pad_mode="constant", L_out=16000, dtype=np.float64, wrapped=True, ref_casts=False):
    """-> dict(wave [N, L_out], stft [N, 1025, F], stretched [N, 1025, F], mel [B, n_mels, F]) in `dtype`, N lanes, B clips"""
    n_frames = 1 + L_out // HOP
    wave, D, S = [], [], []
    for i, x in enumerate(lane_inputs(samples, bg, d)):
        w = aug_wave(np.asarray(x).astype(dtype), int(d.length[i]), d.amp[i], bool(d.speed_applied[i]), float(d.speed_fac[i]), L_out, ref_casts)
        if d.speed_applied[i]:
            assert len(np.arange(0, int(d.length[i]), float(d.speed_fac[i]))) == d.n_interp[i]
        wave.append(w)
        D.append(stft(w, pad_mode))
        S.append(vocoder_shift(D[-1], bool(d.stretch_applied[i]), float(d.rate[i]), int(d.shift[i]), wrapped))
        assert S[-1].shape == (NBIN, n_frames)
    mel = [mel_db(S[b], n_mels, S[d.noise_lane[b]] if d.noise_lane[b] >= 0 else None, float(d.p[b])) for b in range(d.n)]
    return dict(wave=np.stack(wave), stft=np.stack(D), stretched=np.stack(S), mel=np.stack(mel))


def device_layout(D):
    """[N, 1025, F] complex -> float32 [N, F, 1025, 2], what ap_stft writes and the later kernels read"""
    D = np.ascontiguousarray(np.swapaxes(D, 1, 2)).astype(np.complex64)
    return np.stack([D.real, D.imag], axis=-1).astype(np.float32)


def from_device_layout(a):
    """float32 [N, F, 1025, 2] -> complex128 [N, 1025, F]"""
    a = np.asarray(a, dtype=np.float64)
    return np.swapaxes(a[..., 0] + 1j * a[..., 1], 1, 2)


def conditioning(D):
    """min |D| / max |D| over the frames of one STFT that hold signal"""
    m = np.abs(D)
    live = m.max(axis=0) > 0
    return float(m[:, live].min() / m.max()) if live.any() else float("inf")


def err_of_max(got, ref):
    """max |got - ref| / max |ref| (absolute where ref is all zero)"""
    got, ref = np.asarray(got), np.asarray(ref)
    top = float(np.abs(ref).max())
    return float(np.abs(got - ref).max()) / (top if top > 0 else 1.0)


def table(n, **cols):
    """hand-made draws for n lanes without noise (the per-kernel tests): missing columns take the not-applied value"""
    from audiopure_amd.transforms.augment import AugmentDraws
    z = lambda dt, v=0: np.full(n, v, dtype=dt)
    length = np.asarray(cols.get("length", z(np.int32, 16000)), dtype=np.int32)
    speed_fac = np.asarray(cols.get("speed_fac", z(np.float64, 1.0)), dtype=np.float64)
    speed_applied = np.asarray(cols.get("speed_applied", speed_fac != 1.0), dtype=np.bool_)
    rate = np.asarray(cols.get("rate", z(np.float64, 1.0)), dtype=np.float64)
    stretch_applied = np.asarray(cols.get("stretch_applied", rate != 1.0), dtype=np.bool_)
    n_frames = cols.get("n_frames", 32)
    n_interp = np.asarray([len(np.arange(0, int(l), f)) if a else int(l) for l, f, a in zip(length, speed_fac, speed_applied)], dtype=np.int32)
    n_out = np.asarray([len(np.arange(0, n_frames, r)) if a else n_frames for r, a in zip(rate, stretch_applied)], dtype=np.int32)
    amp = np.asarray(cols.get("amp", z(np.float32, 1.0)), dtype=np.float32)
    shift = np.asarray(cols.get("shift", z(np.int32)), dtype=np.int32)
    nc = cols.get("n_clips", n)
    return AugmentDraws(n=nc, source=np.asarray(cols.get("source", np.arange(n)), dtype=np.int64), length=length, amp_applied=amp != 1.0, amp=amp,
                        speed_applied=speed_applied, speed_fac=speed_fac, n_interp=n_interp, stretch_applied=stretch_applied, rate=rate,
                        n_out=n_out, shift_applied=shift != 0, shift=shift,
                        noise_applied=np.asarray(cols.get("noise_lane", z(np.int32, -1)[:nc])) >= 0,
                        noise_lane=np.asarray(cols.get("noise_lane", z(np.int32, -1)[:nc]), dtype=np.int32),
                        p=np.asarray(cols.get("p", z(np.float64)[:nc]), dtype=np.float64))


# ---- the golden items (tests/golden/make_golden_aug.py records the reference's own classes on these) -----------------------------------
GOLDEN_N_BG = 3
GOLDEN_LENGTHS = (16000, 9000, 19000, 16000, 12345, 16000, 16000, 14000)
GOLDEN_STFT_FRAMES = (0, 15, 31)


def golden_inputs():
    """(samples [8, 19000] with GOLDEN_LENGTHS valid each, background [3, 16000])"""
    x = clips(len(GOLDEN_LENGTHS), max(GOLDEN_LENGTHS), seed=23)
    for i, n in enumerate(GOLDEN_LENGTHS):
        x[i, n:] = 0.0
    return x, background(GOLDEN_N_BG)


def golden_draws(seed, length):
    """the draws of ONE dataset item under random.seed(seed)"""
    import random
    return draw_augment(random.Random(seed), 1, GOLDEN_N_BG, [length])


def merge_draws(items):
    """one table for a batch out of per-item draws: the clips first, then the background lanes in item order"""
    from audiopure_amd.transforms.augment import AugmentDraws
    n = len(items)
    lane_cols = ["length", "amp_applied", "amp", "speed_applied", "speed_fac", "n_interp", "stretch_applied", "rate", "n_out", "shift_applied", "shift"]
    bgs = [d for d in items if d.lanes > 1]
    cat = lambda c: np.concatenate([getattr(d, c)[:1] for d in items] + [getattr(d, c)[1:] for d in bgs])
    source = np.concatenate([np.arange(n, dtype=np.int64)] + [d.source[1:] for d in bgs])
    noise_lane, k = [], n
    for d in items:
        noise_lane.append(k if d.lanes > 1 else -1)
        k += d.lanes > 1
    return AugmentDraws(n=n, source=source, noise_applied=np.concatenate([d.noise_applied for d in items]),
                        noise_lane=np.asarray(noise_lane, dtype=np.int32), p=np.concatenate([d.p for d in items]),
                        **{c: cat(c) for c in lane_cols})


# ---- the cases of the GPU tests (the CPU tests check their conditioning and that the bar tells the two accumulators apart) ----------
WAVE_L_MAX, WAVE_L_OUT = 19000, 16000
# (length, speed factor or None, amplitude): stretched and padded, compressed and padded, stretched and cut, the copies; lane 0's last
# position lies in (len - 1, len)
WAVE_LANES = [(9000, 1 / 1.2, 0.7), (16000, 1.25, 1.0), (19000, 1 / 1.15, 1.1), (9000, 1.25, 0.93), (16000, None, 0.7), (19000, None, 1.0),
              (9000, None, 1.0), (16000, 1 / 1.2, 1.0)]


def wave_case():
    x = clips(len(WAVE_LANES), WAVE_L_MAX, seed=24)
    t = table(len(WAVE_LANES), length=[l for l, _, _ in WAVE_LANES], speed_fac=[f or 1.0 for _, f, _ in WAVE_LANES],
              speed_applied=[f is not None for _, f, _ in WAVE_LANES], amp=[a for _, _, a in WAVE_LANES])
    return x, t


# (rate or None, shift) per lane.  F = 32: 0.8 with +8 keeps steps 8..39, whose last reads the padded columns; 1.2 has 27 steps; 1.0
# applied has alpha = 0 throughout; the copies at -8, +8, 0.  F = 8 (L = 4000): a copy shifted by +-8 is empty.
VOCODER_LANES = {32: [(0.8, 8), (1.2, 0), (1.0, 0), (0.9137, 0), (None, -8), (None, 8), (None, 0), (1.2, -8)],
                 8: [(None, 8), (None, -8), (0.8, 0), (1.2, 3), (0.8, 8)]}


def vocoder_case(n_frames):
    """(D complex64 [N, 1025, F]: float32 STFTs of clips -- the input of both sides --, table)"""
    lanes = VOCODER_LANES[n_frames]
    L = (n_frames - 1) * HOP + (128 if n_frames == 32 else 416)              # 16000, 4000
    x = clips(len(lanes), L, seed=25)
    D = np.stack([stft(v) for v in x])
    assert D.dtype == np.complex64 and D.shape[2] == n_frames
    t = table(len(lanes), length=[L] * len(lanes), rate=[r or 1.0 for r, _ in lanes], stretch_applied=[r is not None for r, _ in lanes],
              shift=[s for _, s in lanes], n_frames=n_frames)
    return D, t


def vocoder_errors(D, t, wrapped):
    """(error of the float32 evaluation against float64 on the complex values, on the magnitudes; of max |D| over all lanes)"""
    top = float(np.abs(D).max())
    ec = em = 0.0
    for i in range(len(D)):
        ref = vocoder_shift(D[i].astype(np.complex128), t.stretch_applied[i], t.rate[i], t.shift[i])
        got = vocoder_shift(D[i], t.stretch_applied[i], t.rate[i], t.shift[i], wrapped)
        assert got.dtype == np.complex64
        ec, em = max(ec, float(np.abs(got - ref).max()) / top), max(em, float(np.abs(np.abs(got) - np.abs(ref)).max()) / top)
    return ec, em
