#!/usr/bin/env python3
"""The REFERENCE's own train-time transform classes (transforms/transforms_wav.py, transforms/transforms_stft.py, imported from the
reference checkout; build container only) and its BackgroundNoiseDataset.__getitem__ on the seeded items of tests/augment_restate.py,
under a stand-in ``librosa`` module whose ``stft``, ``core.phase_vocoder``, ``filters.mel`` and ``power_to_db`` are the float64
restatements of that file (librosa itself is not installed).  The dataset object is made with ``__new__`` plus attributes, so its
file-reading ``__init__`` is skipped and its ``__getitem__`` is the reference's.  This pins the draw order and the pad / cut / interp
index semantics to the reference's code, not to its librosa.

Per item the seed is searched (with draw_augment) so that the eight items between them have every transform applied and not
applied, on clips and on background clips, and five noise mixes.  Stored: the seed, the flags, ``data['mel_spectrogram']`` and three
columns of ``data['stft']`` after the noise step.  Results only.

    python tests/golden/make_golden_aug.py
"""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("AUDIOPURE_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))    # the reference checkout
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import augment_restate as R                                             # noqa: E402


def _stft(y, n_fft=2048, hop_length=None, **kw):
    assert n_fft == R.NFFT and hop_length == R.HOP and not kw
    return R.stft(np.asarray(y, dtype=np.float64))


def _phase_vocoder(D, rate=None, hop_length=None):
    assert hop_length == R.HOP
    return R.phase_vocoder(D, rate)


def _mel(sr=None, n_fft=None, n_mels=128):
    assert sr == 16000 and n_fft == R.NFFT
    return R.mel_basis(n_mels)


def _power_to_db(S, ref=1.0, amin=1e-10, top_db=80.0):
    ref_value = ref(S) if callable(ref) else ref
    log_spec = 10.0 * np.log10(np.maximum(amin, S)) - 10.0 * np.log10(np.maximum(amin, ref_value))
    return np.maximum(log_spec, log_spec.max() - top_db)


librosa = types.ModuleType("librosa")
librosa.core, librosa.filters = types.ModuleType("librosa.core"), types.ModuleType("librosa.filters")
librosa.stft, librosa.power_to_db = _stft, _power_to_db
librosa.core.phase_vocoder, librosa.filters.mel = _phase_vocoder, _mel
sys.modules.update({"librosa": librosa, "librosa.core": librosa.core, "librosa.filters": librosa.filters})
sys.path.insert(0, REF)

import transforms as T                                                  # noqa: E402  (reference package)
import importlib.util                                                   # noqa: E402

_spec = importlib.util.spec_from_file_location("ref_sc_dataset", os.path.join(REF, "datasets", "sc_dataset.py"))   # (reference module)
_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mod)
BackgroundNoiseDataset = _mod.BackgroundNoiseDataset


class Compose:                                                          # torchvision's, which is not installed
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


# train_speech_commands.py:60-63
data_aug_transform = Compose([T.ChangeAmplitude(), T.ChangeSpeedAndPitchAudio(), T.FixAudioLength(), T.ToSTFT(), T.StretchAudioOnSTFT(),
                              T.TimeshiftAudioOnSTFT(), T.FixSTFTDimension()])
samples, bg = R.golden_inputs()
bg_dataset = BackgroundNoiseDataset.__new__(BackgroundNoiseDataset)
bg_dataset.samples, bg_dataset.sample_rate, bg_dataset.transform, bg_dataset.path = bg, 16000, data_aug_transform, ""
add_bg_noise = T.AddBackgroundNoiseOnSTFT(bg_dataset)
train_feature_transform = Compose([T.ToMelSpectrogramFromSTFT(n_mels=32), T.DeleteSTFT(), T.ToTensor("mel_spectrogram", "input")])

# (amp, speed, stretch, shift, noise) of the eight clips; the background clips take what their draws give
WANT = [(1, 1, 1, 1, 1), (0, 0, 0, 0, 0), (1, 0, 1, 0, 1), (0, 1, 0, 1, 0), (0, 1, 1, 0, 1), (1, 0, 0, 1, 0), (0, 0, 1, 1, 1), (1, 1, 0, 0, 1)]


def flags(d, lane):
    return (int(d.amp_applied[lane]), int(d.speed_applied[lane]), int(d.stretch_applied[lane]), int(d.shift_applied[lane]))


out, seed, bg_flags = {}, 0, []
for i, (length, want) in enumerate(zip(R.GOLDEN_LENGTHS, WANT)):
    while True:
        d = R.golden_draws(seed, length)
        if flags(d, 0) + (int(d.noise_applied[0]),) == want:
            break
        seed += 1
    if d.lanes > 1:
        bg_flags.append(flags(d, 1))
    random.seed(seed)
    data = {"samples": samples[i, :length].copy(), "sample_rate": 16000}
    data = add_bg_noise(data_aug_transform(data))
    stft = data["stft"]
    data = train_feature_transform(data)
    mel = np.asarray(data["mel_spectrogram"], dtype=np.float64)
    assert mel.shape == (32, 32) and stft.shape == (1025, 32) and "stft" not in data
    out[f"{i}/seed"], out[f"{i}/flags"] = np.int64(seed), np.asarray(want, dtype=np.int64)
    out[f"{i}/mel"] = mel
    out[f"{i}/stft"] = np.ascontiguousarray(stft[:, list(R.GOLDEN_STFT_FRAMES)]).astype(np.complex128)
    print(f"item {i}: length {length:5d} seed {seed:4d} flags {want} lanes {d.lanes} mel min {mel.min():.2f}")
    seed += 1
for j in range(4):
    assert {f[j] for f in bg_flags} == {0, 1}, ("background clips do not cover flag", j, bg_flags)
path = os.path.join(HERE, "golden_aug_v1.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
