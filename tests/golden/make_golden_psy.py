"""Golden vectors of the attack's second, imperceptible stage from the REFERENCE's own code
(robustness_eval/white_box_attack.py, loaded by file path): ``PsychoacousticMasker`` thresholds and PSD maxima, and the
inputs and outputs of ``AudioAttack._loss_gradient_masking_threshold`` at every iteration of a real
``AudioAttack.generate(..., max_iter_2=4)`` run on a tiny CPU model.

Three stand-ins for what is absent or changed in today's images; everything else runs as written:

* ``librosa`` (not installed): ``core.stft`` with ``center=False`` is the framing of the float32 clip, a float64
  ``np.fft.rfft`` of ``window64 * frame``, cast to complex64 -- what librosa does for float32 input.
* ``torch.stft`` without ``return_complex`` raises since torch 2.0: it is patched to
  ``view_as_real(stft(..., return_complex=True))``, the torch 1.x result the reference was written for.
* ``np.sqrt(8.0 / 3.0) * stft_matrix``: the reference pins numpy 1.21, whose value-based casting keeps a float64 scalar
  times a complex64 array in complex64, so its PSD is fp32.  numpy >= 2 promotes the product to complex128; the module's
  ``np`` is given a ``sqrt`` that returns a Python float for a scalar, which numpy >= 2 treats as 1.21 treated the scalar.

Needs scipy and the reference checkout (path as the first argument, or $AUDIOPURE_REFERENCE); writes
tests/golden/golden_psy_v1.npz."""
import importlib.util
import os
import sys
import types

import numpy as np
import scipy.signal as ss
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _librosa():
    def stft(y, n_fft=2048, hop_length=None, win_length=None, window="hann", center=True, **_):
        assert not center and win_length == n_fft
        w = np.asarray(window, dtype=np.float64)
        F = 1 + (len(y) - n_fft) // hop_length
        frames = np.stack([y[f * hop_length:f * hop_length + n_fft] for f in range(F)], axis=1)   # [n_fft, F]
        return np.fft.rfft(w[:, None] * frames, axis=0).astype(np.complex64)

    lib = types.ModuleType("librosa")
    lib.core = types.ModuleType("librosa.core")
    lib.core.stft = stft
    return lib


class _Numpy121(types.ModuleType):
    def __init__(self):
        super().__init__("numpy")

    def __getattr__(self, k):
        return getattr(np, k)

    @staticmethod
    def sqrt(x, *a, **k):
        return float(np.sqrt(x)) if np.isscalar(x) and not a and not k else np.sqrt(x, *a, **k)


class TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.conv = torch.nn.Conv1d(1, 8, 80, stride=16)
        self.fc = torch.nn.Linear(8, 10)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)

    def forward(self, x):
        h = torch.relu(self.conv(x)).mean(-1)
        return torch.log_softmax(self.fc(h), -1)


def load_reference(ref):
    sys.modules.setdefault("librosa", _librosa())
    spec = importlib.util.spec_from_file_location("ref_white_box_attack", os.path.join(ref, "robustness_eval",
                                                                                        "white_box_attack.py"))
    wb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(wb)
    wb.np = _Numpy121()
    return wb


def clips():
    r = np.random.default_rng(7)
    t16 = np.arange(16000) / 16000.0
    t8 = np.arange(8192) / 16000.0
    tones = (0.3 * np.sin(2 * np.pi * 440 * t8) + 0.2 * np.sin(2 * np.pi * 1000 * t8) + 0.1 * np.sin(2 * np.pi * 3150 * t8)
             + 0.01 * r.standard_normal(8192))
    silent = 0.2 * r.standard_normal(8192)
    silent[2048:6656] = 0.0                                   # frames 4 .. 8 all zero
    return {                                                  # name -> (clip, hop, sample rate)
        "noise": ((0.1 * r.standard_normal(16000) + 0.05 * np.sin(2 * np.pi * 700 * t16)).astype(np.float32), 512, 16000),
        "tones": (tones.astype(np.float32), 512, 16000),
        "silent": (silent.astype(np.float32), 512, 16000),
        "hop256": (tones[::-1].copy().astype(np.float32), 256, 16000),
        "sr44k": ((0.2 * r.standard_normal(8192)).astype(np.float32), 512, 44100),
    }


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AUDIOPURE_REFERENCE")
    if not ref:
        raise SystemExit("usage: make_golden_psy.py /path/to/AudioPure  (or set AUDIOPURE_REFERENCE)")
    wb = load_reference(ref)
    orig_stft = torch.stft
    torch.stft = lambda *a, **k: torch.view_as_real(orig_stft(*a, return_complex=True, **k))
    out = {}
    for sr in (16000, 44100):
        m = wb.PsychoacousticMasker(sample_rate=sr)
        out[f"bark/{sr}"], out[f"ath/{sr}"] = m.bark, m.absolute_threshold_hearing
    out["window"] = ss.get_window("hann", 2048, fftbins=True)
    for name, (x, hop, sr) in clips().items():
        thr, pmax = wb.PsychoacousticMasker(hop_size=hop, sample_rate=sr).calculate_threshold_and_psd_maximum(x)
        assert thr.dtype == np.float32 and isinstance(pmax, np.float32), (thr.dtype, type(pmax))
        out[f"thr/{name}/x"], out[f"thr/{name}/db"], out[f"thr/{name}/psd_max"] = x, thr, pmax
        out[f"thr/{name}/hop"], out[f"thr/{name}/sr"] = np.int64(hop), np.int64(sr)

    # a real generate(): stage 1 (PGD) then stage 2 with the masker; every call of the hinge-loss hook is recorded
    B, L = 2, 6144
    r = np.random.default_rng(11)
    t = np.arange(L) / 16000.0
    x = np.stack([0.3 * np.sin(2 * np.pi * 523 * t) + 0.02 * r.standard_normal(L),
                  0.2 * r.standard_normal(L)])[:, None].astype(np.float32)
    y = np.array([3, 7])
    calls = []
    hook = wb.AudioAttack._loss_gradient_masking_threshold

    def record(self, perturbation, x_, thr_stab, pmax_stab):
        g, loss = hook(self, perturbation, x_, thr_stab, pmax_stab)
        calls.append((perturbation.detach().clone(), loss.clone(), g.clone(), thr_stab, pmax_stab))
        return g, loss

    wb.AudioAttack._loss_gradient_masking_threshold = record
    torch.manual_seed(0)
    attack = wb.AudioAttack(TinyNet().eval(), masker=wb.PsychoacousticMasker(), eps=0.002, learning_rate_1=0.0005,
                            max_iter_1=3, learning_rate_2=1.0, max_iter_2=4, eot_attack_size=1, eot_defense_size=1, verbose=0)
    attack.generate(torch.from_numpy(x), torch.from_numpy(y))
    assert len(calls) == 4, len(calls)
    out["traj/x"] = x
    out["traj/thr_stab"] = calls[0][3].numpy()
    out["traj/psd_max_stab"] = calls[0][4].numpy()
    out["traj/delta"] = np.stack([c[0].numpy() for c in calls])
    out["traj/loss"] = np.stack([c[1].numpy() for c in calls])
    out["traj/grad"] = np.stack([c[2].numpy() for c in calls])
    torch.stft = orig_stft
    path = os.path.join(HERE, "golden_psy_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", {k: (v.dtype.name, v.shape) for k, v in out.items() if k.startswith("traj")})


if __name__ == "__main__":
    main()
