"""Golden vectors of the baseline defenses from the REFERENCE's own functions (transforms/time_defense.py and
transforms/frequency_defense.py, loaded by file path so transforms/__init__ and its librosa import are skipped).

* time_defense.py runs as written; AT's ``torch.randn`` is patched to return a recorded z.
* frequency_defense.py runs with two stand-ins for packages absent from the images: ``torch_lfilter.lfilter`` -> an fp64
  ``scipy.signal.lfilter`` autograd function whose adjoint is the reversed-time filter, and
  ``torchaudio.transforms.Resample`` -> torchaudio 0.11's sinc_interpolation kernel restated in numpy
  (``defense_design.resample_kernel``).  The reference's design calls, fp32 coefficient cast, batch-global clamp rule and
  ``same_size`` slicing run as written.

Forwards and input gradients (for a fixed cotangent) are recorded on small clips, with buttord / butter outputs for the
defaults and non-default parameter sets.  Needs scipy and the reference checkout (path as the first argument);
commits tests/golden/golden_defense_v1.npz."""
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from audiopure_amd.transforms import defense_design as D  # noqa: E402

REF = None                                  # the reference checkout: argv[1] or $AUDIOPURE_REFERENCE


class _LFilter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, b, a, x):                      # x [T, 1] as frequency_defense.py:94 passes it
        ctx.ba = (b.double().numpy(), a.double().numpy())
        y = signal.lfilter(ctx.ba[0], ctx.ba[1], x.detach().double().numpy(), axis=0)
        return torch.from_numpy(y).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        b, a = ctx.ba
        gr = g.detach().double().numpy()[::-1]
        dx = signal.lfilter(b, a, gr, axis=0)[::-1].copy()
        return None, None, torch.from_numpy(dx).to(g.dtype)


class _Resample(torch.nn.Module):
    """torchaudio 0.11 Resample(orig, new, resampling_method='sinc_interpolation') with its default width / rolloff."""

    def __init__(self, orig_freq, new_freq, resampling_method="sinc_interpolation"):
        super().__init__()
        assert resampling_method == "sinc_interpolation"
        g = math.gcd(int(orig_freq), int(new_freq))
        self.orig, self.new = int(orig_freq) // g, int(new_freq) // g
        k, self.width = D.resample_kernel(orig_freq, new_freq)
        self.kernel = torch.from_numpy(k.astype(np.float32)).view(self.new, 1, -1)

    def forward(self, w):
        shape = w.size()
        w = w.reshape(-1, shape[-1])
        n, L = w.shape
        w = F.pad(w, (self.width, self.width + self.orig))
        r = F.conv1d(w[:, None], self.kernel, stride=self.orig).transpose(1, 2).reshape(n, -1)
        r = r[..., :int(math.ceil(self.new * L / self.orig))]
        return r.view(shape[:-1] + r.shape[-1:])


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    global REF
    REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AUDIOPURE_REFERENCE")
    if not REF:
        raise SystemExit("usage: make_golden_defense.py /path/to/AudioPure  (or set AUDIOPURE_REFERENCE)")
    ta = types.ModuleType("torchaudio")
    ta.transforms = types.SimpleNamespace(Resample=_Resample)
    tl = types.ModuleType("torch_lfilter")
    tl.lfilter = lambda b, a, x: _LFilter.apply(b, a, x)
    sys.modules["torchaudio"], sys.modules["torch_lfilter"] = ta, tl
    td = _load("ref_time_defense", os.path.join(REF, "transforms", "time_defense.py"))
    fd = _load("ref_frequency_defense", os.path.join(REF, "transforms", "frequency_defense.py"))

    rng = np.random.default_rng(2026)
    B, L = 3, 2048
    x = np.clip(rng.normal(0, 0.3, (B, L)), -0.99, 0.99).astype(np.float32)     # tie-free, |x| <= 1
    xq = (np.round(rng.normal(0, 0.002, (B, L)) * 32768) / 32768).astype(np.float32)   # int16-quantised, ties everywhere
    x16 = np.round(x * 32767).astype(np.float32)                                # int16 scale: the +-32767 clamp branch
    xmix = x.copy()
    xmix[1] *= 4.0                                                              # one clip forces the wide branch for all
    xodd = np.clip(rng.normal(0, 0.3, (1, L + 1)), -0.99, 0.99).astype(np.float32)
    g = rng.normal(0, 1, (B, L)).astype(np.float32)
    godd = rng.normal(0, 1, (1, L + 1)).astype(np.float32)
    z = rng.normal(0, 1, (B, L)).astype(np.float32)
    out = dict(x=x, xq=xq, x16=x16, xmix=xmix, xodd=xodd, g=g, godd=godd, z=z)

    def run(name, fn, xin, gin):
        t = torch.from_numpy(xin).clone().requires_grad_(True)
        y = fn(t)
        (y * torch.from_numpy(gin[:, :y.shape[-1]])).sum().backward()
        out[name + "/y"] = y.detach().numpy().astype(np.float32)
        out[name + "/dx"] = t.grad.numpy().astype(np.float32)

    run("AS", td.AS, x, g)
    run("MS", td.MS, x, g)
    out["MSq/y"] = td.MS(torch.from_numpy(xq)).numpy()
    real_randn = torch.randn
    torch.randn = lambda *a, **k: torch.from_numpy(z).clone()
    try:
        run("AT", td.AT, x, g)
    finally:
        torch.randn = real_randn
    run("DS", fd.DS, x, g)
    run("DSodd", lambda t: fd.DS(t, 0.5, 16000, False), xodd, np.pad(godd, ((0, 0), (0, 1))))
    for kind, fn in (("LPF", fd.LPF), ("BPF", fd.BPF)):
        run(kind, fn, x, g)
        run(kind + "16", fn, x16, g)
        run(kind + "mix", fn, xmix, g)
    run("LPFodd", fd.LPF, xodd, godd)

    designs = {"lpf_default": ((0.5,), (1.0,), "low"), "lpf_a": ((5 / 8000,), (2000 / 8000,), "low"),
               "lpf_b": ((0.25,), (0.5,), "low"), "bpf_default": ((300 / 8000, 0.5), (50 / 8000, 1.0), "bandpass"),
               "bpf_a": ((500 / 8000, 3000 / 8000), (100 / 8000, 6000 / 8000), "bandpass")}
    for name, (wp, ws, bt) in designs.items():
        wp, ws = (np.array(v) if len(v) > 1 else v[0] for v in (wp, ws))
        N, Wn = signal.buttord(wp, ws, 3, 40, analog=False, fs=None)
        b, a = signal.butter(N, Wn, btype=bt, analog=False, output="ba")
        out[f"design/{name}/wp"], out[f"design/{name}/ws"] = np.atleast_1d(wp), np.atleast_1d(ws)
        out[f"design/{name}/N"], out[f"design/{name}/Wn"] = np.array(N), np.atleast_1d(Wn)
        out[f"design/{name}/b"], out[f"design/{name}/a"] = b, a
    path = os.path.join(ROOT, "tests", "golden", "golden_defense_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
