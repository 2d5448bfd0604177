#!/usr/bin/env python
"""Time the device-side speech-commands train pipeline (audiopure_amd.transforms.SpeechCommandsAugment on ap_augment.hip): ms per
batch at B = 96 and 128 one-second clips, with seeded draws (about half the clips mix noise, half of all lanes run the vocoder) and
in the worst case, where every transform is applied to every clip and every clip mixes a background clip (2 B lanes, 2 B vocoders).
For comparison the same pipeline in float32 torch operators on the device (gathers for np.interp, torch.stft, a loop over the
vocoder's steps on [lanes, 1025] tensors, a matmul with the filterbank); the reference's own route is numpy + librosa per sample in
DataLoader workers, and librosa is not installed, so that route is not timed.  Timed per batch: the forward with the draws already
made (table upload, background gather and four launches; device events around --inner forwards, and the host clock around the same
synchronised window), and separately draw_augment on the host.  Median of --repeats windows after --warmup.  Also printed: the largest
|dB| between the two routes' outputs (the same draws), a check that they compute the same thing.  Sets no threshold.
Writes profiles/augment_bench.json (or --out).

    python tools/bench_augment.py [--out FILE] [--repeats 7] [--inner 5] [--batches 96 128]
"""
import argparse
import json
import math
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiopure_amd import synth  # noqa: E402
from audiopure_amd.transforms.augment import HOP, N_FFT, SpeechCommandsAugment, draw_augment  # noqa: E402

L, N_BG = 16000, 60             # one-second clips; the dataset's background table is about a minute per file, 6 files


class AlwaysApply:
    """an rng whose random() is 0.0 -- every transform applied, every clip mixes noise -- with a seeded Random's other draws"""

    def __init__(self, seed):
        self.r = random.Random(seed)

    def random(self):
        return 0.0

    def uniform(self, a, b):
        return self.r.uniform(a, b)

    def randint(self, a, b):
        return self.r.randint(a, b)

    def choice(self, seq):
        return self.r.choice(seq)


def mel_filterbank(n_mels, dev):
    """librosa.filters.mel(sr=16000, n_fft=2048, n_mels) as float32 [n_mels, 1025]"""
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    hz_to_mel = lambda f: min_log_mel + math.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp
    m = torch.linspace(hz_to_mel(0.0), hz_to_mel(8000.0), n_mels + 2, dtype=torch.float64)
    pts = torch.where(m >= min_log_mel, min_log_hz * torch.exp(logstep * (m - min_log_mel)), f_sp * m)
    freqs = torch.linspace(0, 8000.0, N_FFT // 2 + 1, dtype=torch.float64)
    lo, mid, hi = pts[:-2], pts[1:-1], pts[2:]
    up, down = (freqs[None] - lo[:, None]) / (mid - lo)[:, None], (hi[:, None] - freqs[None]) / (hi - mid)[:, None]
    return (torch.clamp(torch.minimum(up, down), min=0.0) * (2.0 / (hi - lo))[:, None]).float().to(dev)


def torch_pipeline(x, bg, d, fb, dev):
    """the pipeline on float32 torch operators: x [B, L] and bg [n_bg, L] on the device, d the draws -> [B, n_mels, 32]"""
    B, nl, F = d.n, d.lanes, 1 + L // HOP
    lanes = torch.cat([x, bg.index_select(0, torch.from_numpy(d.source[B:]).to(dev))]) if nl > B else x
    amp = torch.from_numpy(d.amp).to(dev)[:, None]
    fac, n_interp = torch.from_numpy(d.speed_fac).to(dev)[:, None], torch.from_numpy(d.n_interp).to(dev)[:, None]
    j = torch.arange(L, device=dev)[None]
    pos = j.double() * fac
    i = pos.floor().long()
    i0 = i.clamp(max=L - 2)
    a, b = lanes.gather(1, i0), lanes.gather(1, i0 + 1)
    v = torch.where(i >= L - 1, lanes[:, -1:], (b - a) * (pos - i0).float() + a)
    wave = amp * torch.where(j < n_interp, v, torch.zeros_like(v))
    D = torch.stft(wave, N_FFT, HOP, window=torch.hann_window(N_FFT, device=dev), center=True, pad_mode="constant", return_complex=True)
    Dp = torch.nn.functional.pad(D, (0, 2))                                             # [nl, 1025, F + 2]
    rate = torch.from_numpy(d.rate).to(dev)
    applied = torch.from_numpy(d.stretch_applied).to(dev)
    T = torch.from_numpy(d.n_out).to(dev)
    n_steps = int(d.n_out.max())
    k = torch.arange(N_FFT // 2 + 1, device=dev)
    phi = ((k % 4).float() * (math.pi / 2))[None]
    two_pi = 2 * math.pi
    acc = torch.angle(Dp[:, :, 0])
    cols = []
    for t in range(n_steps):
        s = t * rate
        i = s.floor().long().clamp(max=F)
        alpha = (s - i).float()[:, None]
        idx = i[:, None, None].expand(-1, Dp.shape[1], 1)
        c0, c1 = Dp.gather(2, idx)[..., 0], Dp.gather(2, idx + 1)[..., 0]
        cols.append(torch.polar((1 - alpha) * c0.abs() + alpha * c1.abs(), acc))
        dp = torch.angle(c1) - torch.angle(c0) - phi
        dp = dp - two_pi * torch.round(dp / two_pi)
        acc = acc + (phi + dp)
        acc = acc - two_pi * torch.round(acc / two_pi)
    S = torch.stack(cols, dim=2)
    if n_steps < F + 2:
        S = torch.nn.functional.pad(S, (0, F + 2 - n_steps))
    Dw = torch.nn.functional.pad(Dp, (0, S.shape[2] - Dp.shape[2]))
    S = torch.where(applied[:, None, None], S, Dw)
    c = torch.arange(F, device=dev)[None]
    src = c + torch.from_numpy(d.shift).to(dev)[:, None]
    ok = (src >= 0) & (src < T[:, None]) & (c < T[:, None])
    out = S.gather(2, src.clamp(0, S.shape[2] - 1)[:, None, :].expand(-1, S.shape[1], -1)) * ok[:, None, :]
    clip = out[:B]
    nlane = torch.from_numpy(d.noise_lane).to(dev).long()
    p = torch.from_numpy(d.p.astype(np.float32)).to(dev)[:, None, None]
    mixed = torch.where((nlane >= 0)[:, None, None], clip * (1 - p) + out[nlane.clamp(min=0)] * p, clip)
    db = 10.0 * torch.log10(torch.clamp(fb @ (mixed.real ** 2 + mixed.imag ** 2), min=1e-10))
    return torch.clamp(db - db.amax(dim=(1, 2), keepdim=True), min=-80.0)


def timed(fn, warmup, repeats, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / inner)
        ev.append(a.elapsed_time(b) / inner)
    return {"median_ms": statistics.median(ev), "min_ms": min(ev), "max_ms": max(ev), "host_median_ms": statistics.median(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[96, 128])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_augment needs a GPU"
    dev = torch.device("cuda:0")
    bg_host = synth.noise(0, N_BG, L, seed=2)[:, 0].copy()
    module = SpeechCommandsAugment(bg_host, n_mels=32).to(dev)
    fb = mel_filterbank(32, dev)
    result = {"config": {"clip_samples": L, "background_clips": N_BG, "n_mels": 32, "timed": "forward with the draws made; draw_augment apart",
                         "inner_per_window": args.inner, "repeats": args.repeats, "warmup": args.warmup}, "by_batch": {}}
    for B in args.batches:
        x = torch.from_numpy(synth.waveforms(B, L, seed=3)[:, 0].copy()).to(dev)
        lengths = [L] * B
        row = {}
        for case, rng in (("seeded_draws", random.Random(B)), ("every_transform_and_noise", AlwaysApply(B))):
            d = draw_augment(rng, B, N_BG, lengths)
            t0 = time.perf_counter()
            for _ in range(20):
                draw_augment(rng, B, N_BG, lengths)
            draw_ms = (time.perf_counter() - t0) * 1e3 / 20
            native = timed(lambda: module(x, lengths, draws=d), args.warmup, args.repeats, args.inner)
            ops = timed(lambda: torch_pipeline(x, module.bg_samples, d, fb, dev), args.warmup, args.repeats, args.inner)
            diff = float((module(x, lengths, draws=d) - torch_pipeline(x, module.bg_samples, d, fb, dev)).abs().max())
            row[case] = {"lanes": d.lanes, "vocoder_lanes": int(d.stretch_applied.sum()), "noise_mixes": int(d.noise_applied.sum()),
                         "native": native, "torch_operators": ops, "native_over_torch_operators": native["median_ms"] / ops["median_ms"],
                         "host_draw_augment_ms": draw_ms, "max_abs_db_between_routes": diff}
        result["by_batch"][str(B)] = row
        print(json.dumps({B: row}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
