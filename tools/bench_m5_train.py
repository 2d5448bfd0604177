#!/usr/bin/env python
"""Time one native train-mode step of M5 (``model.train(); F.nll_loss(model(x), y).backward()``: ap_m5_train_fwd + ap_m5_train_bwd,
ap_m5_train.hip) at L = 16 000, B = 10 and B = 256, and where it goes per kernel.  The yardstick is the same step through torch-ROCm's
own operators on the same card in the same process: a plain ``torch.nn`` restatement of M5 built here.  Device events around
synchronised windows, median of 5 after 2 warm-ups (as tools/bench_train_step.py); the per-kernel split is one profiled step
(torch.profiler device activity).  Writes profiles/m5_train_bench.json (or --out).

    python tools/bench_m5_train.py [--out FILE] [--repeats 5] [--batches 10 256]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from audiopure_amd import synth  # noqa: E402
from audiopure_amd.audio_models.M5.M5Net import M5  # noqa: E402
from bench_train_step import timed  # noqa: E402


class TorchM5(nn.Module):
    """M5 through torch's operators: conv -> BatchNorm1d -> ReLU -> MaxPool1d(4), four times; mean over time; linear; log_softmax"""

    def __init__(self, n_output=10, n_channel=32, first_kernel_size=80, stride=16):
        super().__init__()
        chans = [(1, n_channel, first_kernel_size, stride), (n_channel, n_channel, 3, 1), (n_channel, 2 * n_channel, 3, 1),
                 (2 * n_channel, 2 * n_channel, 3, 1)]
        for i, (ci, co, k, s) in enumerate(chans, start=1):
            setattr(self, f"conv{i}", nn.Conv1d(ci, co, k, stride=s))
            setattr(self, f"bn{i}", nn.BatchNorm1d(co))
        self.fc1 = nn.Linear(2 * n_channel, n_output)

    def forward(self, x):
        for i in (1, 2, 3, 4):
            x = F.max_pool1d(F.relu(getattr(self, f"bn{i}")(getattr(self, f"conv{i}")(x))), 4)
        return F.log_softmax(self.fc1(x.mean(dim=-1)), dim=1)


def per_kernel(step):
    """device time of one step by kernel name (microseconds, launches), largest first"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    rows = []
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", None)
        if t is None:
            t = getattr(e, "cuda_time_total", 0.0)
        if str(getattr(e, "device_type", "")).endswith("CUDA") and t > 0:
            rows.append({"kernel": e.key[:96], "launches": int(e.count), "total_us": float(t)})
    return sorted(rows, key=lambda r: -r["total_us"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "m5_train_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[10, 256])
    ap.add_argument("--length", type=int, default=16000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_m5_train needs a GPU"
    dev = torch.device("cuda:0")
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.m5_state_dict(10).items()}
    native, ref = M5(n_input=1, n_output=10), TorchM5(10)
    native.load_state_dict(sd)
    ref.load_state_dict(sd)
    native, ref = native.to(dev).train(), ref.to(dev).train()
    result = {"config": {"L": args.length, "n_channel": 32, "n_output": 10, "step": "zero_grad + nll_loss(model(x), y).backward()"},
              "by_batch": {}}
    for B in args.batches:
        x = torch.from_numpy(synth.waveforms(B, args.length, seed=7)).to(dev)
        y = (torch.arange(B) % 10).to(dev)

        def step_of(model):
            def step():
                model.zero_grad(set_to_none=True)
                F.nll_loss(model(x), y).backward()
            return step

        row = {"native_step": timed(step_of(native), args.warmup, args.repeats),
               "torch_operator_step": timed(step_of(ref), args.warmup, args.repeats)}
        with torch.no_grad():
            row["native_forward_no_grad"] = timed(lambda: native(x), args.warmup, args.repeats)
            row["torch_operator_forward_no_grad"] = timed(lambda: ref(x), args.warmup, args.repeats)
        row["native_over_torch"] = row["native_step"]["median_ms"] / row["torch_operator_step"]["median_ms"]
        try:
            row["native_per_kernel"] = per_kernel(step_of(native))
            row["torch_operator_per_kernel"] = per_kernel(step_of(ref))[:12]
        except Exception as e:                                     # the timing above stands without the split
            row["per_kernel_error"] = f"{type(e).__name__}: {e}"
        result["by_batch"][str(B)] = row
        print(json.dumps({"B": B, **{k: v for k, v in row.items() if not k.endswith("per_kernel")}}))
        for r in row.get("native_per_kernel", []):
            print(f"    {r['total_us']:9.1f} us  x{r['launches']:<3d} {r['kernel']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
