#!/usr/bin/env python
"""Time the native optimizer step (audiopure_amd.optim on ap_optim.hip) on the five full-size parameter sets of the path -- the
DiffWave eps-network, M5, a 2-D ConvNet classifier, the Improved-Diffusion UNet, the KWS classifier -- each with the optimizer its
reference trainer uses, against torch.optim on its default path and with fused=True where this build offers it; for the UNet also
the three walks of train_util.py:247-258 (_log_grad_norm + AdamW.step + one update_ema) against their native equivalent (grad_norm()
+ a step with one tracked EMA rate).  Only the optimizer is timed: the gradients are seeded tensors of the parameters' shapes, set
once.  A window is --inner steps between device events and ends in a synchronise; the host clock around the same window is recorded
too (an optimizer step over hundreds of small tensors is host-bound on every path).  Median of --repeats windows after --warmup.
The achieved bytes per second of the native step are its 28 bytes per parameter for Adam and AdamW (16 for SGD with momentum), + 8
per EMA copy, over the event time.  Writes profiles/optim_bench.json (or --out).

    python tools/bench_optim.py [--out FILE] [--repeats 7] [--inner 10] [--sets wavenet m5 convnet unet kws]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from audiopure_amd import optim, synth  # noqa: E402


def build(name):
    """-> (module with full-size parameters on the CPU, optimizer class name, its arguments as the reference trainer gives them)"""
    if name == "wavenet":
        from audiopure_amd.diffusion_models.DiffWave_Unconditional.WaveNet import WaveNet_Speech_Commands
        return WaveNet_Speech_Commands(**dict(synth.FULL_WAVENET_CONFIG)), "Adam", dict(lr=2e-4)
    if name == "m5":
        from audiopure_amd.audio_models.M5.M5Net import M5
        return M5(n_input=1, n_output=35), "Adam", dict(lr=0.01, weight_decay=1e-4)
    if name == "convnet":
        import synth_convnets as S
        return S.FAMILIES["resnext29_8_64"](), "SGD", dict(lr=0.01, momentum=0.9, weight_decay=1e-2)
    if name == "unet":
        from audiopure_amd.diffusion_models.improved_diffusion_unet import create_model, model_and_diffusion_defaults
        return create_model(**model_and_diffusion_defaults()), "AdamW", dict(lr=1e-4, weight_decay=0.0)
    if name == "kws":
        from audiopure_amd.audio_models.RCNN_KWS import KWSModel
        return KWSModel(in_size=32), "Adam", dict(lr=1e-3, weight_decay=1e-5)
    raise KeyError(name)


def fresh_params(module, dev):
    """seeded parameters and gradients of the module's shapes, as leaves on the device (no module, no image to refresh)"""
    g = torch.Generator().manual_seed(0)
    params = []
    for p in module.parameters():
        q = torch.nn.Parameter((torch.rand(p.shape, generator=g) - 0.5).to(dev))
        q.grad = (torch.randn(p.shape, generator=g) * 1e-2).to(dev)
        params.append(q)
    return params


def timed(fn, warmup, repeats, inner):
    """per-step median and spread (ms): device events around `inner` calls, and the host clock around the same synchronised window"""
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


def reference_update_ema(target_params, source_params, rate=0.99):
    """improved_diffusion/nn.py:55-65"""
    for targ, src in zip(target_params, source_params):
        targ.detach().mul_(rate).add_(src, alpha=1 - rate)


def reference_log_grad_norm(params):
    """train_util.py:254-258: one host read per parameter"""
    sqsum = 0.0
    for p in params:
        sqsum += (p.grad ** 2).sum().item()
    return sqsum ** 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sets", nargs="+", default=["wavenet", "m5", "convnet", "unet", "kws"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_optim needs a GPU"
    dev = torch.device("cuda:0")
    result = {"config": {"timed": "optimizer.step() only, gradients set once", "inner_steps_per_window": args.inner,
                         "repeats": args.repeats, "warmup": args.warmup}, "by_set": {}}
    for name in args.sets:
        module, cls, kw = build(name)
        n_tensors = sum(1 for _ in module.parameters())
        n_params = sum(p.numel() for p in module.parameters())
        per_param = 16 if cls == "SGD" else 28
        row = {"optimizer": cls, "arguments": kw, "tensors": n_tensors, "parameters": n_params, "bytes_per_parameter": per_param}
        variants = [("native", optim, {}), ("torch_default", torch.optim, {}), ("torch_fused", torch.optim, {"fused": True})]
        finals = {}
        for label, mod, extra in variants:
            params = fresh_params(module, dev)
            try:
                opt = getattr(mod, cls)(params, **kw, **extra)
                row[label] = timed(opt.step, args.warmup, args.repeats, args.inner)
            except (RuntimeError, ValueError, TypeError) as e:      # fused=True is not offered for every optimizer / build
                row[label] = {"unavailable": f"{type(e).__name__}: {e}"}
                continue
            finals[label] = [p.detach() for p in params]
        # the variants took the same number of steps on the same seeded gradients: how far apart they ended, in lr
        steps = args.warmup + args.repeats * args.inner
        row["steps_taken"] = steps
        row["max_abs_native_vs_torch_default_over_lr"] = max(
            float((a - b).abs().max()) for a, b in zip(finals["native"], finals["torch_default"])) / kw["lr"]
        ms = row["native"]["median_ms"]
        row["native_bytes_per_second"] = n_params * per_param / (ms * 1e-3)
        row["native_over_torch_default"] = ms / row["torch_default"]["median_ms"]
        if "median_ms" in row["torch_fused"]:
            row["native_over_torch_fused"] = ms / row["torch_fused"]["median_ms"]
        if name == "unet":
            rate = 0.9999
            params = fresh_params(module, dev)
            opt = torch.optim.AdamW(params, **kw)
            ema = [p.detach().clone() for p in params]

            def reference_walks():
                reference_log_grad_norm(params)
                opt.step()
                reference_update_ema(ema, params, rate=rate)

            row["reference_three_walks"] = timed(reference_walks, args.warmup, args.repeats, args.inner)
            nparams = fresh_params(module, dev)
            nopt = optim.AdamW(nparams, **kw)
            nopt.track_ema(rate)

            def native_walks():
                nopt.grad_norm()
                nopt.step()

            row["native_three_walks"] = timed(native_walks, args.warmup, args.repeats, args.inner)
            row["native_three_walks_bytes_per_second"] = n_params * (per_param + 8 + 4) / (row["native_three_walks"]["median_ms"] * 1e-3)
            row["native_over_reference_three_walks"] = row["native_three_walks"]["median_ms"] / row["reference_three_walks"]["median_ms"]
        result["by_set"][name] = row
        print(json.dumps({name: row}))
        del module
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
