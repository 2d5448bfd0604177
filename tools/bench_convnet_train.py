#!/usr/bin/env python
"""Time one native train-mode step of the 2-D ConvNet classifiers (``zero_grad; CrossEntropyLoss(model(x), y).backward()`` through
``NativeConvNet`` in ``train()`` mode: ap_conv2d_fwd, ap_bn2d_train_fwd / _bwd, ap_conv2d_wgrad, ap_conv2d_pack / _pack_bwd and the
element-wise primitives) on ``resnext29_8_64`` and ``wideresnet28_10`` at 1 x 32 x 32, B = 96 (train_speech_commands.py's default)
and B = 10, and where it goes per kernel.  The yardstick is the same step through torch-ROCm's own operators on the SAME module in the
same process -- what train() mode did before the native step existed, outside AUDIOPURE_STRICT.  Device events around synchronised
windows, median of 5 after 2 warm-ups (as tools/bench_train_step.py); the per-kernel split is one profiled step (torch.profiler device
activity).  ap_conv2d_wgrad's share of the fp32 MFMA peak is its algorithmic flops (2 Cout (Cin/g) k k B OH OW per conv step) over its
kernel time over 157.3 TFLOP/s.  The two families with live dropout, ``vgg19_bn`` and ``wideresnet28_10D``, run under
``set_dropout("philox")`` against the torch-operator step of the same module (torch's own dropout).  ``--loss-head`` adds the loss
head alone on [B, 10] scores: ``losses.cross_entropy(..., return_stats=True)`` + backward (loss, seed, pred, correct: three launches)
against ``F.cross_entropy`` + backward + ``max(1)`` + ``eq().sum()``.  Writes profiles/convnet_train_bench.json (or --out); the rows of
models that are not run stay as the file has them.

    python tools/bench_convnet_train.py [--out FILE] [--repeats 5] [--batches 96 10] [--models resnext29_8_64 wideresnet28_10] [--loss-head]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from audiopure_amd import losses, synth  # noqa: E402
from audiopure_amd.convnet import NativeConvNet  # noqa: E402
from bench_m5_train import per_kernel  # noqa: E402
from bench_train_step import timed  # noqa: E402
import synth_convnets as S  # noqa: E402

F32_MFMA_PEAK = 157.3e12                                          # FLOP/s, v_mfma_f32_32x32x2_f32 on every CU at the spec clock
CHW = (1, 32, 32)
MODELS = dict(S.FAMILIES, wideresnet28_10D=lambda: S.WideResNet28_10(10, 1, drop_rate=0.3))       # models/__init__.py:31
LIVE_DROPOUT = ("vgg19_bn", "wideresnet28_10D")


def loss_head_row(B, dev, warmup, repeats, K=10):
    """loss + seed of backward + pred + correct on [B, K] scores: the native head against torch's operators"""
    z = torch.from_numpy(synth.uniform("bench/loss", (B, K), 5, -4.0, 4.0)).to(dev).requires_grad_(True)
    y = (torch.arange(B) % K).to(dev)

    def native():
        z.grad = None
        loss, pred, correct = losses.cross_entropy(z, y, return_stats=True)
        loss.backward()

    def operators():
        z.grad = None
        loss = F.cross_entropy(z, y)
        loss.backward()
        pred = z.data.max(1, keepdim=True)[1]
        pred.eq(y.view_as(pred)).sum()

    row = {"native": timed(native, warmup, repeats), "torch_operators": timed(operators, warmup, repeats), "classes": K}
    row["native_over_torch"] = row["native"]["median_ms"] / row["torch_operators"]["median_ms"]
    row["native_per_kernel"], row["torch_operator_per_kernel"] = per_kernel(native)[:8], per_kernel(operators)[:12]
    return row


def wgrad_flops(plan, B):
    """algorithmic flops of every conv step's weight gradient: 2 x rows x columns x contraction"""
    total = 0
    for s in plan.steps:
        if s.kind == "conv":
            Cout, Cg, kh, kw = s.p["wshape"]
            total += 2 * Cout * Cg * kh * kw * B * s.out.H * s.out.W
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convnet_train_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[96, 10])
    ap.add_argument("--models", nargs="*", default=["resnext29_8_64", "wideresnet28_10"])
    ap.add_argument("--loss-head", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_convnet_train needs a GPU"
    dev = torch.device("cuda:0")
    result = {"config": {"input": list(CHW), "step": "zero_grad + cross_entropy(model(x), y).backward()",
                         "f32_mfma_peak_flops": F32_MFMA_PEAK}, "by_model": {}}
    if os.path.exists(args.out):                                   # rows of models that are not run now stay
        with open(args.out) as f:
            result["by_model"] = json.load(f).get("by_model", {})
    for name in args.models:
        module = synth.synth_init(MODELS[name](), 0).to(dev).train()
        net = NativeConvNet(module, CHW).train()
        if name in LIVE_DROPOUT:
            net.set_dropout("philox")                              # (the yardstick step draws torch's own masks)
        result["by_model"][name] = {}
        for B in args.batches:
            x = torch.from_numpy(synth.uniform("bench/cnt", (B,) + CHW, 5, -2.0, 2.0)).to(dev)
            y = (torch.arange(B) % 10).to(dev)

            def step_of(model):
                def step():
                    module.zero_grad(set_to_none=True)
                    F.cross_entropy(model(x), y).backward()
                return step

            row = {"native_step": timed(step_of(net), args.warmup, args.repeats),
                   "torch_operator_step": timed(step_of(module), args.warmup, args.repeats)}
            assert type(net(x).grad_fn).__name__ == "_ConvNetTrainFnBackward"     # the native route was what was timed
            row["native_over_torch"] = row["native_step"]["median_ms"] / row["torch_operator_step"]["median_ms"]
            flops = wgrad_flops(net._train_plan, B)
            row["wgrad_algorithmic_flops"] = flops
            rows = per_kernel(step_of(net))                        # (a profiler failure fails the benchmark: the split is part of the result)
            row["native_per_kernel"] = rows[:16]
            wg_us = sum(r["total_us"] for r in rows if "conv2d_wgrad_kernel" in r["kernel"])
            assert wg_us > 0, "no conv2d_wgrad_kernel launch in the profiled step"
            row["wgrad_kernel_ms"] = wg_us / 1e3
            row["wgrad_fraction_of_f32_mfma_peak"] = flops / (wg_us * 1e-6) / F32_MFMA_PEAK
            row["torch_operator_per_kernel"] = per_kernel(step_of(module))[:12]
            result["by_model"][name][str(B)] = row
            print(json.dumps({"model": name, "B": B, **{k: v for k, v in row.items() if not k.endswith("per_kernel")}}))
            for r in row.get("native_per_kernel", []):
                print(f"    {r['total_us']:9.1f} us  x{r['launches']:<4d} {r['kernel']}")
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:                         # after every row: a later row's failure loses nothing
                json.dump(result, f, indent=1)
    if args.loss_head:
        result["loss_head"] = {}
        for B in args.batches:
            result["loss_head"][str(B)] = row = loss_head_row(B, dev, args.warmup, args.repeats)
            print(json.dumps({"loss_head": B, **{k: v for k, v in row.items() if not k.endswith("per_kernel")}}))
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
