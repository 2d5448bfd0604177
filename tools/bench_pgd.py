#!/usr/bin/env python
"""Time one ``pgd`` call of the two adversarial-training scripts at their own shapes -- RCNN_KWS/train.py: B = 128, n_mels 32, T = 161
frames (L = 32000), n = 10; adv_train_speech_commands.py: ``resnext29_8_64`` in ``train()``, the 48 adversarial clips of a batch of 96,
L = 16000, n = 10 -- in three legs, alternated in one process:

    (a) script     the scripts' way of running the loop (``script_pgd`` below: per-sample host reads and all; the KWS case with the
                   KWS script's never-cleared gradient) over the native modules with the parameters requiring gradients: what
                   ran before ``audiopure_amd.attacks`` existed, the yardstick
    (b) frozen     the same loop with the parameters frozen: (a) - (b) is what the discarded parameter gradients cost
    (c) native     ``audiopure_amd.attacks.pgd``: (b) - (c) is the loop glue (host reads, small operators, the final gather)

A call is timed by the host clock between two device synchronises; median, min and max over --repeats after --warmup.  Then one
profiled call of (a) and of (c) gives device time per kernel, the name of every kernel (c) launched, and whether a weight-gradient
or bias-gradient kernel (``wgrad`` / ``rowsum`` in its name) is among them.  Writes
profiles/pgd_bench.json (or --out).

    python tools/bench_pgd.py [--out FILE] [--repeats 5] [--warmup 2] [--legs kws convnet]
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
from audiopure_amd import attacks, losses, synth  # noqa: E402
from audiopure_amd.audio_models.RCNN_KWS import KWSModel  # noqa: E402
from audiopure_amd.convnet import NativeConvNet  # noqa: E402
from audiopure_amd.transforms.melspec import MelSpecDB, MelSpecDBHTK  # noqa: E402
from bench_m5_train import per_kernel  # noqa: E402
import synth_convnets as S  # noqa: E402


def script_pgd(model, transform, x, y, criterion, eps=0.002, alpha=0.0004, n=10, zero_grad=True):
    """The scripts' way of running the loop, written for this bench (adv_train_speech_commands.py:139-183; with zero_grad=False
    RCNN_KWS/train.py:84-121, which never clears the perturbation's gradient, so its steps follow the running sum).  Kept, because
    they are what the loop costs: a range check that reads the host, B blocking host reads per iteration (one per sample, a compare
    whose truth value Python needs before it goes on), loss.backward() into the leaf and into every parameter's .grad, the update
    as separate torch operators, and B row slices joined at the end.  Simplified: the row argmax is taken once per iteration for
    the whole batch, not per sample -- so this leg is, if anything, cheaper than the scripts' own text."""
    B = x.shape[0]
    if not (bool(x.min() >= -1) and bool(x.max() <= 1)):
        raise AssertionError("x outside [-1, 1]")
    start = eps * (2 * torch.rand_like(x) - 1)
    delta = ((x + start).clamp(-1, 1) - x).requires_grad_(True)
    kept = {}
    for it in range(n + 1):
        x_pert = x + delta
        scores = model(transform(x_pert))
        wrong = scores.argmax(1) != y
        for j in range(B):
            if bool(wrong[j]):                                   # the blocking read
                kept[j] = x_pert[j]
        if it == n:
            break
        criterion(scores, y).backward()
        with torch.no_grad():
            moved = (delta + alpha * delta.grad.sign()).clamp(-eps, eps)
            delta.copy_((x + moved).clamp(-1, 1) - x)
            if zero_grad:
                delta.grad.zero_()
    return torch.cat([kept.get(j, x_pert[j]) for j in range(B)], dim=0).unsqueeze(1)


def timed_alternated(legs, warmup, repeats):
    """{name: fn} -> {name: median / min / max ms}: the legs take turns, so a drift of the machine falls on all of them alike"""
    ms = {k: [] for k in legs}
    for r in range(warmup + repeats):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}


def wave(B, L, dev):
    return torch.from_numpy(synth.uniform(f"pgdbench/{B}/{L}", (B, 1, L), 3, -0.5, 0.5)).to(dev)


def run(name, model, transform, x, y, n, args, accumulate):
    crit = losses.CrossEntropyLoss()
    params = list(model.parameters())

    def script():
        for p in params:
            p.requires_grad_(True)
        script_pgd(model, transform, x, y, crit, n=n, zero_grad=not accumulate)
        for p in params:                                         # the caller's optimizer.zero_grad()
            p.grad = None

    def frozen():
        with attacks._frozen(model):
            script_pgd(model, transform, x, y, crit, n=n, zero_grad=not accumulate)

    def native():
        attacks.pgd(model, x, y, n=n, transform=transform, criterion=crit, accumulate=accumulate)

    row = {"B": x.shape[0], "L": x.shape[2], "n": n, "model": name, "accumulate": accumulate}
    row.update(timed_alternated({"script": script, "frozen": frozen, "native": native}, args.warmup, args.repeats))
    a, b, c = (row[k]["median_ms"] for k in ("script", "frozen", "native"))
    row["parameter_gradients_ms"], row["loop_glue_ms"], row["native_over_script"] = a - b, b - c, c / a
    row["native_below_script_by_more_than_its_spread"] = row["native"]["max_ms"] < row["script"]["min_ms"]
    try:
        every = per_kernel(native)                               # every kernel of the call, not the largest alone
        row["native_per_kernel"] = every[:16]
        row["native_kernel_names"] = sorted({r["kernel"] for r in every})
        row["native_launches_wgrad_or_rowsum"] = any("wgrad" in r["kernel"] or "rowsum" in r["kernel"] for r in every)
        row["script_per_kernel"] = per_kernel(script)[:16]
        row["script_launches_wgrad_or_rowsum"] = any("wgrad" in r["kernel"] or "rowsum" in r["kernel"] for r in per_kernel(script))
    except Exception as e:                                       # the timing above stands without the split
        row["per_kernel_error"] = f"{type(e).__name__}: {e}"
    print(json.dumps({k: v for k, v in row.items() if not k.endswith("per_kernel") and k != "native_kernel_names"}))
    for r in row.get("native_per_kernel", [])[:8]:
        print(f"    {r['total_us']:9.1f} us  x{r['launches']:<4d} {r['kernel']}")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgd_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--legs", nargs="+", default=["kws", "convnet"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pgd needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    result = {"config": {"eps": 0.002, "alpha": 0.0004, "p": "linf", "timing": "host clock between device synchronises, legs alternated",
                         "legs": {"script": "the script's pgd over the native modules, parameters requiring gradients",
                                  "frozen": "the same, parameters frozen", "native": "audiopure_amd.attacks.pgd"}}, "by_case": {}}
    if "kws" in args.legs:
        m = KWSModel(in_size=32).to(dev).train()
        x = wave(128, 32000, dev)
        result["by_case"]["kws_128x161"] = run("KWSModel(32)", m, MelSpecDBHTK(32), x, (torch.arange(128) % 4).to(dev), args.n, args,
                                                accumulate=True)          # the KWS script's own loop
    if "convnet" in args.legs:
        module = synth.synth_init(S.FAMILIES["resnext29_8_64"](), 0).to(dev).train()
        net = NativeConvNet(module, (1, 32, 32)).train()
        x = wave(48, 16000, dev)
        result["by_case"]["resnext29_8_64_48"] = run("resnext29_8_64", net, MelSpecDB(32), x, (torch.arange(48) % 10).to(dev), args.n, args,
                                                      accumulate=False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
