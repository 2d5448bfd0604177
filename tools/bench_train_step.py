#!/usr/bin/env python
"""Time one native training step (``util.training_loss`` + ``.backward()``) of the shipped eps-network -- fp32, C = S = 256,
36 layers, L = 16 000, B = 2 and B = 8 -- and where it goes: the saving forward, the input-gradient sweep, the weight-gradient
launches, the weight-norm unfold, and the re-fold / re-pack after a parameter update.  The yardstick is ``EpsGrad.forward_save`` +
``EpsGrad.backward`` without parameter gradients on the same shapes in the same process.  Device events around synchronised
windows, medians over repeats after warm-up.  Writes profiles/train_step_bench.json (or --out).

    python tools/bench_train_step.py [--out FILE] [--repeats 5] [--batches 2 8]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiopure_amd import _native as N  # noqa: E402
from audiopure_amd import synth  # noqa: E402
from audiopure_amd.diffusion_models import _grad as G  # noqa: E402
from audiopure_amd.diffusion_models.DiffWave_Unconditional.WaveNet import WaveNet_Speech_Commands  # noqa: E402
from audiopure_amd.diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams, training_loss  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def timed(fn, warmup, repeats):
    """Median and spread (ms) of fn() between device events, each window ending in a synchronise."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--length", type=int, default=16000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_train_step needs a GPU"
    dev = torch.device("cuda:0")
    cfg = dict(synth.FULL_WAVENET_CONFIG)
    net = WaveNet_Speech_Commands(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.wavenet_state_dict(cfg, 0).items()})
    net = net.to(dev)
    dh = calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG)
    C_, S_, NL, L = cfg["res_channels"], cfg["skip_channels"], cfg["num_res_layers"], args.length
    loss_fn = torch.nn.MSELoss()
    eg = G._eps_grad_of(net)
    lib = N.lib()
    result = {"config": {"C": C_, "S": S_, "layers": NL, "L": L, "precision": "f32"}, "peak_f32_mfma_flops": PEAK_F32_MFMA, "by_batch": {}}
    for B in args.batches:
        x = torch.from_numpy(synth.waveforms(B, L, seed=7)).to(dev)
        z = torch.from_numpy(synth.noise(0, B, L, seed=7)).to(dev)
        v = torch.from_numpy(synth.noise(1, B, L, seed=7)).to(dev) / (B * L)
        steps = [50] * B                                             # one step group: the whole batch in one sweep
        src = (torch.tensor(steps), z)

        def step():
            net.zero_grad(set_to_none=True)
            training_loss(net, loss_fn, x, dh, noise_source=src).backward()

        row = {"training_loss_plus_backward": timed(step, args.warmup, args.repeats)}
        row["forward_save"] = timed(lambda: eg.forward_save(x, 50.0), args.warmup, args.repeats)
        _, saved = eg.forward_save(x, 50.0)
        row["input_gradient_sweep"] = timed(lambda: eg.backward(saved, v), args.warmup, args.repeats)
        pg = G.ParamGrads(net)
        row["sweep_with_weight_gradients"] = timed(lambda: eg.backward(saved, v, pg.at(x, 50.0)), args.warmup, args.repeats)
        row["unfold"] = timed(pg.finish, args.warmup, args.repeats)

        # the ap_wgrad_corr launches of one sweep alone, on the sweep's own operands' shapes
        dy, dhp, dsk = torch.randn(B, 2 * C_, L, device=dev), torch.randn(B, C_, L, device=dev), torch.randn(B, S_, L, device=dev)
        film = torch.randn(C_, device=dev)
        eng = eg._prepare()
        pg.at(x, 50.0).begin(eg, eng, B, L, dev)

        def dilated(n):
            pg.corr(dy, saved.hs[n], film, pg.w1[n], B, 2 * C_, C_, L, 3, 2 ** (n % cfg["dilation_cycle"]), 1, 1.0)

        def pointwise(n):
            if n + 1 < NL:
                pg.corr(dhp, saved.pre_gate[n], None, pg.res_w[n], B, C_, C_, L, 1, 1, 2, G._RS)
            pg.corr(dsk, saved.pre_gate[n], None, pg.skip_w[n], B, S_, C_, L, 1, 1, 2, 1.0)

        def all_corr():
            pg.corr(dsk, saved.skip, None, pg.f1_w, B, S_, S_, L, 1, 1, 0, 1.0)
            for n in range(NL):
                dilated(n)
                pointwise(n)

        row["wgrad_corr_launches"] = t_corr = timed(all_corr, args.warmup, args.repeats)
        row["wgrad_corr_dilated_per_layer"] = timed(lambda: [dilated(n) for n in range(NL)], args.warmup, args.repeats)
        row["wgrad_corr_res_skip_per_layer"] = timed(lambda: [pointwise(n) for n in range(NL)], args.warmup, args.repeats)
        for k in ("wgrad_corr_dilated_per_layer", "wgrad_corr_res_skip_per_layer"):
            row[k] = {kk: vv / NL for kk, vv in row[k].items()}
        flop = 2.0 * B * L * (NL * 2 * C_ * C_ * 3 + (NL - 1) * C_ * C_ + NL * S_ * C_ + S_ * S_)
        row["wgrad_corr_flop"] = flop
        row["wgrad_corr_fraction_of_fp32_mfma_peak"] = flop / (t_corr["median_ms"] * 1e-3) / PEAK_F32_MFMA

        # the forward block per layer (ap_resblock_fwd_save: the same flops as a layer's three contractions)
        hs, pre, part, skip = saved.hs, saved.pre_gate, saved.part, torch.empty_like(saved.skip)

        def blocks():
            for n in range(NL):
                N.check(lib.ap_resblock_fwd_save(eng.ctx, n, N.ptr(hs[n]), N.ptr(part[n * C_:(n + 1) * C_]), N.ptr(hs[n + 1]), N.ptr(skip),
                                                 N.ptr(pre[n]), 1 if n else 0, B, L, N.stream()), "ap_resblock_fwd_save")

        row["resblock_fwd_save_per_layer"] = {k: v_ / NL for k, v_ in timed(blocks, args.warmup, args.repeats).items()}

        # after optimizer.step(): the next call re-folds the weights (engine()) and re-packs the backward images (_prepare())
        def refold():
            with torch.no_grad():
                net.final_conv[2].conv.bias.add_(0.0)                # bumps a parameter's version, changes no value
            eg._prepare()

        row["refold_and_repack"] = timed(refold, 1, max(3, args.repeats // 2))
        base = row["forward_save"]["median_ms"] + row["input_gradient_sweep"]["median_ms"]
        row["yardstick_forward_save_plus_backward_ms"] = base
        row["weight_gradient_sweep_multiple_of_yardstick"] = (row["sweep_with_weight_gradients"]["median_ms"]
                                                              - row["input_gradient_sweep"]["median_ms"]) / base
        row["step_multiple_of_yardstick"] = row["training_loss_plus_backward"]["median_ms"] / base
        result["by_batch"][str(B)] = row
        print(json.dumps({"B": B, **row}))
        del saved, pg, dy, dhp, dsk, hs, pre, part, skip
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
