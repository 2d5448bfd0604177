#!/usr/bin/env python
"""Time one native train step of the Improved-Diffusion UNet at the shipped configuration (script_util.py:15-35: 128 channels, 3 res
blocks, (1, 2, 2, 2), attention at 16 and 8, 4 heads, dropout 0.3): ``zero_grad`` + ``training_losses`` + ``.mean().backward()``
(UNetModel.forward_train, ap_unet_train.hip, ap_conv2d_wgrad) at B = 230 (the reference's batch per rank, spect_train_mpi_run.sh) and
B = 16, and where it goes per kernel.  The yardstick is the same step through torch-ROCm's own operators on the SAME module in the same
process: a plain-torch walk of the holder module with ``F.dropout``.  Device events around synchronised windows, median of 5 after 2
warm-ups (as tools/bench_train_step.py); the per-kernel split is one profiled step.  Writes profiles/unet_train_bench.json (or --out).

    python tools/bench_unet_train.py [--out FILE] [--repeats 5] [--batches 230 16]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from audiopure_amd import synth  # noqa: E402
from audiopure_amd.diffusion_models.improved_diffusion_ddpm import GaussianTables  # noqa: E402
from audiopure_amd.diffusion_models.improved_diffusion_train import training_losses  # noqa: E402
from audiopure_amd.diffusion_models.improved_diffusion_unet import create_model, model_and_diffusion_defaults  # noqa: E402
from bench_m5_train import per_kernel  # noqa: E402
from bench_train_step import timed  # noqa: E402
from synth_convnets import synth_init  # noqa: E402


def _silu(x):
    return x * torch.sigmoid(x)


def torch_eps(m, x, t, p):
    """unet.py:462-491 on the holder module's parameters through torch's operators, nn.Dropout(p) live (F.dropout)"""
    def gn(g, h):
        return F.group_norm(h, g.num_groups, g.weight, g.bias, g.eps)

    def run(seq, h, emb):
        for layer in seq:
            name = type(layer).__name__
            if name == "ResBlock":
                r = layer.in_layers[2](_silu(gn(layer.in_layers[0], h)))
                scale, shift = torch.chunk(layer.emb_layers[1](_silu(emb))[..., None, None], 2, dim=1)
                r = F.dropout(_silu(gn(layer.out_layers[0], r) * (1 + scale) + shift), p, training=True)
                h = layer.skip_connection(h) + layer.out_layers[3](r)
            elif name == "AttentionBlock":
                b, c, *spatial = h.shape
                xf = h.reshape(b, c, -1)
                qkv = layer.qkv(gn(layer.norm, xf)).reshape(b * layer.num_heads, -1, xf.shape[2])
                ch = qkv.shape[1] // 3
                q, k, v = torch.split(qkv, ch, dim=1)
                s = 1 / math.sqrt(math.sqrt(ch))
                w = torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1)
                h = (xf + layer.proj_out(torch.einsum("bts,bcs->bct", w, v).reshape(b, -1, xf.shape[2]))).reshape(b, c, *spatial)
            elif name == "Downsample":
                h = layer.op(h)
            elif name == "Upsample":
                h = layer.conv(F.interpolate(h, scale_factor=2, mode="nearest"))
            else:
                h = layer(h)
        return h

    half = m.model_channels // 2
    args = t[:, None].float() * m._freqs[None]
    emb = m.time_embed[2](_silu(m.time_embed[0](torch.cat([torch.cos(args), torch.sin(args)], dim=-1))))
    hs, h = [], x
    for blk in m.input_blocks:
        h = run(blk, h, emb)
        hs.append(h)
    h = run(m.middle_block, h, emb)
    for blk in m.output_blocks:
        h = run(blk, torch.cat([h, hs.pop()], dim=1), emb)
    assert half * 2 == m.model_channels
    return m.out[2](_silu(gn(m.out[0], h)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet_train_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[230, 16])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_unet_train needs a GPU"
    dev = torch.device("cuda:0")
    cfg = model_and_diffusion_defaults()
    m = synth_init(create_model(**cfg), 0).to(dev).train()
    p, tb = m.dropout_p, GaussianTables(cfg["diffusion_steps"])
    result = {"config": {"model": "create_model(**model_and_diffusion_defaults())", "dropout": p, "image": [1, 32, 32],
                         "step": "zero_grad + training_losses(model, x, t)['loss'].mean().backward()"}, "by_batch": {}}
    for B in args.batches:
        x0 = torch.from_numpy(synth.uniform("bench/unet/x", (B, 1, 32, 32), 0, -1.0, 1.0)).to(dev)
        z = torch.from_numpy(synth.normal("bench/unet/z", (B, 1, 32, 32), 0)).to(dev)
        t = (torch.arange(B) * 7) % tb.T
        a = torch.from_numpy(tb.sqrt_ac[t.numpy()].astype(np.float32)).to(dev).reshape(-1, 1, 1, 1)
        b = torch.from_numpy(tb.sqrt_1m_ac[t.numpy()].astype(np.float32)).to(dev).reshape(-1, 1, 1, 1)
        td = t.to(dev)

        def native():
            m.zero_grad(set_to_none=True)
            training_losses(m, x0, t, noise=z, tables=tb)["loss"].mean().backward()

        def through_torch():
            m.zero_grad(set_to_none=True)
            eps = torch_eps(m, a * x0 + b * z, td, p)
            ((z - eps) ** 2).flatten(1).mean(1).mean().backward()

        row = {"native_step": timed(native, args.warmup, args.repeats),
               "torch_operator_step": timed(through_torch, args.warmup, args.repeats)}
        row["native_over_torch"] = row["native_step"]["median_ms"] / row["torch_operator_step"]["median_ms"]
        row["native_per_kernel"] = per_kernel(native)[:24]
        row["torch_operator_per_kernel"] = per_kernel(through_torch)[:12]
        result["by_batch"][str(B)] = row
        print(json.dumps({"B": B, **{k: v for k, v in row.items() if not k.endswith("per_kernel")}}))
        for r in row["native_per_kernel"]:
            print(f"    {r['total_us']:9.1f} us  x{r['launches']:<3d} {r['kernel']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
