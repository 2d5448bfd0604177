"""Time the baseline defenses (AS / MS / AT / DS / LPF / BPF) on the GPU, forward and backward, at B = 512 x L = 16000 and
B = 10, next to a PyTorch-operator restatement of AS (F.conv1d), MS (unfold + median) and DS (the strided-conv resampler)
in the same process on the same GPU.

    python tools/bench_defenses.py [--iters 20] [--out profiles/defense_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o defenses -- python tools/bench_defenses.py --iters 5 --no-torch
    python tools/bench_defenses.py --summarize <dir>/defenses_kernel_trace.csv [--out profiles/defense_kernel_times.txt]

Times are device-event means over ``--iters`` calls after a warm-up; the rocprofv3 run gives per-kernel times
(``*_kernel_stats.csv``); ``--summarize`` turns its kernel trace into the median time of every library kernel per batch size
(the grid's y extent is the batch for the per-clip-tiled kernels; x / 1024 for AT's one-workgroup-per-clip launches).  Needs a
GPU; there is no CPU mode (``--summarize`` only reads a trace)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiopure_amd.transforms import defense_design as D  # noqa: E402
from audiopure_amd.transforms import defenses as DF  # noqa: E402


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # microseconds per call


def _native(name, x, g):
    z = torch.randn_like(x)
    fwd = {"AS": lambda t: DF.AS(t), "MS": lambda t: DF.MS(t), "AT": lambda t: DF.AT(t, noise=z),
           "DS": lambda t: DF.DS(t), "LPF": lambda t: DF.LPF(t), "BPF": lambda t: DF.BPF(t)}[name]

    def f():
        with torch.no_grad():
            fwd(x)

    def fb():
        t = x.detach().requires_grad_(True)
        fwd(t).backward(g)
    return f, fb


def _torch_ops(name, x, g):
    """PyTorch-operator restatements (the reference's own operator choices for AS / MS; the torchaudio 0.11 resampler's
    pad + strided conv1d for DS)."""
    dev = x.device
    if name == "AS":
        w = torch.full((1, 1, 3), 1.0 / 3, device=dev)
        fwd = lambda t: F.conv1d(t.unsqueeze(1), w, padding=1).squeeze(1)          # noqa: E731
    elif name == "MS":
        fwd = lambda t: torch.median(F.pad(t, (1, 1)).unfold(-1, 3, 1), -1)[0]     # noqa: E731
    elif name == "DS":
        kd, ku = D.ds_taps()
        kd = torch.from_numpy(kd).view(1, 1, -1).to(dev)
        ku = torch.from_numpy(ku).view(2, 1, -1).to(dev)

        def fwd(t):
            B, L = t.shape
            d = F.conv1d(F.pad(t, (13, 15)).unsqueeze(1), kd, stride=2).reshape(B, -1)[:, :(L + 1) // 2]
            u = F.conv1d(F.pad(d, (7, 8)).unsqueeze(1), ku).transpose(1, 2).reshape(B, -1)
            return u[:, :L]
    else:
        return None

    def f():
        with torch.no_grad():
            fwd(x)

    def fb():
        t = x.detach().requires_grad_(True)
        fwd(t).backward(g)
    return f, fb


def summarize(trace, out=None):
    import collections
    import csv
    times = collections.defaultdict(list)
    for r in csv.DictReader(open(trace)):
        name = r["Kernel_Name"]
        if "ap::" not in name:
            continue
        short = name.replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
        gx, gy = int(r["Grid_Size_X"]), int(r["Grid_Size_Y"])
        if short.startswith("iir_carry_kernel"):           # one thread per clip, 64 per workgroup
            B = f"<={gx}"
        elif short.startswith("at_"):
            B = gx // int(r["Workgroup_Size_X"])
        else:
            B = gy
        times[(short, B)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    lines = [f"{'kernel':32s} {'B':>8s} {'calls':>6s} {'median us':>10s}"]
    for (k, B), v in sorted(times.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))):
        lines.append(f"{k:32s} {str(B):>8s} {len(v):6d} {sorted(v)[len(v) // 2]:10.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as fh:
            fh.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize", default=None, help="a rocprofv3 kernel-trace CSV to summarise (no GPU needed)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-torch", action="store_true", help="native ops only (for the rocprofv3 kernel-trace run)")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, args.out)
    assert torch.cuda.is_available(), "bench_defenses needs a GPU"
    dev = torch.device("cuda:0")
    rows = []
    for B in (512, 10):
        L = 16000
        gen = torch.Generator(device=dev).manual_seed(B)
        x = (torch.rand(B, L, device=dev, generator=gen) - 0.5).contiguous()
        g = torch.randn(B, L, device=dev, generator=gen)
        for name in ("AS", "MS", "AT", "DS", "LPF", "BPF"):
            f, fb = _native(name, x, g)
            row = {"op": name, "B": B, "L": L, "native_fwd_us": _time(f, args.iters),
                   "native_fwd_bwd_us": _time(fb, args.iters)}
            t = None if args.no_torch else _torch_ops(name, x, g)
            if t is not None:
                row["torch_ops_fwd_us"] = _time(t[0], args.iters)
                row["torch_ops_fwd_bwd_us"] = _time(t[1], args.iters)
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
