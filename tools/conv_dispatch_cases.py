#!/usr/bin/env python3
"""The case list that pins ap_conv2d_fwd's dispatch plan (audiopure_amd/csrc/ap_conv_plan.h), and where its golden comes from.

    python tools/conv_dispatch_cases.py --write-golden        CPU: plan every case, write tests/golden/conv_dispatch_v1.json; fails
                                                              unless the list reaches every kernel x tile x form of the product build
    python tools/conv_dispatch_cases.py --run                 GPU: every runnable case once through ap_conv2d_fwd / _slice, one line per
                                                              case with the plan and a SHA-256 of the output (run it under
                                                              `rocprofv3 --kernel-trace`, once per library: AUDIOPURE_HIP_LIB)
    python tools/conv_dispatch_cases.py --check-trace A.csv B.csv A.out B.out
                                                              the two kernel traces agree launch for launch, the hashes are equal, and
                                                              the plan's kernel / tile / grid of every case is what trace A shows
    python tools/conv_dispatch_cases.py --sweep-file F        the random sweep of tests/test_conv_plan_cpu.py as a text file, for the
                                                              sanitizer build of tests/conv_plan_driver.cpp (build_driver(.., True))
"""
import csv
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_dispatch_v1.json")
WS = 128 << 20                                                 # _native.CONV_WS_BYTES, what use_conv_workspace registers
FAMILY = ["generic", "few", "big", "big2", "split", "splith", "w3", "p1"]
FIELDS = ["rc", "family", "BM", "BN", "buf", "p1", "k3_nb", "splits", "reduce", "gx", "gy", "gz", "lds", "cls", "Ho", "Wo"]
SEED, SWEEP_N = 20260, 4000


def build_driver(outdir, sanitize=False):
    """tests/conv_plan_driver.cpp with the host compiler: a shared object for ctypes, or (sanitize) the stand-alone ASan + UBSan program"""
    src = os.path.join(ROOT, "tests", "conv_plan_driver.cpp")
    out = os.path.join(outdir, "conv_plan_asan" if sanitize else "libconv_plan.so")
    mode = ["-DDRIVER_MAIN", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-shared", "-fPIC"]
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + mode + [src, "-o", out], check=True)
    return out


def load(path):
    lib = C.CDLL(path)

    def plan(args, ws):
        out = (C.c_longlong * 16)()
        lib.ap_plan((C.c_int * 14)(*args), C.c_longlong(ws), out)
        d = dict(zip(FIELDS, list(out)))
        d["family"] = FAMILY[d["family"]]
        return {"rc": d["rc"]} if d["rc"] else d

    def images(Cout, Cin_g, kh, kw, groups):
        out = (C.c_longlong * 8)()
        lib.ap_plan_images(Cout, Cin_g, kh, kw, groups, out)
        return dict(zip(["has_frag", "has_w3", "frag_elems", "frag", "split", "splith", "w3", "total"], list(out)))
    return plan, images


def L(B, Cin, H, W, Cout, k, s=1, p=None, g=1, flags=0, kh=None, xcs=0, ocs=0, oco=0):
    """one layer as ap_plan's 14 ints (p: k // 2; kh: k; xcs: Cin)"""
    return [B, Cin, H, W, Cout, k if kh is None else kh, k, s, k // 2 if p is None else p, g, flags, xcs or Cin, ocs, oco]


def cases():
    """[(name, 14 ints, workspace?, runnable?)]"""
    out = []
    # test_gpu_convnet_steps.OFF_SQUARE and the square list of test_gpu_convnets.test_conv2d_primitive_edge_shapes (restated: importing
    # those modules needs the GPU fixtures), under the three flag words
    off = [(3, 8, 9, 5, 12, 3, 1, 1, 1, 1), (2, 16, 16, 10, 40, 3, 2, 1, 4, 0), (5, 33, 7, 4, 70, 1, 1, 0, 1, 1), (33, 32, 32, 20, 200, 3, 1, 1, 1, 1),
           (70, 64, 31, 18, 272, 3, 2, 1, 2, 1), (40, 48, 30, 17, 160, 1, 1, 0, 1, 0), (36, 24, 32, 12, 136, 3, 1, 1, 1, 1), (7, 32, 5, 9, 200, 3, 1, 1, 1, 1),
           (9, 128, 16, 6, 176, 3, 1, 1, 2, 0), (4, 16, 6, 11, 64, 3, 1, 2, 1, 1), (2, 8, 5, 8, 24, 5, 1, 4, 1, 0), (33, 32, 32, 40, 200, 3, 1, 1, 1, 1),
           (70, 64, 31, 36, 272, 3, 2, 1, 2, 1), (36, 24, 32, 30, 136, 3, 1, 1, 1, 1)]
    square = [(3, 8, 9, 12, 3, 1, 1, 1), (2, 16, 16, 40, 3, 2, 1, 4), (5, 33, 7, 70, 1, 1, 0, 1), (1, 64, 4, 64, 3, 1, 1, 8), (4, 1, 32, 64, 3, 1, 1, 1),
              (33, 32, 32, 200, 3, 1, 1, 1), (70, 64, 31, 272, 3, 2, 1, 2), (40, 48, 30, 160, 1, 1, 0, 1), (36, 24, 32, 136, 3, 1, 1, 1),
              (7, 32, 5, 200, 3, 1, 1, 1), (9, 128, 16, 176, 3, 1, 1, 2)]
    for fl in (0, 0x100, 0x400):
        for i, (B, Cin, H, W, Cout, k, s, p, g, relu) in enumerate(off):
            out.append((f"off{i}/{fl:#x}", L(B, Cin, H, W, Cout, k, s, p, g, relu | fl), True, True))
        for i, (B, Cin, H, Cout, k, s, p, g) in enumerate(square):
            out.append((f"sq{i}/{fl:#x}", L(B, Cin, H, H, Cout, k, s, p, g, 1 | fl), True, True))
    # test_split_k_and_few_output_paths...: the UNet's 4 x 4 map, with and without the workspace; Cout <= 4 (all eight instantiations)
    for ws in (True, False):
        out.append((f"splitk/ws{int(ws)}", L(64, 256, 4, 4, 256, 3), ws, True))
    for cout in (1, 2, 3, 4):
        for k in (3, 1):
            out.append((f"few{cout}k{k}", L(5, 128, 9, 7, cout, k, p=1), True, True))
    out.append(("slice/128x128", L(16, 128, 32, 32, 128, 3, ocs=192, oco=0), True, True))           # F(2,3) serves it
    out.append(("slice/pointwise", L(16, 256, 16, 16, 256, 1, ocs=384, oco=0), True, True))
    out.append(("slice/splitk", L(64, 256, 4, 4, 256, 3, ocs=512, oco=0), True, True))
    out.append(("slice/offset", L(8, 64, 16, 16, 192, 3, ocs=224, oco=16), True, True))
    out.append(("slice/refused", L(2, 24, 8, 8, 64, 3, ocs=96, oco=0), True, False))
    out.append(("1d/dil2", L(4, 64, 1, 1000, 128, 3, p=2, flags=0x200 | (2 << 16), kh=1), True, True))
    out.append(("1d/dil128", L(3, 64, 1, 777, 64, 3, p=128, flags=0x200 | (128 << 16), kh=1), True, True))
    # over 2 GB (x slab = B x_cstride H W 4 bytes): the pointer form of each tile -- planned, never run
    out.append(("2gb/128x128", L(4096, 16, 64, 64, 128, 3, xcs=32), True, False))
    out.append(("2gb/128x64", L(192, 16, 8, 8, 128, 3, xcs=1 << 17), True, False))
    out.append(("2gb/64x128", L(4096, 16, 64, 64, 64, 3, xcs=32), True, False))
    out.append(("2gb/64x64", L(1, 16, 8, 8, 128, 3, xcs=1 << 23), True, False))
    out.append(("w3/rt2/gather", L(32, 64, 16, 12, 256, 3), True, True))                              # F(2,3) forms: W / 2 no power of two
    out.append(("w3/rt1/gather", L(64, 64, 16, 12, 128, 3), True, True))
    out.append(("w3/rt2/nb", L(64, 64, 32, 32, 256, 3), True, True))
    out.append(("w3/rt2/nb/sliced", L(32, 64, 16, 16, 256, 3), True, True))
    out.append(("w3/rt1/gather/whole", L(683, 32, 16, 12, 128, 3), True, True))
    out.append(("w3/rt2/gather/whole", L(342, 32, 16, 12, 256, 3), True, True))
    # one step either side of each threshold, with and without the workspace
    pairs = {"tiles128>=512": (L(511, 16, 16, 8, 128, 3), L(512, 16, 16, 8, 128, 3)),
             "192-tile rule": (L(191, 16, 8, 8, 128, 3), L(192, 16, 8, 8, 128, 3)),
             "splitk small<192": (L(191, 64, 64, 1, 128, 3), L(192, 64, 64, 1, 128, 3)),
             "splitk t2": (L(191, 64, 128, 1, 128, 3), L(192, 64, 128, 1, 128, 3)),
             "splitk cap": (L(95, 256, 64, 1, 128, 3), L(96, 256, 64, 1, 128, 3)),
             "splitk K/(2S)>=16": (L(96, 1008, 8, 8, 128, 1), L(96, 1024, 8, 8, 128, 1)),
             "splitk K>=32": (L(96, 496, 8, 8, 128, 1), L(96, 512, 8, 8, 128, 1)),
             "w3 worth": (L(511, 64, 16, 16, 128, 3), L(512, 64, 16, 16, 128, 3)),
             "w3 32-tile floor": (L(31, 64, 16, 16, 128, 3), L(32, 64, 16, 16, 128, 3)),
             "w3 3 chunks (S=2)": (L(32, 32, 16, 16, 128, 3), L(32, 64, 16, 16, 128, 3)),
             "w3 3 chunks (S=4)": (L(32, 96, 16, 16, 128, 3), L(32, 128, 16, 16, 128, 3)),
             "Mg<128": (L(512, 16, 16, 8, 127, 3), L(512, 16, 16, 8, 128, 3))}
    for name, (lo, hi) in pairs.items():
        for ws in (True, False):
            out.append((f"{name}/below/ws{int(ws)}", lo, ws, True))
            out.append((f"{name}/at/ws{int(ws)}", hi, ws, True))
    return out


# what conv_launch can take in the product build: (family, BM, BN, buf, p1, k3_nb, K-sliced).  <128, 128, buf, p1> is built but never
# planned there (pointwise layers leave the 128 x 128 tile unless ap_debug_conv_path(2)).
REQUIRED = ({("big2", bm, bn, b, 0, 0, 0) for bm in (128, 64) for bn in (128, 64) for b in (0, 1)} | {("big2", 128, 64, 1, 1, 0, 0)}
            | {("big2", 128, 64, 1, 0, 0, 1), ("big2", 64, 64, 1, 0, 0, 1)}
            | {(f, bm, 128, b, 0, 0, 0) for f in ("split", "splith") for bm in (64, 128) for b in (0,)}
            | {("few", c, 256, 0, 0, k3, 0) for c in (1, 2, 3, 4) for k3 in (0, 1)} | {("big", 128, 128, 0, 0, 0, 0), ("generic", 64, 64, 0, 0, 0, 0)}
            | {("w3", bm, 192 - bm // 2, 0, 0, nb, s) for bm in (128, 256) for nb in (0, 1) for s in (0, 1)})


def form(p):
    big2 = p["family"] == "big2"                                 # (buf / p1 are forms of the streamed-weight kernel only)
    return (p["family"], p["BM"], p["BN"], p["buf"] * big2, p["p1"] * big2, p["k3_nb"], int(p["splits"] > 1))


def dump(plan):
    return [{"name": n, "args": a, "ws": WS if ws else 0, "run": run, "plan": plan(a, WS if ws else 0)} for n, a, ws, run in cases()]


def expected_launches(c, n_cu=256):
    """[(kernel name pattern, workgroups)] the plan of one golden case stands for"""
    p, tf = c["plan"], ("false", "true")
    name = {"big2": f"conv2d_f32_big2_kernel<{p['BM']}, {p['BN']}, {tf[p['buf']]}, {tf[p['p1']]}>", "split": f"conv2d_split_kernel<{p['BM']}, 128, false>",
            "splith": f"conv2d_split_kernel<{p['BM']}, 128, true>", "few": f"conv2d_few_kernel<{p['BM']}, {tf[p['k3_nb']]}>", "big": "conv2d_f32_big_kernel(",
            "generic": "conv2d_f32_kernel(", "w3": f"conv2d_w3_kernel<{p['BM'] // 128}, {tf[p['k3_nb']]}>"}[p["family"]]
    wgs = min(p["gx"], n_cu) if p["family"] == "w3" else p["gx"] * p["gy"] * p["gz"]
    total = c["args"][0] * c["args"][4] * p["Ho"] * p["Wo"]
    return [(name, wgs)] + ([("conv_splitk_reduce_kernel(", (total // 4 + 255) // 256 + 1)] if p["reduce"] else [])


def run_gpu():
    import torch
    sys.path.insert(0, ROOT)
    from audiopure_amd import _native as N
    assert N.CONV_WS_BYTES == WS
    lib, dev = N.lib(), torch.device("cuda:0")
    for i, c in enumerate(json.load(open(GOLDEN))):
        if not c["run"]:
            continue
        B, Cin, H, W, Cout, kh, kw, s, p, g, flags, xcs, ocs, oco = c["args"]
        torch.manual_seed(i)
        x, w, b = torch.randn(B, xcs, H, W, device=dev), torch.randn(Cout, Cin // g, kh, kw, device=dev) * 0.05, torch.randn(Cout, device=dev)
        res = torch.randn(B, Cout, c["plan"]["Ho"], c["plan"]["Wo"], device=dev)
        wT = torch.empty(lib.ap_conv2d_packed_elems(Cout, Cin // g, kh, kw, g), device=dev)
        N.check(lib.ap_conv2d_pack(N.ptr(w), None, N.ptr(wT), Cout, Cin // g, kh, kw, g, N.stream()))
        if c["ws"]:
            N.use_conv_workspace(dev)
        else:
            N.check(lib.ap_conv2d_set_workspace(None, 0))
        out = torch.full((B, ocs or Cout, c["plan"]["Ho"], c["plan"]["Wo"]), 7.0, device=dev)
        head = (N.ptr(x), N.ptr(wT), N.ptr(b), N.ptr(res), N.ptr(out), B, Cin, H, W, Cout, kh, kw, s, p, g, flags, xcs, 0)
        N.check(lib.ap_conv2d_fwd_slice(*head, ocs, oco, N.stream()) if ocs else lib.ap_conv2d_fwd(*head, N.stream()))
        torch.cuda.synchronize()
        print(f"case {c['name']}: {form(c['plan'])} grid {c['plan']['gx']} {c['plan']['gy']} {c['plan']['gz']} sha256 "
              f"{hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()}", flush=True)
    N.use_conv_workspace(dev)


def trace_rows(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    keep = [r for r in rows if re.search(r"conv2d_|conv_splitk_reduce", r["Kernel_Name"])]
    return [(r["Kernel_Name"], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"), int(r["LDS_Block_Size"]))
            for r in keep]


def check_trace(csv_a, csv_b, out_a, out_b):
    ta, tb = trace_rows(csv_a), trace_rows(csv_b)
    ha, hb = ([ln for ln in open(f).read().splitlines() if ln.startswith("case ")] for f in (out_a, out_b))
    print(f"trace A (parent library): {len(ta)} conv launches; trace B (this tree): {len(tb)}")
    bad = int(len(ta) != len(tb)) + sum(a != b for a, b in zip(ta, tb))
    print(f"launch for launch (kernel name, grid, workgroup size, LDS bytes): {'equal' if not bad else f'{bad} DIFFERENCES'}")
    bad_h = int(len(ha) != len(hb)) + sum(a != b for a, b in zip(ha, hb))
    print(f"output hashes of {len(ha)} cases: {'equal' if not bad_h else f'{bad_h} DIFFERENCES'}")
    it, bad_p = iter(ta), 0
    print("case | plan (kernel, workgroups) | trace A (kernel, grid in threads, workgroup, LDS bytes) | trace B kernel")
    ib = iter(tb)
    for c in json.load(open(GOLDEN)):
        if not c["run"]:
            continue
        for name, wgs in expected_launches(c):
            got, gb = next(it, None), next(ib, None)
            ok = got is not None and name in got[0] and got[1][0] * got[1][1] * got[1][2] == wgs * 256
            bad_p += not ok
            short = lambda r: "-" if r is None else re.sub(r"^void ap::|\(.*$", "", r[0])
            print(f"{c['name']} | {name.rstrip('(')} x {wgs} | {short(got)} {got and got[1:]} | {short(gb)} | {'ok' if ok else 'MISMATCH'}")
    bad_p += sum(1 for _ in it)
    print(f"plan against trace A: {'every case matches' if not bad_p else f'{bad_p} MISMATCHES'}")
    return 1 if bad or bad_h or bad_p else 0


def sweep(seed=SEED, n=SWEEP_N):
    """n random layers (14 ints + ws_bytes), skewed to the shapes where the rule branches"""
    r = np.random.RandomState(seed)
    rows = []
    for _ in range(n):
        g = int(r.choice([1, 1, 1, 2, 4, 8]))
        Cin, Cout = g * int(r.choice([1, 3, 8, 16, 24, 32, 64, 96, 128, 256, 512, 1024])), g * int(r.choice([1, 2, 3, 4, 10, 63, 64, 100, 127, 128, 200, 256, 384, 512]))
        k = int(r.choice([1, 3, 3, 5]))
        one_d = int(r.randint(0, 5) == 0)
        H, W = (1 if one_d else int(r.choice([1, 4, 4, 7, 8, 8, 16, 32, 64]))), int(r.choice([1, 2, 4, 4, 7, 8, 8, 12, 16, 32, 64, 130, 1000]))
        B = int(r.choice([1, 2, 7, 16, 31, 32, 64, 64, 96, 191, 192, 256, 511, 512, 2048, 65536]))
        dil = int(r.choice([1, 1, 2, 16])) if one_d else 1
        if r.randint(0, 4) == 0:                                   # a quarter: low-resolution maps with a long K, where K is sliced
            g, k, one_d, dil = 1, int(r.choice([1, 3])), 0, 1
            Cin, Cout, B = int(r.choice([128, 256, 512, 1024])), int(r.choice([128, 256, 512])), int(r.choice([4, 16, 31, 64, 96, 192]))
            H, W = int(r.choice([4, 8, 16])), int(r.choice([4, 8, 16]))
        flags = int(r.randint(0, 2)) | int(r.choice([0, 0, 0x100, 0x400])) | (0x200 if one_d else 0) | ((dil << 16) if dil > 1 else 0)
        sl = int(r.randint(0, 3) == 0)
        ocs, oco = (Cout + int(r.choice([0, 8, 64])), int(r.choice([0, 8]))) if sl else (0, 0)
        ocs = max(ocs, oco + Cout) if sl else 0
        ws = int(r.choice([0, 1 << 12, 1 << 20, WS, WS, WS, 1 << 34]))
        rows.append(L(B, Cin, H, W, Cout, k, int(r.choice([1, 1, 2])), int(r.randint(0, k // 2 + 2)) * dil, g, flags, kh=1 if one_d else k,
                      xcs=Cin + int(r.choice([0, 0, 16, 1 << 20])), ocs=ocs, oco=oco) + [ws])
    return rows


def main():
    import tempfile
    if "--run" in sys.argv:
        return run_gpu()
    if "--check-trace" in sys.argv:
        return check_trace(*sys.argv[sys.argv.index("--check-trace") + 1:][:4])
    if "--sweep-file" in sys.argv:
        with open(sys.argv[sys.argv.index("--sweep-file") + 1], "w") as f:
            f.writelines(" ".join(map(str, row)) + "\n" for row in sweep())
        return 0
    with tempfile.TemporaryDirectory() as d:
        plan, _ = load(build_driver(d))
        got = dump(plan)
    missing = REQUIRED - {form(c["plan"]) for c in got if not c["plan"]["rc"]}
    if missing:
        print("the case list does not reach:", sorted(missing))
        return 1
    if "--write-golden" in sys.argv:
        with open(GOLDEN, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(c) for c in got) + "\n]\n")
    print(f"{len(got)} cases, {len(REQUIRED)} forms reached")
    return 0


if __name__ == "__main__":
    sys.exit(main())
