#!/usr/bin/env python3
"""The case list that pins the residual block's dispatch plan (audiopure_amd/csrc/ap_block_plan.h), and where its golden comes from.

    python tools/block_dispatch_cases.py --write-golden       CPU: plan every case, write tests/golden/block_dispatch_v1.json; fails
                                                              unless the list reaches every family x instantiation of the product build
    python tools/block_dispatch_cases.py --run                GPU: every runnable case once through its public entry point, one line per
                                                              case with the plan and a SHA-256 of each output (run it under
                                                              `rocprofv3 --kernel-trace`, once per library: AUDIOPURE_HIP_LIB)
    python tools/block_dispatch_cases.py --check-trace A.csv B.csv A.out B.out
                                                              the two kernel traces agree launch for launch, the hashes are equal, and
                                                              the plan's kernel / tags / grid of every case is what trace A shows
    python tools/block_dispatch_cases.py --sweep-file F       the random sweep of tests/test_block_plan_cpu.py as a text file, for the
                                                              sanitizer build of tests/block_plan_driver.cpp (build_driver(.., True))
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "block_dispatch_v1.json")
FAMILY = ["f32_direct", "f32_f23", "split_direct", "split_f23", "bf16_p", "bf16_s", "bf16u_p", "bf16u_s"]
FIELDS = ["rc", "family", "tile", "save", "noh", "q16", "dcls", "diet", "ws", "rag", "ds", "savef", "e4", "d", "logd", "np", "ntiles", "ntiles2",
          "nblk", "nblk2", "grid", "grid2", "wg"]
SEED, SWEEP_N = 20261, 4000
F32, BF16, SPLIT, BSTORE = 0, 1, 2, 4                          # AP_PREC_*
MODES = {"f32d": (F32, 0), "f32": (F32, 1), "f32s": (SPLIT, 0), "f32sw": (SPLIT, 1), "bf16": (BF16, 1), "bf16s": (BSTORE, 1)}   # (precision, f32_form)
NL, CYCLE = 12, 12                                             # synth.mini_wavenet_config(C, 12, 12)
F32W_DIET = 5302                                               # AP_F32W_DIET of ap_resblock_f32w.hip (the kernel names of the trace carry it)


def build_driver(outdir, sanitize=False):
    """tests/block_plan_driver.cpp with the host compiler: a shared object for ctypes, or (sanitize) the stand-alone ASan + UBSan program"""
    src = os.path.join(ROOT, "tests", "block_plan_driver.cpp")
    out = os.path.join(outdir, "block_plan_asan" if sanitize else "libblock_plan.so")
    mode = ["-DDRIVER_MAIN", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-shared", "-fPIC"]
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + mode + [src, "-o", out], check=True)
    return out


def load(path):
    lib = C.CDLL(path)
    arr = lambda a: (C.c_longlong * 20)(*a)

    def plan(a):
        out, err = (C.c_longlong * 23)(), C.create_string_buffer(512)
        lib.ap_block(arr(a), out, err, 512)
        d = dict(zip(FIELDS, list(out)))
        d["family"] = FAMILY[d["family"]]
        return {"rc": d["rc"], "err": err.value.decode()} if d["rc"] else d

    def skipgemm(a, layer0, nl):
        out, err = (C.c_longlong * 6)(), C.create_string_buffer(512)
        lib.ap_skipgemm(arr(a), layer0, nl, out, err, 512)
        return {"rc": out[0], "err": err.value.decode()} if out[0] else dict(zip(["rc", "rag", "ntiles", "nblk", "grid", "wg"], list(out)))

    def final(a):
        out, err = (C.c_longlong * 7)(), C.create_string_buffer(512)
        lib.ap_final(arr(a), out, err, 512)
        return {"rc": out[0], "err": err.value.decode()} if out[0] else dict(zip(["rc", "bf16", "S", "tile", "ntiles", "grid", "wg"], list(out)))
    return {"plan": plan, "skipgemm": skipgemm, "final": final, "drops": lambda a: int(lib.ap_block_drops_last_h(arr(a)))}


def ask(mode, layer, B, L, out="plain", hout=True, C=256, n_cu=256):
    """the 20 values of the driver's ap_block: the context of `mode` at C = S channels (which weight images exist follows from the
    precision and C, as ap_ctx_load_wavenet builds them) and one call; out: plain | aout | gout | gout+fout"""
    prec, form = MODES[mode]
    bf = prec in (BF16, BSTORE)
    return [prec, C, C, NL, CYCLE, form, int(prec == F32 and C == 256), int(prec == SPLIT and C == 256), int(bf), int(bf), layer, B, L, n_cu,
            int(hout), int(out in ("plain", "aout")), int(out == "aout"), int(out.startswith("gout")), int(out == "gout+fout"), int(mode == "bf16s")]


def runnable(mode, out, hout, L, n_cu):
    """does a public per-block entry point reach this ask?  ap_resblock_fwd / _save need h_out (the fp32 modes' form without h' is
    the net's last layer: the ap_eps_fwd cases run it); _gate / _gate_save / _u / _u_save take a null h_out / u_out"""
    return n_cu == 256 and L < (1 << 20) and (hout or out.startswith("gout"))


def cases():
    """[(name, kind, ask or eps spec, runnable?)]"""
    out = []
    add = lambda name, mode, layer, B, L, o="plain", hout=True, C=256, n_cu=256, run=None: out.append(
        (name, "block", ask(mode, layer, B, L, o, hout, C, n_cu), runnable(mode, o, hout, L, n_cu) if run is None else run))
    outs = {"f32d": ("plain", "aout"), "f32": ("plain", "aout"), "f32s": ("plain",), "f32sw": ("plain",), "bf16": ("plain", "gout", "gout+fout"),
            "bf16s": ("gout", "gout+fout")}
    # every precision x form x outputs asked, with and without h' (u' on the u-image interface): one aligned and one ragged clip
    for mode in MODES:
        for o in outs[mode]:
            for hout in (True, False):
                for L in (256, 130):
                    add(f"form/{mode}/{o}/h{int(hout)}/L{L}", mode, 2, 2, L, o, hout)
    for Cc in (64, 128):                                         # the direct fp32 kernel's other widths (SAVE: 64 and 256 only)
        for L in (65, 128):
            add(f"direct/C{Cc}/plain/L{L}", "f32", 3, 3, L, C=Cc)
            add(f"direct/C{Cc}/aout/L{L}", "f32", 3, 3, L, "aout", C=Cc, run=Cc == 64)
    # clip lengths: ragged and L % 4 == 0, L < 4 for the split kernel, one tile / two tiles / a partial tile
    for mode, o in (("f32d", "plain"), ("f32", "plain"), ("f32s", "plain"), ("f32sw", "plain"), ("bf16", "plain"), ("bf16", "gout"), ("bf16", "gout+fout"),
                    ("bf16s", "gout"), ("bf16s", "gout+fout")):
        for L in (1, 3, 4, 63, 64, 65, 127, 128, 129, 130, 256, 258):
            add(f"len/{mode}/{o}/L{L}", mode, 2, 2, L, o)
    for mode in ("f32", "f32sw"):                                # F(2,3): L not a multiple of 2 d (d = 32: remainder below and above d)
        for L in (130, 100):
            add(f"pairs/{mode}/d32/L{L}", mode, 5, 2, L)
    # layers d = 1, 2, 4, 32, 64, 2048: every staging form, both quad classes; ragged d = 4 .. 32: the three-tap form
    for layer in (0, 1, 2, 5, 6, 11):
        for L in (128, 130):
            for mode, o, hout in (("f32", "plain", True), ("f32", "aout", True), ("f32", "plain", False), ("f32sw", "plain", True), ("bf16", "plain", True),
                                  ("bf16", "gout+fout", True), ("bf16", "gout+fout", False), ("bf16s", "gout", True)):
                add(f"layer{layer}/{mode}/{o}/h{int(hout)}/L{L}", mode, layer, 2, L, o, hout)
            add(f"layer{layer}/bf16/gout/persistent/L{L}", "bf16", layer, 260, L, "gout")     # 260 or 520 tiles: past the small-tile rule
            add(f"layer{layer}/bf16/gout/persistent/h0/L{L}", "bf16", layer, 260, L, "gout", False)
    for B in (256, 257):                                         # the one-tile-per-CU rule, either side
        add(f"small/bf16/B{B}", "bf16", 2, B, 128, "gout")
        add(f"small/bf16s/B{B}", "bf16s", 2, B, 128, "gout")
        add(f"small/bf16s/h0/B{B}", "bf16s", 2, B, 128, "gout", False)
    for n_cu in (256, 304, 64):                                  # grid rounding: below, at and above a group of 8, above the CU count
        for B, L in ((7, 128), (8, 128), (13, 128), (3, 16000)):
            for mode, o in (("f32", "plain"), ("bf16", "plain"), ("bf16", "gout+fout"), ("bf16s", "gout+fout")):
                add(f"grid/cu{n_cu}/{mode}/{o}/B{B}L{L}", mode, 2, B, L, o, n_cu=n_cu)
    # length limits: planned, never run
    for mode, o, Ls in (("bf16", "gout", (1 << 21, (1 << 22) - 1)), ("bf16", "plain", ((1 << 22),)), ("bf16s", "gout", (1 << 21, (1 << 22) - 1)),
                        ("f32", "plain", ((1 << 20) - 1, 1 << 20)), ("f32sw", "plain", ((1 << 21) - 1, 1 << 21)), ("bf16", "gout+fout", ((1 << 21) - 128,))):
        for L in Ls:
            add(f"limit/{mode}/{o}/L{L}", mode, 2, 1, L, o, run=False)
    add("limit/f32/tile-count", "f32", 11, 40000000, 2047, run=False)     # d > L: 64 tiles a clip where the predicate counts 33
    # each refusal once
    add("refuse/save outside f32", "f32s", 2, 2, 128, "aout", run=False)
    add("refuse/bf16s on the fp32 interface", "bf16s", 2, 2, 128, run=False)
    out[-1][2][19] = 0
    add("refuse/gout outside bf16", "f32", 2, 2, 128, "gout", run=False)
    add("refuse/bf16 channels", "bf16", 2, 2, 128, C=128, run=False)
    add("refuse/split channels", "f32s", 2, 2, 128, C=128, run=False)
    add("refuse/f23 save without h'", "f32", 2, 2, 128, "aout", False, run=False)
    add("refuse/direct without h'", "f32d", 2, 2, 128, hout=False, run=False)
    add("refuse/direct save channels", "f32", 2, 2, 128, "aout", C=128, run=False)
    add("refuse/direct channels", "f32", 2, 2, 128, C=32, run=False)
    add("refuse/u interface outside bf16s", "bf16", 2, 2, 128, "gout", run=False)
    out[-1][2][19] = 1
    add("refuse/u image too long", "bf16s", 2, 1, 1 << 22, "gout", run=False)
    add("refuse/g image too long", "bf16", 2, 1, 1 << 22, "gout", run=False)
    add("refuse/bf16 factor image too long", "bf16", 2, 1, 1 << 21, "gout+fout", run=False)
    add("refuse/bf16s factor image too long", "bf16s", 2, 1, 1 << 21, "gout+fout", run=False)
    # the siblings: skip GEMM (ragged or not, grid = min(tiles, CUs)) and final conv (bf16 or fp32 kernel, S, tile), with their refusals
    for B, L in ((2, 128), (2, 130), (3, 16000)):
        out.append((f"skipgemm/B{B}L{L}", "skipgemm", ask("bf16", 0, B, L, "gout"), True))
        for mode, Cc in (("f32", 64), ("f32", 128), ("f32", 256), ("bf16", 256), ("bf16s", 256)):
            out.append((f"final/{mode}/S{Cc}/B{B}L{L}", "final", ask(mode, 0, B, L, C=Cc), True))
    out.append(("skipgemm/refuse/no image", "skipgemm", ask("f32", 0, 2, 128), False))
    out.append(("skipgemm/refuse/too long", "skipgemm", ask("bf16", 0, 1, 1 << 21), False))
    out.append(("final/refuse/channels", "final", ask("f32", 0, 2, 128, C=32), False))
    # one ap_eps_fwd per mode: the merged sweep of run_net issues the launch sequence of the three it replaces
    for mode, G in (("f32d", 0), ("f32", 0), ("f32s", 0), ("f32sw", 0), ("bf16", 0), ("bf16", 5), ("bf16s", 0), ("bf16s", 5)):
        out.append((f"eps/{mode}/G{G}", "eps", {"mode": mode, "G": G, "B": 2, "L": 1000}, True))
    return out


def kernel_name(p):
    tf = lambda v: "true" if v else "false"
    return {"f32_direct": lambda: f"resblock_f32_kernel<{p['wg'] * 64 // p['tile']}, {p['tile']}, {tf(p['save'])}>",
            "f32_f23": lambda: f"resblock_f32w_kernel<{tf(p['noh'])}, {tf(p['save'])}, {tf(p['q16'])}, {F32W_DIET if p['q16'] else 0}, {p['dcls']}>",
            "split_direct": lambda: f"resblock_f32s_kernel<256, {tf(p['e4'])}, false>", "split_f23": lambda: "f32s_gate_kernel(",
            "bf16_p": lambda: f"resblock_bf16p_kernel<{p['ws']}, {tf(p['rag'])}, {tf(p['ds'])}, {tf(p['noh'])}, {tf(p['savef'])}>",
            "bf16_s": lambda: f"resblock_bf16s_kernel<{tf(p['noh'])}>", "bf16u_p": lambda: f"resblock_bf16u_kernel<{tf(p['noh'])}, {tf(p['savef'])}>",
            "bf16u_s": lambda: f"resblock_bf16us_kernel<{tf(p['noh'])}>"}[p["family"]]()


def block_launches(p):
    """[(kernel name pattern, threads of the grid)] one planned block stands for"""
    return [(kernel_name(p), p["grid"] * p["wg"])] + ([("f32s_out_kernel(", p["grid2"] * p["wg"])] if p["family"] == "split_f23" else [])


def skipgemm_launch(s):
    return ("skipgemm_bf16_kernel<" + ("true" if s["rag"] else "false") + ">", s["grid"] * s["wg"])


def final_launch(f):
    return ("final_bf16_kernel(" if f["bf16"] else f"final_f32_kernel<{f['S']}, {f['tile']}>", f["grid"] * f["wg"])


def eps_launches(drv, spec):
    """run_net + the final conv, restated over the driver's plans: groups of G layers, a skip GEMM behind each in the deferred-skip
    form, the last layer without h' where the plan has such a form"""
    mode, G, B, L = spec["mode"], spec["G"], spec["B"], spec["L"]
    u = mode == "bf16s"
    defer = u or (mode == "bf16" and G > 0)
    group = (G if G > 0 else NL) if defer else NL
    o = "gout" if defer else "plain"
    drop = drv["drops"](ask(mode, 0, B, L, o, False))
    seq = []
    for n0 in range(0, NL, group):
        nl = min(group, NL - n0)
        for n in range(n0, n0 + nl):
            seq += block_launches(drv["plan"](ask(mode, n, B, L, o, not (drop and n + 1 == NL))))
        if defer:
            seq.append(skipgemm_launch(drv["skipgemm"](ask(mode, 0, B, L, o), n0, nl)))
    return seq + [final_launch(drv["final"](ask(mode, 0, B, L)))]


def plan_of(drv, kind, a):
    if kind == "block":
        return drv["plan"](a)
    if kind == "skipgemm":
        return drv["skipgemm"](a, 0, 1)
    if kind == "final":
        return drv["final"](a)
    return {"launches": [list(x) for x in eps_launches(drv, a)]}


def dump(drv):
    return [{"name": n, "kind": kind, "ask": a, "run": run, "plan": plan_of(drv, kind, a)} for n, kind, a, run in cases()]


def expected_launches(c):
    p = c["plan"]
    return {"block": lambda: block_launches(p), "skipgemm": lambda: [skipgemm_launch(p)], "final": lambda: [final_launch(p)],
            "eps": lambda: [tuple(x) for x in p["launches"]]}[c["kind"]]()


def form(p):
    """the instantiation a planned block launches: family + every template tag"""
    return (p["family"], p["tile"], p["save"], p["noh"], p["q16"], p["dcls"] if p["q16"] else 4, p["ws"], p["rag"], p["ds"], p["savef"], p["e4"],
            p["wg"] if p["family"] == "f32_direct" else 0)           # (the direct kernel's width: 64 x C / tile threads)


def _required():
    """every family x instantiation launch_resblock / launch_resblock_bf16u can take in the product build"""
    req = {("f32_direct", 64, s, 0, 0, 4, 0, 0, 0, 0, 0, Cc) for Cc, s in ((64, 0), (128, 0), (256, 0), (64, 1), (256, 1))}   # (128-sample tiles: the tools build)
    req |= {("f32_f23", 64, s, n, q, dc if q else 4, 0, 0, 0, 0, 0, 0) for s, n in ((0, 0), (1, 0), (0, 1)) for q in (0, 1) for dc in (1, 2, 4)}
    req |= {("split_direct", 128, 0, 0, 0, 4, 0, 0, 0, 0, e4, 0) for e4 in (0, 1)} | {("split_f23", 128, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0)}
    for ws, rag in ((0, 0), (1, 0), (2, 0), (-1, 0), (1, 1), (2, 1), (-1, 1)):
        req |= {("bf16_p", 128, 0, n, 0, 4, ws, rag, ds, sf, 0, 0) for ds, n, sf in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1))}
    req |= {(f, 64, 0, n, 0, 4, 0, 0, 1, 0, 0, 0) for f in ("bf16_s", "bf16u_s") for n in (0, 1)}
    req |= {("bf16u_p", 128, 0, n, 0, 4, 0, 0, 1, sf, 0, 0) for n in (0, 1) for sf in (0, 1)}
    return req


REQUIRED = _required()


def run_gpu():
    import torch
    sys.path.insert(0, ROOT)
    from audiopure_amd import synth, _native as N
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.WaveNet import WaveNet_Speech_Commands
    dev, nets = torch.device("cuda:0"), {}
    sha = lambda t: hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]

    def engine(mode, Cc):
        if (mode, Cc) not in nets:
            cfg = synth.mini_wavenet_config(Cc, NL, CYCLE)
            net = WaveNet_Speech_Commands(**cfg)
            net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.wavenet_state_dict(cfg, 3).items()})
            nets[(mode, Cc)] = net.to(dev).set_precision(mode)
        return nets[(mode, Cc)], nets[(mode, Cc)].engine()

    for i, c in enumerate(json.load(open(GOLDEN))):
        if not c["run"]:
            continue
        torch.manual_seed(i)
        if c["kind"] == "eps":
            s = c["ask"]
            net, eng = engine(s["mode"], 256)
            eng.skip_group = s["G"]                                  # (bf16s: 0 = one group of all layers)
            res = {"eps": net.eps(torch.randn(s["B"], 1, s["L"], device=dev), 3.0)}
            eng.skip_group = min(eng.SKIP_GROUP, NL)
        else:
            a = c["ask"]
            Cc, layer, B, L, hout, _, aout, gout, fout, u = [a[1]] + a[10:13] + a[14:]
            mode = {F32: ("f32d", "f32"), SPLIT: ("f32s", "f32sw"), BF16: ("bf16",) * 2, BSTORE: ("bf16s",) * 2}[a[0]][a[5]]
            net, eng = engine(mode, Cc)
            lib, ctx, st = eng.lib, eng.ctx, N.stream()
            h, pt = torch.randn(B, Cc, L, device=dev), torch.randn(Cc, device=dev) * 0.5
            res = {}
            if c["kind"] == "final":
                res["eps"] = torch.empty(B, L, device=dev)
                N.check(lib.ap_final_affine(ctx, N.ptr(h), None, N.ptr(res["eps"]), None, 0.0, 0.0, 0.0, None, 0, 0, 0, B, L, st))
            elif c["kind"] == "skipgemm":
                g, res["skip"] = torch.randn(B, L, Cc, device=dev).to(torch.bfloat16), torch.randn(B, Cc, L, device=dev)
                N.check(lib.ap_skip_gemm(ctx, 3, 1, g.data_ptr(), N.ptr(res["skip"]), 1, B, L, st))
            else:
                if hout:
                    res["h"] = torch.zeros(B, Cc, L, device=dev, dtype=torch.bfloat16 if u else torch.float32)
                if gout:
                    res["g"] = torch.zeros(B, L, Cc, device=dev, dtype=torch.bfloat16)
                if fout:
                    res["f"] = torch.zeros(lib.ap_gate_factor_bytes(B, L), device=dev, dtype=torch.uint8)
                if aout:
                    res["a"] = torch.zeros(B, 2 * Cc, L, device=dev)
                if not gout:
                    res["skip"] = torch.randn(B, Cc, L, device=dev)
                ho = res["h"].data_ptr() if hout else None
                if u:
                    uin = h.to(torch.bfloat16)
                    args = (ctx, layer, uin.data_ptr(), N.ptr(pt) if hout else None, ho, res["g"].data_ptr())
                    N.check(lib.ap_resblock_fwd_u_save(*args, res["f"].data_ptr(), B, L, st) if fout else lib.ap_resblock_fwd_u(*args, B, L, st))
                elif gout:
                    args = (ctx, layer, N.ptr(h), N.ptr(pt), ho, res["g"].data_ptr())
                    N.check(lib.ap_resblock_fwd_gate_save(*args, res["f"].data_ptr(), B, L, st) if fout else lib.ap_resblock_fwd_gate(*args, B, L, st))
                elif aout:
                    N.check(lib.ap_resblock_fwd_save(ctx, layer, N.ptr(h), N.ptr(pt), ho, N.ptr(res["skip"]), N.ptr(res["a"]), 1, B, L, st))
                else:
                    N.check(lib.ap_resblock_fwd(ctx, layer, N.ptr(h), N.ptr(pt), ho, N.ptr(res["skip"]), 1, B, L, st))
        torch.cuda.synchronize()
        launches = " + ".join(f"{n.rstrip('(')} x {t}" for n, t in expected_launches(c)) if c["kind"] != "eps" else f"{len(c['plan']['launches'])} launches"
        print(f"case {c['name']}: {launches} sha256 " + " ".join(f"{k}={sha(v)}" for k, v in sorted(res.items())), flush=True)


KERNELS = r"resblock_|f32s_gate_kernel|f32s_out_kernel|skipgemm_bf16|final_(f32|bf16)_kernel"


def _demangled(name):
    """rocprofv3 leaves a name mangled where its demangler does not know a parameter type (__bf16: resblock_bf16s_kernel): the
    one-bool template of namespace ap, as the other names read"""
    m = re.match(r"_ZN2ap\d+(\w+?)ILb([01])EEE", name)
    return f"void ap::{m.group(1)}<{'true' if m.group(2) == '1' else 'false'}>(" if m else name


def trace_rows(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        r["Kernel_Name"] = _demangled(r["Kernel_Name"])
    keep = [r for r in rows if re.search(r"\bap::", r["Kernel_Name"])]                    # every kernel of the library, in launch order
    return [(r["Kernel_Name"], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"), int(r["LDS_Block_Size"]))
            for r in keep]


def check_trace(csv_a, csv_b, out_a, out_b):
    ta, tb = trace_rows(csv_a), trace_rows(csv_b)
    ha, hb = ([ln for ln in open(f).read().splitlines() if ln.startswith("case ")] for f in (out_a, out_b))
    print(f"trace A (parent library): {len(ta)} launches of the library's kernels; trace B (this tree): {len(tb)}")
    bad = int(len(ta) != len(tb)) + sum(a != b for a, b in zip(ta, tb))
    print(f"launch for launch (kernel name, grid, workgroup size, LDS bytes): {'equal' if not bad else f'{bad} DIFFERENCES'}")
    bad_h = int(len(ha) != len(hb)) + sum(a != b for a, b in zip(ha, hb))
    print(f"output hashes of {len(ha)} cases: {'equal' if not bad_h else f'{bad_h} DIFFERENCES'}")
    pick = lambda t: iter([r for r in t if re.search(KERNELS, r[0])])                     # (not the pack / embed / init-conv kernels)
    it, ib, bad_p = pick(ta), pick(tb), 0
    short = lambda r: "-" if r is None else re.sub(r"^void ap::|\(.*$", "", r[0])
    print("case | plan (kernel x threads) | trace A (kernel, grid in threads, workgroup, LDS bytes) | trace B kernel")
    for c in json.load(open(GOLDEN)):
        if not c["run"]:
            continue
        exp, n_bad = expected_launches(c), 0
        for k, (name, threads) in enumerate(exp):
            got, gb = next(it, None), next(ib, None)
            ok = got is not None and name in got[0] and got[1][0] * got[1][1] * got[1][2] == threads
            n_bad += not ok
            if c["kind"] != "eps" or not ok:
                print(f"{c['name']}{'' if c['kind'] != 'eps' else f' launch {k}'} | {name.rstrip('(')} x {threads} | {short(got)} {got and got[1:]} | {short(gb)} | "
                      f"{'ok' if ok else 'MISMATCH'}")
        if c["kind"] == "eps":
            print(f"{c['name']} | {len(exp)} launches: " + ", ".join(sorted({n.split('<')[0].rstrip('(') for n, _ in exp})) + f" | {'ok' if not n_bad else 'MISMATCH'}")
        bad_p += n_bad
    bad_p += sum(1 for _ in it)
    print(f"plan against trace A: {'every case matches' if not bad_p else f'{bad_p} MISMATCHES'}")
    return 1 if bad or bad_h or bad_p else 0


def sweep(seed=SEED, n=SWEEP_N):
    """n random asks (the 20 values of ap_block), skewed to the shapes where the rule branches; about one in five is refused"""
    r = np.random.RandomState(seed)
    valid = {F32: ["plain", "plain", "aout"], SPLIT: ["plain"], BF16: ["plain", "gout", "gout+fout"], BSTORE: ["gout", "gout+fout"]}
    rows = []
    for _ in range(n):
        mode = str(r.choice(list(MODES)))
        Cc = int(r.choice([256] * 12 + [64, 128, 32, 512]))
        if Cc in (64, 128) and r.randint(0, 4):
            mode = str(r.choice(["f32", "f32d"]))                # (the widths only the direct fp32 kernel is built for)
        B = int(r.choice([1, 2, 3, 7, 8, 13, 64, 255, 256, 257, 512, 65536]))
        L = int(r.choice([1, 3, 4, 63, 64, 65, 127, 128, 129, 130, 256, 258, 1000, 16000, int(r.randint(1, 70000)), int(r.randint(1, 70000))]))
        if r.randint(0, 8) == 0:                                 # the length limits
            L = int(r.choice([(1 << 20) - 4, 1 << 20, 1 << 21, (1 << 22) - 1, 1 << 22]))
        o = str(r.choice(valid[MODES[mode][0]]))                 # outputs the mode has an entry point for ...
        if r.randint(0, 12) == 0:
            o = str(r.choice(["plain", "aout", "gout", "gout+fout"]))   # ... and now and then any
        hout = bool(r.randint(0, 4)) or (MODES[mode][0] in (F32, SPLIT) and (mode != "f32" or o == "aout") and bool(r.randint(0, 8)))
        a = ask(mode, int(r.randint(0, NL)), B, L, o, hout, Cc, int(r.choice([256, 256, 304, 64, 8, 1])))
        if r.randint(0, 16) == 0:
            a[2] = int(r.choice([64, 128, 256]))                 # skip channels of their own
        if r.randint(0, 24) == 0:
            a[19] = 1 - a[19]                                    # the other interface
        if r.randint(0, 16) == 0:
            a[6] = a[7] = 0                                      # (no F(2,3) image)
        rows.append(a)
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
        got = dump(load(build_driver(d)))
    missing = REQUIRED - {form(c["plan"]) for c in got if c["kind"] == "block" and not c["plan"]["rc"]}
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
