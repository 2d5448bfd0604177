"""Same-process A/Bs of the F(2,3) fp32 block (tools build).

   python tools/ab_f32w.py [--out FILE]      the GEMM1 diet: the kernel before it (tools/csrc/ap_resblock_f32w_parent.hip) against the
                                             present source with no item, each item alone (carried prefetch, constants in LDS) and
                                             both; B = 256 and 512, layers 0, 5, 11; interleaved repeats; the table goes
                                             to FILE (default profiles/f32w_diet_ab.txt, whose records -- everything from its first
                                             line that starts with "== " -- are kept)
   python tools/ab_f32w.py --edges [--out FILE]   the h' epilogue under MFMAs: DIET mask 6 (the diet alone) against 22 (GEMM2 by rows, the
                                             res tiles leaving under the skip rows: the product), the parent kernel beside them;
                                             same method; default FILE profiles/f32w_edges_ab.txt
   python tools/ab_f32w.py --pk [--out FILE]      fewer vector-ALU slots: DIET mask 22 (the product before this change) against each new
                                             bit alone on top of it -- 54 (pair gate and transform), 150 (no zeroing of m1, m3, m4) --
                                             and 182 (both: the product); same
                                             method; default FILE profiles/f32w_pk_ab.txt
   python tools/ab_f32w.py --seam [--out FILE]    MFMAs through the chunk turn: DIET mask 182 (the product before this change) against 1206
                                             (the chunk's barrier in its last unit, the next chunk's first fragment behind it, X requested
                                             in MFMA gaps: the product); same method; default FILE profiles/f32w_seam_ab.txt, whose record
                                             holds the run with the two removed bits (694, 2230) and all three (3766)
   python tools/ab_f32w.py --quad [--out FILE]    wider and fewer memory instructions: DIET mask 1206 (the product before this change) against
                                             5302 (X staged by channel and pair quad, four 16-byte loads per chunk: the product); same
                                             method, layers 0, 2, 5, 11; default FILE profiles/f32w_quad_ab.txt, whose record holds the run
                                             with the removed bit (9398) and both (13494)
   python tools/ab_f32w.py --epilogue [B]    the two epilogue forms: 16-byte stores through LDS patches (clip lengths that are
                                             multiples of four) against the 4-byte form every other length takes"""
import os
import sys

import _toolslib  # noqa: F401
import ctypes as C

import torch

from audiopure_amd import synth, _native as N
from audiopure_amd.diffusion_models.DiffWave_Unconditional.WaveNet import WaveNet_Speech_Commands

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDS_MARK = "\n== "                                           # the sections tools/ab_f32w.py does not write: kept across runs
DIET = [("parent", None), ("no item", 0), ("carry", 2), ("const", 4), ("both", 6)]
EDGES = [("parent", None), ("mask 6", 6), ("rows", 22)]
PK = [("mask 22", 22), ("pairs", 54), ("zero", 150), ("both", 182)]
SEAM = [("mask 182", 182), ("seam", 1206)]
QUAD = [("mask 1206", 1206), ("quad", 5302)]
PRODUCT_MASK = 5302
DIET_HEAD = ["F(2,3) fp32 block, GEMM1 diet: ms per launch (HIP events, 6 launches after 2), L = 16000, accumulate = 1, h' form, one process,",
             "the variants interleaved within each repeat; median of 3 repeats [min .. max]; gain against the parent kernel.",
             "parent = the kernel before the diet (tools/csrc/ap_resblock_f32w_parent.hip); the others are ap_resblock_f32w.hip with DIET mask",
             "0 (no item), 2 (carried weight prefetch, no X request past chunk 7), 4 (b1, b2, part_t in LDS), 6 (both).", ""]
EDGES_HEAD = ["F(2,3) fp32 block, the h' epilogue under MFMAs: ms per launch (HIP events, 6 launches after 2), L = 16000, accumulate = 1,",
              "h' form, one process, the variants interleaved within each repeat; median of 3 repeats [min .. max]; gain against mask 6.",
              "parent = tools/csrc/ap_resblock_f32w_parent.hip (the kernel before the GEMM1 diet); the others are ap_resblock_f32w.hip with DIET",
              "mask 6 (the diet alone: the product before this change) and 22 (+ DIET_ROWS_: the product).", ""]
PK_HEAD = ["F(2,3) fp32 block, fewer vector-ALU issue slots: ms per launch (HIP events, 6 launches after 2), L = 16000, accumulate = 1,",
           "h' form, one process, the variants interleaved within each repeat; median of 3 repeats [min .. max]; gain against mask 22.",
           "ap_resblock_f32w.hip with DIET mask 22 (the product before this change), 54 (+ DIET_PK_: output transform and gate on register",
           "pairs), 150 (+ DIET_ZERO_: chunk 0 peeled, m1, m3, m4 start from the instruction's constant 0) and 182 (both: the product).", ""]
SEAM_HEAD = ["F(2,3) fp32 block, MFMAs through the chunk turn: ms per launch (HIP events, 6 launches after 2), L = 16000, accumulate = 1,",
             "h' form, one process, the variants interleaved within each repeat; median of 3 repeats [min .. max]; gain against mask 182.",
             "ap_resblock_f32w.hip with DIET mask 182 (the product before this change) and 1206 (+ DIET_SEAM_: the chunk's barrier in its last",
             "unit, the next chunk's first fragment behind it, the X request in unit 13's gaps: the product).", ""]
QUAD_HEAD = ["F(2,3) fp32 block, wider and fewer memory instructions: ms per launch (HIP events, 6 launches after 2), L = 16000, accumulate = 1,",
             "h' form, one process, the variants interleaved within each repeat; median of 3 repeats [min .. max]; gain against mask 1206.",
             "ap_resblock_f32w.hip with DIET mask 1206 (the product before this change) and 5302 (+ DIET_QUAD_: X staged by (channel, quad of",
             "four pairs), four 16-byte loads per chunk, part_t from the LDS copy, packed adds: the product).", ""]


def setup(B):
    dev = torch.device("cuda:0")
    cfg = synth.mini_wavenet_config(256, 12, 12)
    net = WaveNet_Speech_Commands(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.wavenet_state_dict(cfg, 3).items()})
    net = net.to(dev)
    eng = net.engine()
    L = 16000
    hd = torch.rand(B, 256, L, device=dev) * 3 - 1.5
    hout = torch.empty_like(hd)
    sk = torch.zeros_like(hd)
    pt = torch.rand(256, device=dev)
    return net, eng, (hd, pt, hout, sk, B, L)


def timer(call, n=6):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        call()
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def epilogue_ab(B):
    net, eng, (hd, pt, hout, sk, B, L) = setup(B)
    lib = eng.lib
    lib.ap_debug_f32w_q16.argtypes = [C.c_int]
    for rep in range(2):
        for layer in (0, 5, 11):
            call = lambda: N.check(lib.ap_resblock_fwd(eng.ctx, layer, N.ptr(hd), N.ptr(pt), N.ptr(hout), N.ptr(sk), 1, B, L, N.stream()))
            t16 = timer(call)
            lib.ap_debug_f32w_q16(0)
            t4 = timer(call)
            lib.ap_debug_f32w_q16(1)
            print(f"layer {layer:2d}  16-byte epilogue: {t16:7.3f} ms   4-byte epilogue: {t4:7.3f} ms", flush=True)


def diet_ab(out, DIET=DIET, head=DIET_HEAD, base_name="parent", layers=(0, 5, 11)):
    lines = list(head)
    for B in (256, 512):
        net, eng, (hd, pt, hout, sk, B, L) = setup(B)
        lib = eng.lib
        lib.ap_debug_f32w_diet.argtypes = [C.c_int]
        lib.ap_debug_resblock_f32w_parent.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_void_p] * 2
        for layer in layers:
            new = lambda: N.check(lib.ap_resblock_fwd(eng.ctx, layer, N.ptr(hd), N.ptr(pt), N.ptr(hout), N.ptr(sk), 1, B, L, N.stream()))
            old = lambda: N.check(lib.ap_debug_resblock_f32w_parent(eng.ctx, layer, N.ptr(hd), N.ptr(pt), N.ptr(hout), N.ptr(sk), 1, B, L,
                                                                    N.stream(), None))
            ts = {name: [] for name, _ in DIET}
            for rep in range(3):
                for name, mask in DIET:
                    if mask is None:
                        ts[name].append(timer(old))
                    else:
                        assert lib.ap_debug_f32w_diet(mask) == 0
                        ts[name].append(timer(new))
            assert lib.ap_debug_f32w_diet(PRODUCT_MASK) == 0
            base = sorted(ts[base_name])[1]
            for name, _ in DIET:
                v = sorted(ts[name])
                lines.append(f"B={B:3d} layer {layer:2d}  {name:8s} {v[1]:8.3f} ms  [{v[0]:8.3f} .. {v[2]:8.3f}]  {100 * (base - v[1]) / base:+6.2f} %")
                print(lines[-1], flush=True)
            lines.append("")
        del net, eng, hd, pt, hout, sk
        torch.cuda.empty_cache()
    keep = []
    if os.path.exists(out):
        old_text = open(out).read()
        if RECORDS_MARK in old_text:
            keep = [old_text[old_text.index(RECORDS_MARK) + 1:].rstrip("\n")]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines + keep) + "\n")


def main():
    if "--epilogue" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--epilogue"]
        return epilogue_ab(int(rest[0]) if rest else 256)
    edges, pk, seam, quad = "--edges" in sys.argv, "--pk" in sys.argv, "--seam" in sys.argv, "--quad" in sys.argv
    out = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
           else os.path.join(ROOT, "profiles", "f32w_quad_ab.txt" if quad else "f32w_seam_ab.txt" if seam else "f32w_pk_ab.txt" if pk else "f32w_edges_ab.txt" if edges else "f32w_diet_ab.txt"))
    if quad:
        diet_ab(out, QUAD, QUAD_HEAD, "mask 1206", layers=(0, 2, 5, 11))
    elif seam:
        diet_ab(out, SEAM, SEAM_HEAD, "mask 182")
    elif pk:
        diet_ab(out, PK, PK_HEAD, "mask 22")
    elif edges:
        diet_ab(out, EDGES, EDGES_HEAD, "mask 6")
    else:
        diet_ab(out)


if __name__ == "__main__":
    main()
