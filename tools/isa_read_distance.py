"""How far ahead of its use does the compiled kernel issue each LDS fragment read?  Host only: no GPU.

   python tools/isa_read_distance.py SOURCE.hip [--tools] [--kernel SUBSTRING] [--flags "-D..."] [--out FILE]
   python tools/isa_read_distance.py --asm LISTING.s [--kernel SUBSTRING] [--out FILE]

Compiles SOURCE with the flags the build gives it (__graft_entry__.hip_flags; -S --cuda-device-only) and, per kernel and per region of
its static code -- a region ends at an s_barrier, a branch or a branch target -- prints for every ds_read_b128, in program order, the number of
v_mfma instructions between the read and the s_waitcnt lgkmcnt(N) that retires it.  A read still in flight at its region's end
is followed into the code that comes next in the listing and its distance marked "+" (carried over a barrier or a loop's back
edge; "-": never waited for).  LDS reads retire in order, so a read is retired by the first wait whose N is not larger than the
number of LDS instructions issued behind it.  Beside the distances: VGPRs / AGPRs / scratch bytes of the kernel and the static
count of vector-ALU instructions that are not MFMAs.

The parser looks at v_mfma, ds_ (reads, and writes as places in the in-order LDS queue), s_waitcnt, s_barrier, branch and label lines
only (and counts the lines that start with v_).  Scalar loads share the lgkmcnt counter and are not followed, so a wait that only
retires those shows up as a wait for the reads in front of it: distances are lower bounds.  profiles/f32w_seam_isa.txt is this script's output for the fp32
F(2,3) block."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_LGKM = re.compile(r"lgkmcnt\((\d+)\)")
_KERNEL = re.compile(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$")
_LABEL = re.compile(r"^\.LBB\d+_\d+:")


def parse(text, kernel_filter=None):
    """-> list of kernels: {"name", "vgpr", "agpr", "scratch", "valu", "regions": [{"line", "end", "mfma", "reads": ["3", "15+" or None]}]}"""
    kernels, cur, region, pending, total = [], None, None, [], 0

    def close_region(end, lineno):
        nonlocal region
        if region is not None:
            for p in pending:                                     # still in flight at the region's end: followed in static order
                p[3] = True
            region["end"] = end
            if region["mfma"] or region["reads"]:
                cur["regions"].append(region)
        region = {"line": lineno + 1, "end": None, "mfma": 0, "reads": []}

    for lineno, raw in enumerate(text.splitlines(), 1):
        line = raw.strip()
        if cur is None:
            m = _KERNEL.match(raw)
            if m and not raw.startswith("."):
                cur = {"name": m.group(1), "vgpr": None, "agpr": None, "scratch": None, "valu": 0, "regions": []}
                region, pending, total = None, [], 0
                close_region(None, lineno)
            continue
        if line.startswith("; NumVgprs:"):
            cur["vgpr"] = int(line.split(":")[1])
        elif line.startswith("; NumAgprs:"):
            cur["agpr"] = int(line.split(":")[1])
        elif line.startswith("; ScratchSize:"):
            cur["scratch"] = int(line.split(":")[1])
            if kernel_filter is None or kernel_filter in cur["name"]:
                kernels.append(cur)
            cur = None
        elif region is None:
            continue
        elif line.startswith("s_endpgm"):
            close_region("end", lineno)
            region = None
        elif line.startswith("v_mfma"):
            region["mfma"] += 1
            total += 1
        elif line.startswith("v_"):
            cur["valu"] += 1
        elif line.startswith("ds_"):
            for p in pending:
                p[2] += 1                                         # one more LDS operation behind it
            if line.startswith("ds_read_b128"):
                pending.append([region["reads"], total, 0, False, len(region["reads"])])
                region["reads"].append(None)
            else:
                pending.append([None, total, 0, False, 0])
        elif line.startswith("s_waitcnt"):
            m = _LGKM.search(line)
            if m:
                n = int(m.group(1))
                for p in [p for p in pending if p[2] >= n]:
                    if p[0] is not None:
                        p[0][p[4]] = f"{total - p[1]}{'+' if p[3] else ''}"
                    pending.remove(p)
        elif line.startswith("s_barrier"):
            close_region("barrier", lineno)
        elif line.startswith("s_cbranch") or line.startswith("s_branch"):
            close_region("branch", lineno)
        elif _LABEL.match(line):
            close_region("label", lineno)
    return kernels


def report(kernels):
    out = []
    for k in kernels:
        out.append(f"{k['name']}")
        out.append(f"  VGPRs {k['vgpr']}  AGPRs {k['agpr']}  scratch {k['scratch']} B  non-MFMA vector-ALU instructions (static) {k['valu']}")
        for r in k["regions"]:
            if not r["reads"] and r["mfma"] == 0:
                continue
            d = " ".join("-" if x is None else str(x) for x in r["reads"])
            out.append(f"  line {r['line']:6d} .. {r['end'] or '':7s} {r['mfma']:4d} MFMAs, {len(r['reads']):3d} ds_read_b128: {d}")
        out.append("")
    return "\n".join(out)


def compile_to_asm(src, tools=False, extra=()):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + G.hip_flags(src, tools) + list(extra) + ["-S", "--cuda-device-only", src, "-o", "-"]
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode()


def main(argv):
    def opt(name):
        return argv[argv.index(name) + 1] if name in argv else None
    values = {opt(n) for n in ("--asm", "--kernel", "--flags", "--out")}
    pos = [a for a in argv if not a.startswith("--") and a not in values]
    if opt("--asm"):
        text, what = open(opt("--asm")).read(), opt("--asm")
    else:
        if not pos:
            print(__doc__)
            return 2
        extra = (opt("--flags") or "").split()
        text = compile_to_asm(pos[0], "--tools" in argv, extra)
        what = os.path.relpath(os.path.abspath(pos[0]), ROOT) + (" " + " ".join(extra) if extra else "") + (" (tools build)" if "--tools" in argv else "")
    body = (f"{what}: v_mfma instructions between each ds_read_b128 and the s_waitcnt lgkmcnt that retires it, per region of the\n"
            f"static code, in program order ('+': carried past the region's end)  [tools/isa_read_distance.py]\n\n"
            + report(parse(text, opt("--kernel"))))
    if opt("--out"):
        with open(opt("--out"), "w") as f:
            f.write(body)
    else:
        print(body)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
