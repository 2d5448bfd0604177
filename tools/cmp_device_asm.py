#!/usr/bin/env python3
"""Is the device code of two source trees the same?  No GPU needed.

    python tools/cmp_device_asm.py [--by-symbol] <tree A> <tree B> [source.hip ...]

Compiles every source of HIP_SOURCES (product flags) and of HIP_SOURCES + TOOLS_ONLY_SOURCES (-DAP_TOOLS) of both trees to gfx950
assembly with the flags build_hip gives that file plus `--cuda-device-only -S`, and compares the two outputs line by line.  Dropped
before comparing: comment lines, `.file` / `.ident` lines and the `__hip_cuid_<hash>` symbol (a hash of the source text).
Prints identical/different per file and exits 1 if any file differs -- the check of a refactor that must not move an instruction.
--by-symbol: a file that differs line by line still counts as identical if its symbols are the same set and every symbol's text
(function, kernel descriptor, metadata entry; the function's running number taken out of local labels) is the same -- a reordered
host launcher changes the order in which template instantiations are emitted and nothing else.  By symbol, three more things that
move with a symbol's position and not with its code are left out of its text: the remark behind a local label (`; in Loop: ...`,
padded to a column by the label's width), bare `.text` lines (there or not by whether a template's own section follows), and the
file's tail (`.p2alignl` padding, `.AMDGPU.gpr_maximums`, the metadata's `amdhsa.target` / `amdhsa.version`), which is compared
under the key "" and not as part of whichever symbol happens to come last.  Every differing symbol is listed.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G  # noqa: E402


def device_asm(tree, name, tools):
    csrc = os.path.join(tree, "audiopure_amd", "csrc")
    src = os.path.join(csrc, name)
    if not os.path.exists(src):
        src = os.path.join(tree, "tools", "csrc", name)
    flags = [csrc if f == G.CSRC else f for f in G.hip_flags(src, tools)]
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", src, "-o", "-"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + p.stderr)
    keep = []
    for line in p.stdout.splitlines():
        t = line.strip()
        if not t or t.startswith((";", "//", ".file", ".ident")) or "__hip_cuid_" in t:
            continue
        keep.append(line)
    return keep


_ANNOUNCE = re.compile(r"^\s*(?:\.(?:globl|weak|protected|hidden)\s+([^\s,]+)|\.section\s+\.text\.([^\s,]+),)")
_LOCAL = re.compile(r"(\.L|Header=|Loop )(BB|func_begin|func_end|tmp)\d+")   # "Loop ": the `; Parent Loop BB<n>_<k>` remark behind a label


def by_symbol(lines):
    """{symbol: its lines}: function text + kernel descriptor (from the first directive that names the symbol to the next symbol's)
    and, under "meta:<symbol>", its entry of the metadata's kernel list; "" holds what belongs to no symbol.  The per-function
    number in local labels (.LBB<n>_<k>, .Lfunc_end<n>) is dropped: it is the function's position in the file; so are a label's
    trailing remark (padded by that number's width) and bare `.text` lines."""
    out, key, meta = {}, "", False
    for line in lines:
        if ".amdgpu_metadata" in line:
            meta, key = not line.strip().startswith(".end"), ""
        if meta and line.startswith("  - "):
            key = ("meta", len(out))                    # named by the entry's own .name line below
        elif not meta:
            m = _ANNOUNCE.match(line)
            if m:
                key = m.group(1) or m.group(2)
        if (meta and line.startswith("amdhsa.")) or ".p2alignl" in line or ".AMDGPU.gpr_maximums" in line:
            key = ""                                    # the file's own tail, not the last symbol's
        if meta and isinstance(key, tuple) and line.startswith("    .name:"):
            out["meta:" + line.split()[1]] = out.pop(key)
            key = "meta:" + line.split()[1]
        if line.strip() == ".text":                     # switches back from a template's own section: there or not by what follows
            continue
        line = _LOCAL.sub(r"\1\2", line)
        if line.startswith(".L"):                       # a label's remark is padded to a column that moves with the number's width
            line = line.split(";")[0].rstrip()
        out.setdefault(key, []).append(line)
    return out


def main():
    args = [x for x in sys.argv[1:] if x != "--by-symbol"]
    sym = "--by-symbol" in sys.argv[1:]
    a, b = (os.path.abspath(p) for p in args[:2])
    jobs = [(n, False) for n in G.HIP_SOURCES] + [(n, True) for n in G.HIP_SOURCES + G.TOOLS_ONLY_SOURCES]
    if args[2:]:
        jobs = [j for j in jobs if j[0] in args[2:]]
    with ThreadPoolExecutor(int(os.environ.get("MAX_JOBS", "8"))) as ex:
        res = list(ex.map(lambda j: (device_asm(a, *j), device_asm(b, *j)), jobs))
    bad = 0
    for (name, tools), (xa, xb) in zip(jobs, res):
        same, note = xa == xb, ""
        if not same and sym:                            # the same symbols with the same text, emitted in another order
            sa, sb = by_symbol(xa), by_symbol(xb)
            diff = sorted(k for k in set(sa) | set(sb) if sa.get(k) != sb.get(k))
            same, note = not diff, f"  ({len(sa)} symbols, order differs)" if not diff else "  differing symbols:" + "".join("\n    " + str(k) for k in diff)
        bad += not same
        print(f"{'tools  ' if tools else 'product'} {name:28s} {len(xa):7d} lines  {'identical' if same else 'DIFFERENT'}{note}")
    print(f"{len(jobs) - bad} of {len(jobs)} identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
