#!/usr/bin/env python3
"""Is the device code of two source trees the same?  No GPU needed.

    python tools/cmp_device_asm.py <tree A> <tree B> [source.hip ...]

Compiles every source of HIP_SOURCES (product flags) and of HIP_SOURCES + TOOLS_ONLY_SOURCES (-DAP_TOOLS) of both trees to gfx950
assembly with the flags build_hip gives that file plus `--cuda-device-only -S`, and compares the two outputs line by line.  Dropped
before comparing: comment lines, `.file` / `.ident` lines and the `__hip_cuid_<hash>` symbol (a hash of the source text).
Prints identical/different per file and exits 1 if any file differs -- the check of a refactor that must not move an instruction.
"""
import os
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


def main():
    a, b = (os.path.abspath(p) for p in sys.argv[1:3])
    jobs = [(n, False) for n in G.HIP_SOURCES] + [(n, True) for n in G.HIP_SOURCES + G.TOOLS_ONLY_SOURCES]
    if sys.argv[3:]:
        jobs = [j for j in jobs if j[0] in sys.argv[3:]]
    with ThreadPoolExecutor(int(os.environ.get("MAX_JOBS", "8"))) as ex:
        res = list(ex.map(lambda j: (device_asm(a, *j), device_asm(b, *j)), jobs))
    bad = 0
    for (name, tools), (xa, xb) in zip(jobs, res):
        same = xa == xb
        bad += not same
        print(f"{'tools  ' if tools else 'product'} {name:28s} {len(xa):7d} lines  {'identical' if same else 'DIFFERENT'}")
    print(f"{len(jobs) - bad} of {len(jobs)} identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
