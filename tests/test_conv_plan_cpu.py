"""ap_conv2d_fwd's dispatch rule (audiopure_amd/csrc/ap_conv_plan.h) pinned on the CPU: the header behind tests/conv_plan_driver.cpp,
built with the host compiler into tmp_path and loaded with ctypes -- nothing of the GPU library is loaded.  The golden's plans were
matched against a kernel trace of the library before the plan existed (profiles/conv_plan_dispatch_trace.txt)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import conv_dispatch_cases as D  # noqa: E402


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return D.load(D.build_driver(str(tmp_path_factory.mktemp("conv_plan"))))


def test_plan_equals_golden(driver):
    """Kernel family, tile, form, K slices, grid, dynamic LDS and profile class of every committed case: the layers of the GPU tests
    under the three flag words, split-K / few-output / sliced / 1-D / over-2-GB layers and a pair either side of every threshold,
    with and without a workspace.  The list reaches every form conv_launch can take in the product build."""
    plan, _ = driver
    golden = json.load(open(D.GOLDEN))
    got = D.dump(plan)
    assert [c["name"] for c in got] == [c["name"] for c in golden]
    for g, c in zip(got, golden):
        assert g == c, (c["name"], g["plan"], c["plan"])
    assert not D.REQUIRED - {D.form(c["plan"]) for c in golden if not c["plan"]["rc"]}
    # the class sequences tests/test_gpu_convnet_steps.py records for its two layer lists (printed on the MI355X before the plan existed)
    seq = lambda prefix, fl: [c["plan"]["cls"] for c in golden if c["name"].startswith(prefix) and c["name"].endswith(f"/{fl:#x}")]
    assert seq("sq", 0) == [5, 5, 5, 5, 5, 0, 0, 2, 4, 2, 1] and seq("off", 0) == [5, 5, 5, 2, 2, 2, 5, 2, 1, 1, 5, 0, 0, 4]
    for fl in (0x100, 0x400):
        assert seq("sq", fl) == [5, 5, 5, 5, 5, 3, 3, 3, 4, 3, 3] and seq("off", fl) == [5, 5, 5, 3, 3, 3, 5, 3, 3, 3, 5, 3, 3, 4]
    # a pair either side of a threshold differs
    by = {c["name"]: c["plan"] for c in golden}
    for name in {c["name"].split("/below/")[0] for c in golden if "/below/" in c["name"]}:
        assert by[f"{name}/below/ws1"] != by[f"{name}/at/ws1"], name


def _packed_elems(Cout, Cin_g, kh, kw, groups):
    """ap_conv2d_packed_elems as it stood before conv_images, restated"""
    up4 = lambda n: (n + 3) & ~3
    n = Cout * Cin_g * kh * kw
    nf = groups * ((Cout // groups + 31) // 32) * 32 * Cin_g * kh * kw
    if Cin_g % 16 == 0 and Cout // groups >= 64:
        n = up4(n) + nf + up4(nf * 3 // 2) + up4(nf)
    if kh == 3 and kw == 3 and groups == 1 and Cin_g % 32 == 0 and Cout % 128 == 0:
        n = up4(n) + 4 * Cout * Cin_g * 3
    return n


def test_image_offsets_are_aligned_disjoint_and_sum_to_the_closed_form(driver):
    _, images = driver
    kinds = set()
    for groups in (1, 2, 4):
        for cout_g in (1, 3, 10, 63, 64, 65, 96, 127, 128, 136, 256, 384):
            for Cin_g in (1, 3, 8, 16, 24, 31, 32, 48, 64, 96, 129, 256):
                for kh, kw in ((1, 1), (3, 3), (1, 3), (5, 5), (3, 1)):
                    Cout = cout_g * groups
                    im = images(Cout, Cin_g, kh, kw, groups)
                    n = Cout * Cin_g * kh * kw
                    assert im["total"] == _packed_elems(Cout, Cin_g, kh, kw, groups), (Cout, Cin_g, kh, kw, groups)
                    spans = [(0, n)]
                    if im["has_frag"]:
                        nf = im["frag_elems"]
                        spans += [(im["frag"], nf), (im["split"], (nf * 3 + 1) // 2), (im["splith"], nf)]
                    if im["has_w3"]:
                        spans.append((im["w3"], 4 * Cout * Cin_g * 3))
                    for (o0, n0), (o1, _) in zip(spans, spans[1:] + [(im["total"], 0)]):
                        assert o0 % 4 == 0 and o0 + n0 <= o1 < o0 + n0 + 4, (Cout, Cin_g, kh, kw, groups, spans)
                    kinds.add(len(spans) - 1)
    assert kinds == {0, 3, 4}                                  # shapes with none, three and all four extra images


def test_sweep_invariants(driver):
    """Over a fixed random sweep: a plan never asks for more partial-sum bytes than the workspace holds, never splits K with groups,
    never has a zero grid dimension, and serves a sliced output only from the streamed-weight fp32 kernel or (as the library has done
    since the F(2,3) kernel took the UNet's 3 x 3 layers, output slice included) from that kernel's F(2,3) form -- never from the
    split-operand, few-output, LDS-staged or generic kernels.  tests/conv_plan_driver.cpp -DDRIVER_MAIN runs the same sweep
    (tools/conv_dispatch_cases.py --sweep-file) under ASan + UBSan outside Python."""
    plan, _ = driver
    rows = D.sweep()
    assert len(rows) == D.SWEEP_N >= 3000 and rows == D.sweep()
    planned = sliced = split = 0
    for row in rows:
        a, ws = row[:14], row[14]
        p = plan(a, ws)
        if p["rc"]:
            assert p["rc"] == -22
            continue
        planned += 1
        if p["splits"] > 1:
            split += 1
            assert p["reduce"] and a[9] == 1, row
            assert p["splits"] * a[0] * a[4] * p["Ho"] * p["Wo"] * 4 <= ws, row
        else:
            assert not p["reduce"]
        if a[12] and (a[12] != a[4] or a[13]):
            sliced += 1
            assert p["family"] in ("big2", "w3") and not a[10] & 0x500, row
        assert p["gx"] >= 1 and p["gy"] >= 1 and p["gz"] >= 1, row
    assert planned > 2000 and sliced > 100 and split > 50, (planned, sliced, split)
