"""The residual block's dispatch rule (audiopure_amd/csrc/ap_block_plan.h) pinned on the CPU: the header behind
tests/block_plan_driver.cpp, built with the host compiler into tmp_path and loaded with ctypes -- nothing of the GPU library is loaded.
The golden's plans were matched against a kernel trace of the library before the plan existed (profiles/block_plan_dispatch_trace.txt)."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import block_dispatch_cases as D  # noqa: E402


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return D.load(D.build_driver(str(tmp_path_factory.mktemp("block_plan"))))


def test_plan_equals_golden(driver):
    """Kernel family, every template tag, dilation, tile counts, grid(s), workgroup size -- or the refusal's code and text -- of every
    committed case: each precision x form x outputs asked with and without h', the clip lengths either side of a tile and of L % 4,
    the layers of every staging form and quad class, the one-tile-per-CU rule, the grid rounding at two more CU counts, the length
    limits, each refusal, the skip GEMM, the final conv, and the launch sequence of one ap_eps_fwd per mode.  The list reaches every
    family x instantiation launch_resblock and launch_resblock_bf16u can take in the product build."""
    golden = json.load(open(D.GOLDEN))
    got = D.dump(driver)
    assert [c["name"] for c in got] == [c["name"] for c in golden]
    for g, c in zip(got, golden):
        assert g == c, (c["name"], g["plan"], c["plan"])
    assert not D.REQUIRED - {D.form(c["plan"]) for c in golden if c["kind"] == "block" and not c["plan"]["rc"]}
    refusals = {c["plan"]["err"] for c in golden if c["plan"].get("rc")}
    assert len(refusals) >= 17 and all(refusals)                # every refusal text of the three plans but the two no product build reaches


def test_a_pair_either_side_of_each_threshold_differs(driver):
    by = {c["name"]: c["plan"] for c in json.load(open(D.GOLDEN))}
    fam = lambda n: by[n]["family"]
    assert (fam("small/bf16/B256"), fam("small/bf16/B257")) == ("bf16_s", "bf16_p")                 # one 128-sample tile per CU of 256
    assert (fam("small/bf16s/B256"), fam("small/bf16s/B257")) == ("bf16u_s", "bf16u_p")
    assert (by["len/f32/plain/L127"]["q16"], by["len/f32/plain/L128"]["q16"]) == (0, 1)             # L % 4
    assert (by["len/bf16/plain/L129"]["rag"], by["len/bf16/plain/L128"]["rag"]) == (1, 0)
    assert (by["len/bf16/plain/L129"]["ws"], by["len/bf16/plain/L128"]["ws"]) == (-1, 0)            # ragged d = 4: the three-tap form
    assert (by["len/f32s/plain/L3"]["e4"], by["len/f32s/plain/L4"]["e4"]) == (0, 1)                 # L >= 4
    assert [by[f"len/bf16/plain/L{L}"]["ntiles"] for L in (128, 129, 256, 258)] == [1, 2, 2, 3]
    assert [by[f"layer{n}/bf16/plain/h1/L128"]["ws"] for n in (0, 1, 2, 5, 6, 11)] == [1, 2, 0, 0, -1, -1]
    assert [by[f"layer{n}/f32/plain/h1/L128"]["dcls"] for n in (0, 1, 2, 11)] == [1, 2, 4, 4]
    assert [by[f"grid/cu256/bf16/plain/B{B}L128"]["grid"] for B in (7, 8, 13)] == [7, 8, 8]           # whole groups of 8 from 8 on
    assert [by[f"grid/cu{cu}/bf16/plain/B3L16000"]["grid"] for cu in (256, 304, 64)] == [256, 304, 64]
    assert [by[f"grid/cu{cu}/f32/plain/B13L128"]["grid"] for cu in (256, 64)] == [26, 26]             # (fp32 F(2,3): 64-sample tiles, not rounded)
    assert by["pairs/f32/d32/L130"]["np"] == 66 and by["pairs/f32/d32/L100"]["np"] == 64              # 2 x 32 + min(2, 32); 32 + min(36, 32)
    assert by["limit/f32/plain/L1048575"]["family"] == "f32_f23" and by["limit/f32/plain/L1048576"]["family"] == "f32_direct"
    assert by["limit/f32sw/plain/L2097151"]["family"] == "split_f23" and by["limit/f32sw/plain/L2097152"]["family"] == "split_direct"
    assert by["limit/bf16s/gout/L4194303"]["rc"] == 0 and by["refuse/u image too long"]["rc"] == -22
    assert by["limit/bf16/gout+fout/L2097024"]["rc"] == 0 and by["refuse/bf16 factor image too long"]["rc"] == -22
    assert by["limit/f32/tile-count"] == {"rc": 1, "err": "resblock: too many tiles for the minimal-filtering block"}   # (1, as found)
    # the last layer drops h' exactly where the launch has a form without it
    drops = lambda mode, o: driver["drops"](D.ask(mode, 0, 2, 1000, o, True))
    assert [drops(m, "plain") for m in ("f32d", "f32", "f32s", "f32sw", "bf16")] == [0, 1, 0, 0, 0]
    assert drops("bf16", "gout") == 1 and drops("bf16s", "gout") == 1


def test_sweep_invariants(driver):
    """Over a fixed random sweep: no zero grid dimension; a persistent grid never above min(tiles, CUs); a small-tile family only at
    B * ceil(L / 128) <= 256; NOH only where no h' was asked for; SAVE / SAVEF only where the buffer was given; the F(2,3) families only
    at C = S = 256 in form 1 with the image present; a refusal returns -22 and a text.  tests/block_plan_driver.cpp -DDRIVER_MAIN runs
    the same sweep (tools/block_dispatch_cases.py --sweep-file) under ASan + UBSan outside Python."""
    plan = driver["plan"]
    rows = D.sweep()
    assert len(rows) == D.SWEEP_N >= 3000 and rows == D.sweep()
    seen, refused = set(), 0
    for a in rows:
        p = plan(a)
        C_, S_, form, w1w, w1w_s, B, L, n_cu, hout, aout, fout = a[1], a[2], a[5], a[6], a[7], a[11], a[12], a[13], a[14], a[16], a[18]
        if p["rc"]:
            refused += 1
            assert p["rc"] == -22 and p["err"], (a, p)
            continue
        fam = p["family"]
        seen.add(fam)
        assert p["grid"] >= 1 and p["wg"] >= 64 and (fam != "split_f23" or p["grid2"] >= 1), (a, p)
        if fam in ("f32_f23", "bf16_p", "bf16u_p"):
            assert p["grid"] <= min(p["nblk"], n_cu), (a, p)
        else:
            assert p["grid"] == p["nblk"], (a, p)
        if fam in ("bf16_s", "bf16u_s"):
            assert B * ((L + 127) // 128) <= 256, (a, p)
        assert not (p["noh"] and hout) and not (p["save"] and not aout) and not (p["savef"] and not fout), (a, p)
        if fam in ("f32_f23", "split_f23"):
            assert C_ == S_ == 256 and form == 1 and (w1w if fam == "f32_f23" else w1w_s), (a, p)
    assert seen == set(D.FAMILY) and 300 < refused < 1200, (seen, refused)      # most asks are launches; every kind of refusal is met
