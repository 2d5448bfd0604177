"""tools/isa_read_distance.py: the parser on a short synthetic listing (no compiler, no GPU)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_read_distance", os.path.join(ROOT, "tools", "isa_read_distance.py"))
ird = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ird)

MFMA = "\tv_mfma_f32_32x32x2_f32 a[0:15], v1, v2, a[0:15]\n"
LISTING = (
    "\t.text\n"
    "_Z5otherv:                              ; @_Z5otherv\n"
    "\tv_add_f32_e32 v0, v0, v1\n"
    "\ts_endpgm\n"
    "; NumVgprs: 3\n; NumAgprs: 0\n; ScratchSize: 0\n"
    "_Z4kernv:                               ; @_Z4kernv\n"
    "\tds_read_b128 v[0:3], v9\n"                                  # waited for at once: 0
    "\ts_waitcnt lgkmcnt(0)\n"
    + MFMA
    + "\tds_read_b128 v[4:7], v9 offset:16\n"                      # two MFMAs, then retired by lgkmcnt(1): 2
    + MFMA * 2
    + "\tds_read_b32 v8, v9\n"                                     # (a place in the queue, not reported)
    "\tv_add_f32_e32 v0, v0, v1\n"
    "\ts_waitcnt vmcnt(3) lgkmcnt(1)\n"
    + MFMA
    + "\tds_write_b128 v9, v[0:3]\n"                               # LDS writes count in the in-order queue
    "\tds_read_b128 v[0:3], v9 offset:32\n"                        # carried over the barrier: 1 + 3 = 4+
    + MFMA
    + "\ts_waitcnt vmcnt(0)\n"                                     # (no lgkmcnt: retires nothing)
    "\ts_barrier\n"
    + MFMA * 3
    + "\ts_waitcnt lgkmcnt(0)\n"
    ".LBB1_2:                                ; =>This Inner Loop Header: Depth=1\n"
    + MFMA
    + "\tds_read_b128 v[4:7], v9\n"                                # never waited for
    "\ts_cbranch_scc1 .LBB1_2\n"
    "\ts_endpgm\n"
    "; NumVgprs: 243\n; NumAgprs: 256\n; TotalNumVgprs: 500\n; ScratchSize: 16\n"
)


def test_parser_on_a_synthetic_listing():
    kernels = ird.parse(LISTING)
    assert [k["name"] for k in kernels] == ["_Z5otherv", "_Z4kernv"]
    k = kernels[1]
    assert (k["vgpr"], k["agpr"], k["scratch"], k["valu"]) == (243, 256, 16, 1)
    regions = k["regions"]
    assert [(r["end"], r["mfma"]) for r in regions] == [("barrier", 5), ("label", 3), ("branch", 1)]
    assert regions[0]["reads"] == ["0", "2", "4+"]
    assert regions[1]["reads"] == []
    assert regions[2]["reads"] == [None]


def test_kernel_filter_and_report():
    kernels = ird.parse(LISTING, "kern")
    assert [k["name"] for k in kernels] == ["_Z4kernv"]
    text = ird.report(kernels)
    assert "VGPRs 243  AGPRs 256  scratch 16 B" in text
    assert "0 2 4+" in text and text.rstrip().splitlines()[-1].endswith(": -")
