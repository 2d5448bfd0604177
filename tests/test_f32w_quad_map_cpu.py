"""The quad staging's lane map (tests/f32w_quad_map.py restates it from audiopure_amd/csrc/ap_resblock_f32w.hip), host only: for
all twelve dilations and L in {64, 192, 196, 4096, 16000}, every (product, column, k) of a chunk image is written exactly once,
from the sample the 4-byte staging takes; every 16-byte piece is aligned and wholly inside or wholly outside the clip; a 32-lane
group's ds_write_b32 meets each LDS bank at most twice."""
import collections

import pytest

import f32w_quad_map as M

LENGTHS = (64, 192, 196, 4096, 16000)
THREADS = [M.thread(w, l) for w in range(4) for l in range(64)]


def test_threads_cover_the_chunk_once():
    assert sorted(THREADS) == [(c, q) for c in range(32) for q in range(8)]


def test_image_written_exactly_once():
    seen = collections.Counter(M.write_address(comp, xc, xq, i) for xc, xq in THREADS for comp in range(4) for i in range(4))
    want = {comp * M.XCOMP + col * M.XS + k for comp in range(4) for col in range(M.NP) for k in range(M.KCW)}
    assert set(seen) == want and set(seen.values()) == {1}


def test_bank_ways():
    for wave in range(4):
        for half in range(2):
            for comp in range(4):
                for i in range(4):
                    banks = collections.Counter(M.write_address(comp, *M.thread(wave, 32 * half + l), i) % 32 for l in range(32))
                    assert max(banks.values()) <= 2, (wave, half, comp, i, banks)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("logd", range(12))
def test_pieces(L, logd):
    assert L % 4 == 0
    np_ = M.pair_count(L, logd)
    assert np_ % 4 == 0 or logd < 2                               # (d = 1, 2 with L % 8 != 0: a last quad with pairs past the count, staged as before)
    for p0 in range(0, np_, M.NP):
        for xq in range(8):
            pieces = [M.piece(p0, xq, k, L, logd) for k in range(4)]
            for tp, inside in pieces:
                assert tp % 4 == 0
                assert inside == all(0 <= tp + i < L for i in range(4)) == any(0 <= tp + i < L for i in range(4))
                for xc in (0, 31):
                    off = M.byte_offset(xc, p0, xq, pieces.index((tp, inside)), L, logd)
                    assert off == M.OUTSIDE if not inside else (off % 16 == 0 and xc * L * 4 <= off and off + 16 <= (xc + 1) * L * 4)
            for i in range(4):                                    # tap k of pair 4 xq + i, as the 4-byte staging takes it
                for k in range(4):
                    pc, el = M.source(i, k, logd)
                    tp, inside = pieces[pc]
                    assert M.old_tap(p0, 4 * xq + i, k, L, logd) == (tp + el if inside else None)
