"""CPU side of test_gpu_wgrad_edges.py: every row of wgrad_restate.py's case table reaches the branches of wgrad_corr_kernel it is
tagged with, the restated slicing agrees with the library's own host arithmetic, every tap window stays inside what the kernel
stages, and the integer rows satisfy the precondition of an exact comparison -- all on the restatement and the float64
reference alone, so that a GPU run is never the first place one of these fails."""
import numpy as np
import pytest
import torch

import wgrad_restate as R
from audiopure_amd import _native as N


@pytest.mark.parametrize("row", R.ALL_ROWS, ids=lambda r: r.name)
def test_every_row_reaches_the_branches_it_is_tagged_with(row):
    """Equality, not inclusion: a row also may not reach a branch it does not name."""
    got = R.plan_tags(row.B, row.M, row.N, row.L)
    for dil in row.dils:
        got |= R.tap_tags(row.taps, dil, row.L)
    assert got == set(row.tags), (row.name, got ^ set(row.tags))
    assert set(row.tags) <= set(R.PLAN_TAGS) | set(R.TAP_TAGS)


def test_the_table_reaches_every_tag_on_both_load_paths():
    tags = lambda rows, vec: set().union(*(r.tags for r in rows if ("scalar" in r.tags) != vec))
    assert tags(R.EXACT_ROWS, True) >= set(R.PLAN_TAGS + R.TAP_TAGS) - {"scalar"}
    assert tags(R.EXACT_ROWS, False) >= set(R.PLAN_TAGS + R.TAP_TAGS)
    for vec in (True, False):
        assert tags(R.GATE_ROWS, vec) >= {"deep", "straddle"}
    assert len({r.name for r in R.ALL_ROWS}) == len(R.ALL_ROWS)
    # the exact rows, as asked for: the wide dilation set on the three 512 x 256 rows, 1..9 on the cheap one, 1..4 at L = 3
    for name in ("deep_vec", "deep_scalar", "clip_per_chunk"):
        r = R.ROWS[name]
        assert (r.M, r.N, r.taps) == (512, 256, 3) and set(r.dils) == {1, 2, 3, 5, 33, 1024, r.L - 1, r.L, 2048}
    assert R.ROWS["dil_sweep"].dils == tuple(range(1, 10)) and R.ROWS["one_chunk_3"].dils == (1, 2, 3, 4)


def test_plans_are_the_recorded_ones():
    for (B, M, Nn, L), (slices, deepest, straddling) in R.RECORDED_PLANS.items():
        p = R.plan(B, M, Nn, L)
        assert (p.slices, max(c1 - c0 for c0, c1 in p.runs), len(R.straddling_slices(B, M, Nn, L))) == (slices, deepest, straddling), (B, M, Nn, L)
    assert {(r.B, r.M, r.N, r.L) for r in R.ALL_ROWS} == set(R.RECORDED_PLANS)
    p = R.plan(3, 512, 256, 1100)
    assert p.cpc == 35 and p.runs[10] == (32, 36) and p.runs[21] == (68, 72) and R.straddling_slices(3, 512, 256, 1100) == [10, 21]
    assert all(c1 - c0 in (3, 4) for c0, c1 in R.plan(100, 512, 256, 20).runs) and R.plan(100, 512, 256, 20).cpc == 1
    # the workload itself: about 60 chunks of each clip per slice, walking across clips
    p = R.plan(8, 256, 256, 16000)
    assert p.slices == 64 and min(c1 - c0 for c0, c1 in p.runs) >= 62
    # what the suite ran before: never more than two chunks in a slice
    for B, M, Nn, L in [(1, 64, 32, 37), (2, 512, 256, 640), (2, 32, 32, 129), (2, 512, 256, 300), (3, 256, 256, 777), (2, 256, 256, 640)]:
        assert "deep" not in R.plan_tags(B, M, Nn, L) and "straddle" not in R.plan_tags(B, M, Nn, L)


def test_runs_partition_the_chunks():
    rng = np.random.RandomState(7)
    shapes = [(r.B, r.M, r.N, r.L) for r in R.ALL_ROWS] + [(int(rng.randint(1, 9)), 32 * int(rng.randint(1, 20)), 32 * int(rng.randint(1, 12)),
                                                            int(rng.randint(1, 3000))) for _ in range(300)]
    for B, M, Nn, L in shapes:
        p = R.plan(B, M, Nn, L)
        assert 1 <= p.slices <= p.nchunk and p.runs[0][0] == 0 and p.runs[-1][1] == p.nchunk
        assert all(a[1] == b[0] for a, b in zip(p.runs, p.runs[1:])) and all(c0 < c1 for c0, c1 in p.runs)   # no empty slice


def test_workspace_bytes_agree_with_the_library():
    """ap_wgrad_workspace_bytes is host-only: the restated slicing is the library's, for every row and 400 random shapes."""
    lib = N.lib()
    rng = np.random.RandomState(11)
    shapes = [(r.B, r.M, r.N, r.L, r.taps) for r in R.ALL_ROWS]
    shapes += [(int(rng.randint(1, 130)), 32 * int(rng.randint(1, 24)), 32 * int(rng.randint(1, 24)), int(rng.randint(1, 20000)),
                int(rng.choice([1, 3]))) for _ in range(400)]
    for B, M, Nn, L, taps in shapes:
        p = R.plan(B, M, Nn, L)
        assert p.slices * M * Nn * taps * 4 == R.workspace_bytes(B, M, Nn, L, taps) == lib.ap_wgrad_workspace_bytes(B, M, Nn, L, taps), (B, M, Nn, L)
    assert lib.ap_wgrad_workspace_bytes(1, 32, 32, 40, 2) == 0 and lib.ap_wgrad_workspace_bytes(0, 32, 32, 40, 3) == 0


def test_tap_windows_stay_inside_the_staged_window():
    used = {(r.taps, dil, r.L) for r in R.ALL_ROWS for dil in r.dils} | {(3, d, 16000) for d in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048)}
    used |= {(3, R.DIL_LIMIT(1100), 1100)}
    for taps, dil, L in used:
        w = R.tap_windows(taps, dil, L)
        assert len(w) == taps and w[taps // 2] == (0, 0, 0, True)
        for off, al, sh, on in w:
            assert al % 4 == 0 and 0 <= sh <= 3 and al + sh == off
            assert sh + R.WG_KC <= R.WG_QW == 36                  # the fragment read [sh, sh + 32) of a 36-sample window
            assert on == any(0 <= t + off < L for t in (0, L - 1))
            assert -2 ** 31 <= al and (L + 31) // 32 * 32 + al + R.WG_QW < 2 ** 31
    assert [w[1:3] for w in R.tap_windows(3, 1, 100)] == [(-4, 3), (0, 0), (0, 1)]
    assert R.tap_windows(3, 5, 100)[0] == (-5, -8, 3, True) and R.tap_windows(3, 5, 100)[2] == (5, 4, 1, True)
    assert R.tap_windows(3, 100, 100)[0][3] is False and R.tap_windows(3, 99, 100)[0][3] is True
    assert R.tap_windows(1, 77, 100) == [(0, 0, 0, True)]         # one tap: the dilation does not enter
    assert R.DIL_LIMIT(1100) * 2 + 1100 + 64 <= 0x7FFFFFFF < (R.DIL_LIMIT(1100) + 1) * 2 + 1100 + 64


def test_uses_vec():
    assert R.uses_vec(1100, 4096, 8192) and not R.uses_vec(1102, 4096, 8192)
    assert not R.uses_vec(1100, 4100, 8192) and not R.uses_vec(1100, 4096, 8196) and R.uses_vec(20, 16, 32)


@pytest.mark.parametrize("name", [r.name for r in R.EXACT_ROWS])
def test_integer_rows_meet_the_precondition_of_an_exact_comparison(name):
    """Inputs are the integers promised, and sum |terms| of every output element stays below 2^24 (with the prior of the accumulate
    call added): every partial sum in any order is then an exactly representable integer, in fp32 as in float64."""
    r = R.ROWS[name]
    P, Q, film, prior = R.integer_inputs(name)
    assert P.dtype == Q.dtype == film.dtype == prior.dtype == torch.float32
    assert set(P.unique().tolist()) == set(Q.unique().tolist()) == {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0} or r.L < 8
    assert torch.count_nonzero(P).item() == P.numel() and torch.count_nonzero(Q).item() == Q.numel()
    assert set(film.unique().tolist()) <= {4.0, 5.0, 6.0}
    Qf = Q + film.view(1, -1, 1)
    assert float(Qf.min()) >= 1.0 and float(Qf.max()) <= 9.0
    assert torch.equal(prior, prior.round()) and float(prior.abs().max()) <= 50
    for dil in (r.dils[0], r.dils[-1]):                           # |terms| of the centre tap bound those of every window
        for mode in (R.PLAIN, R.FILM):
            worst = float(R.abs_terms(P, Q, film, r.taps, dil, mode).max()) + 50
            assert worst < 2 ** 24, (name, dil, worst)
    assert 3 * 9 * r.B * r.L + 50 < 2 ** 24                       # the same, from the value ranges alone: every dilation


def test_reference_is_the_direct_sum():
    """corr_reference against the triple loop it abbreviates, on a shape small enough to write out."""
    P, Q, film = (torch.from_numpy(R.synth.uniform(k, s, 3)) for k, s in (("rfP", (2, 3, 7)), ("rfQ", (2, 4, 7)), ("rff", (4,))))
    for dil in (1, 3, 6, 7):
        G = R.corr_reference(P, Q, film, 3, dil, R.FILM)
        want = torch.zeros(3, 4, 3, dtype=torch.float64)
        for k in range(3):
            for b in range(2):
                for t in range(7):
                    u = t + (k - 1) * dil
                    if 0 <= u < 7:
                        want[:, :, k] += P[b, :, t].double().view(3, 1) * (Q[b, :, u].double() + film.double()).view(1, 4)
        assert float((G - want).abs().max()) < 1e-12
    Qg = torch.cat([Q, Q.flip(1)], 1)
    G = R.corr_reference(P, Qg, None, 1, 1, R.GATE)
    want = torch.einsum("bmt,bnt->mn", P.double(), torch.tanh(Qg[:, :4].double()) * torch.sigmoid(Qg[:, 4:].double()))
    assert float((G[:, :, 0] - want).abs().max()) < 1e-12


def test_gate_inputs_hold_the_planted_values():
    for r in R.GATE_ROWS:
        P, Q = R.gate_inputs(r.name)
        assert Q.shape == (r.B, 2 * r.N, r.L)
        assert all(bool((Q[:, :r.N] == v).any()) for v in R.GATE_PLANTS_TANH)
        assert all(bool((Q[:, r.N:] == v).any()) for v in R.GATE_PLANTS_SIGMOID)
        assert float(Q[:, :r.N].abs().max()) == 40.0 and float(Q[:, r.N:].abs().max()) == 100.0
        assert bool((Q[:, :, 0].abs() >= 15).any()) and bool((Q[:, :, r.L - 1].abs() >= 15).any())   # at both ends of a clip
