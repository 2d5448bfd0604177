"""Host and index arithmetic of ap_wgrad_corr (ap_wgrad.hip) restated in plain Python, the float64 reference of its contraction,
and the case table of test_gpu_wgrad_edges.py.  Every row of the table names the branches of wgrad_corr_kernel it exists to
reach; test_wgrad_restate_cpu.py asserts from the restated plan that it really reaches them, so a later retuning of the chunk,
the tile or the slice target cannot quietly turn an edge case into a plain one.  Test infrastructure only."""
import collections
import functools

import numpy as np
import torch

from audiopure_amd import synth

PLAIN, FILM, GATE = 0, 1, 2

# ap_wgrad.hip
WG_KC = 32                      # samples per staged chunk
WG_BM, WG_BN = 128, 64          # tile of G per workgroup
WG_QW = WG_KC + 4               # samples per staged Q window
WG_TARGET = 512                 # workgroups wgrad_slices aims at
DIL_LIMIT = lambda L: (0x7FFFFFFF - L - 64) // 2          # the largest dil ap_wgrad_corr's range check lets through

Plan = collections.namedtuple("Plan", "tiles cpc nchunk slices runs")


def plan(B, M, N, L):
    """wgrad_slices and the kernel's split of the chunks: tiles of G, chunks per clip, chunks in all, slices, and each slice's run
    [c0, c1) of chunks (chunk c is clip c // cpc, samples [32 (c % cpc), 32 (c % cpc) + 32) of it)."""
    tiles = -(-M // WG_BM) * -(-N // WG_BN)
    cpc = -(-L // WG_KC)
    nchunk = B * cpc
    slices = min(max(-(-WG_TARGET // tiles), 1), nchunk)
    runs = [(z * nchunk // slices, (z + 1) * nchunk // slices) for z in range(slices)]
    return Plan(tiles, cpc, nchunk, slices, runs)


def workspace_bytes(B, M, N, L, taps):
    return plan(B, M, N, L).slices * M * N * taps * 4


def tap_windows(taps, dil, L):
    """(off, al, sh, on) per tap: the tap's offset, the 16-byte-aligned start of its staged window relative to the chunk, the
    remainder the fragment read adds, and whether any sample of a clip meets it.  (One tap runs at dil = 1, as the launcher has it.)"""
    dil = 1 if taps == 1 else dil
    out = []
    for k in range(taps):
        off = (k - taps // 2) * dil
        al = off & ~3                                             # floor to a multiple of 4, for negative offsets too
        out.append((off, al, off - al, -L < off < L))
    return out


def uses_vec(L, p_addr, q_addr):
    """Whether the launcher takes the 16-byte loads: every row of P and Q must start on a 16-byte boundary."""
    return L % 4 == 0 and p_addr % 16 == 0 and q_addr % 16 == 0


def corr_reference(P, Q, film, taps, dil, mode):
    """G[m][n][k] = sum_{b,t} P[b][m][t] Q~[b][n][t + (k - taps/2) dil] in float64; Q~ zero outside [0, L)."""
    P, Q = P.double(), Q.double()
    B, M, L = P.shape
    if mode == FILM:
        Q = Q + film.double().view(1, -1, 1)
    elif mode == GATE:
        Nn = Q.shape[1] // 2
        Q = torch.tanh(Q[:, :Nn]) * torch.sigmoid(Q[:, Nn:])
    G = torch.zeros(M, Q.shape[1], taps, dtype=torch.float64)
    for k in range(taps):
        off = (k - taps // 2) * dil
        lo, hi = max(0, -off), min(L, L - off)                    # t with 0 <= t + off < L
        if lo < hi:
            G[:, :, k] = torch.einsum("bmt,bnt->mn", P[:, :, lo:hi], Q[:, :, lo + off:hi + off])
    return G


def abs_terms(P, Q, film, taps, dil, mode):
    """sum |terms| of every output element: the reference of |P| and |Q~| (FiLM added before the absolute value)."""
    Qa = (Q.double() + film.double().view(1, -1, 1)).abs() if mode == FILM else Q.double().abs()
    return corr_reference(P.abs(), Qa, None, taps, dil, PLAIN)


# ---- the tags ------------------------------------------------------------------------------------------------------------------
PLAN_TAGS = ("deep", "straddle", "scalar", "m_half", "n_half", "one_chunk")
TAP_TAGS = ("sh1", "sh2", "sh3", "neg", "off_tap")


def plan_tags(B, M, N, L):
    p = plan(B, M, N, L)
    tags = set()
    if any(c1 - c0 >= 3 for c0, c1 in p.runs):
        tags.add("deep")
    # a clip's partial last chunk followed, inside one slice, by chunk 0 of the next clip
    if L % WG_KC and any(c % p.cpc == p.cpc - 1 and c + 1 < c1 for c0, c1 in p.runs for c in range(c0, c1)):
        tags.add("straddle")
    if L % 4:
        tags.add("scalar")
    if M % 64 == 32:                                              # a wave's rows [64 wm, 64 wm + 64): the i = 1 half is absent
        tags.add("m_half")
    if N % WG_BN == 32:                                           # the last column tile is half empty
        tags.add("n_half")
    if p.nchunk == 1:
        tags.add("one_chunk")
    return tags


def tap_tags(taps, dil, L):
    tags = set()
    for off, al, sh, on in tap_windows(taps, dil, L):
        if not on:
            tags.add("off_tap")
            continue
        if sh:
            tags.add(f"sh{sh}")
        if al < 0:
            tags.add("neg")
    return tags


def straddling_slices(B, M, N, L):
    p = plan(B, M, N, L)
    return [z for z, (c0, c1) in enumerate(p.runs) if L % WG_KC and any(c % p.cpc == p.cpc - 1 and c + 1 < c1 for c in range(c0, c1))]


# ---- the case table ------------------------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "name B M N L taps dils tags")

_WIDE = lambda L: (1, 2, 3, 5, 33, 1024, L - 1, L, 2048)          # L - 1: one live sample per outer tap; L and 2048: none
_ALL_TAPS = {"sh1", "sh2", "sh3", "neg", "off_tap"}

# exact comparison on integer data, PLAIN and FILM (test 2a)
EXACT_ROWS = [
    Row("deep_vec", 3, 512, 256, 1100, 3, _WIDE(1100), {"deep", "straddle"} | _ALL_TAPS),
    Row("deep_scalar", 3, 512, 256, 1102, 3, _WIDE(1102), {"deep", "straddle", "scalar"} | _ALL_TAPS),
    Row("clip_per_chunk", 100, 512, 256, 20, 3, _WIDE(20), {"deep", "straddle"} | _ALL_TAPS),
    Row("dil_sweep", 3, 128, 64, 300, 3, tuple(range(1, 10)), {"sh1", "sh2", "sh3", "neg"}),
    Row("m96_n96", 2, 96, 96, 200, 3, (1, 2, 7), {"m_half", "n_half", "sh1", "sh2", "sh3", "neg"}),
    Row("m160_n32", 2, 160, 32, 203, 3, (1, 2, 7), {"m_half", "n_half", "scalar", "sh1", "sh2", "sh3", "neg"}),
    Row("one_chunk_32", 1, 32, 32, 32, 3, (1, 5, 31, 32), {"one_chunk", "m_half", "n_half", "sh1", "sh3", "neg", "off_tap"}),
    Row("one_chunk_3", 1, 32, 32, 3, 3, (1, 2, 3, 4), {"one_chunk", "scalar", "m_half", "n_half", "sh1", "sh2", "sh3", "neg", "off_tap"}),
    Row("one_tap", 2, 96, 96, 200, 1, (1,), {"m_half", "n_half"}),
]
EXACT_CASES = [(r.name, dil) for r in EXACT_ROWS for dil in r.dils]

# GATE against float64 (test 2b)
GATE_ROWS = [
    Row("gate_vec", 5, 256, 256, 1252, 1, (1,), {"deep", "straddle"}),
    Row("gate_scalar", 5, 256, 256, 1251, 1, (1,), {"deep", "straddle", "scalar"}),
    Row("gate_three_taps", 2, 96, 96, 200, 3, (3,), {"m_half", "n_half", "sh1", "sh3", "neg"}),
]
ALL_ROWS = EXACT_ROWS + GATE_ROWS
ROWS = {r.name: r for r in ALL_ROWS}

# the plans the issue behind these tests recorded: (B, M, N, L) -> (slices, deepest run, straddling slices)
RECORDED_PLANS = {(3, 512, 256, 1100): (32, 4, 2), (3, 512, 256, 1102): (32, 4, 2), (5, 256, 256, 1252): (64, 4, 3),
                  (5, 256, 256, 1251): (64, 4, 3), (100, 512, 256, 20): (32, 4, 32), (2, 96, 96, 200): (14, 1, 0),
                  (2, 160, 32, 203): (14, 1, 0), (1, 32, 32, 32): (1, 1, 0), (1, 32, 32, 3): (1, 1, 0), (3, 128, 64, 300): (30, 1, 0)}


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _ints(key, shape, values):
    """int-valued float32 tensor drawn uniformly from `values`, determined by (key, shape) alone"""
    idx = np.floor(synth.uniform(key, shape, 3, 0.0, float(len(values)))).astype(np.int64)
    return torch.from_numpy(np.asarray(values, dtype=np.float32)[np.clip(idx, 0, len(values) - 1)])


@functools.lru_cache(maxsize=None)
def integer_inputs(name):
    """(P, Q, film, prior) of an exact row: P and Q in {-3..3} \\ {0}, film in {4, 5, 6} (Q + film lies in 1..9: no sample of Q~ is 0,
    so a sample read from the wrong place or dropped always moves an integer), an integer prior for accumulate = 1."""
    r = ROWS[name]
    nz = (-3, -2, -1, 1, 2, 3)
    return (_ints(f"wgi.{name}.P", (r.B, r.M, r.L), nz), _ints(f"wgi.{name}.Q", (r.B, r.N, r.L), nz),
            _ints(f"wgi.{name}.f", (r.N,), (4, 5, 6)), _ints(f"wgi.{name}.G0", (r.M, r.N, r.taps), tuple(range(-50, 51))))


GATE_PLANTS_TANH = (15.0, -15.0, 16.0, -16.0, 40.0, -40.0)
GATE_PLANTS_SIGMOID = (80.0, -80.0, 100.0, -100.0)


@functools.lru_cache(maxsize=None)
def gate_inputs(name):
    """(P, Q) of a GATE row: P uniform in [-1, 1), the pre-activations Q [B][2N][L] uniform in [-2, 2) with saturating values planted
    in both halves -- at the first and the last sample of a clip among others, where the windows of the outer taps end."""
    r = ROWS[name]
    P = torch.from_numpy(synth.uniform(f"wgg.{name}.P", (r.B, r.M, r.L), 3))
    Q = torch.from_numpy(synth.uniform(f"wgg.{name}.Q", (r.B, 2 * r.N, r.L), 3, -2.0, 2.0)).clone()
    spots = [0, r.L - 1, r.L // 2, 31, 32, 33]
    for i, v in enumerate(GATE_PLANTS_TANH):
        Q[i % r.B, (7 * i) % r.N, spots[i % len(spots)]] = v
        Q[(i + 1) % r.B, r.N - 1 - i, spots[(i + 2) % len(spots)]] = v
    for i, v in enumerate(GATE_PLANTS_SIGMOID):
        Q[i % r.B, r.N + (5 * i) % r.N, spots[i % len(spots)]] = v
        Q[(i + 1) % r.B, 2 * r.N - 1 - i, spots[(i + 3) % len(spots)]] = v
    return P, Q
