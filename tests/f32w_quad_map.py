"""The lane map of the F(2,3) fp32 block's quad staging (DIET_QUAD_ of audiopure_amd/csrc/ap_resblock_f32w.hip), restated in Python
for tests/test_f32w_quad_map_cpu.py.  A workgroup is four waves of 64 lanes; a tile is 32 pairs, a chunk 32 channels."""

NP, KCW = 32, 32                  # pairs per tile, channels per chunk
XS = KCW + 4                      # floats per (product, column) row of the X image
XCOMP = NP * XS                   # one product's image
OUTSIDE = 0x80000000              # the byte offset of a piece outside the clip: no descriptor reaches it, the load answers +0


def dilation_class(logd):
    """The kernel's DCLS template argument: 1 (d = 1), 2 (d = 2), 4 (d >= 4)."""
    return min(1 << logd, 4)


def first_output(p, logd):
    d = 1 << logd
    return ((p >> logd) << (logd + 1)) + (p & (d - 1))


def pair_count(L, logd):
    d = 1 << logd
    return (L // (2 * d)) * d + min(L % (2 * d), d)


def thread(wave, lane):
    """(channel of the chunk, quad of the tile) of a thread: a wave is 16 channels x 4 quads, the quad the fast lane index (four
    neighbouring lanes load 64 consecutive bytes)."""
    return 16 * (wave & 1) + (lane >> 2), 4 * (wave >> 1) + (lane & 3)


def piece(p0, xq, k, L, logd):
    """First sample of the thread's k-th 16-byte piece, and whether the kernel loads it.  d >= 4: the piece holds tap k of pairs
    p0 + 4 xq .. + 3; d = 1, 2: the four pieces are the window [tf - 4, tf + 12) of the quad's first output tf."""
    tp = first_output(p0 + 4 * xq, logd) + (k - 1) * max(1 << logd, 4)
    return tp, 0 <= tp < L


def source(i, k, logd):
    """(piece, element) that feeds tap k of pair i of the quad: the fixed table of each dilation class."""
    cls = dilation_class(logd)
    if cls == 4:
        return k, i
    w = 2 * (1 + 2 * (i >> 1) + k) + (i & 1) if cls == 2 else 2 * i + k + 3      # sample of the window
    return w >> 2, w & 3


def byte_offset(xc, p0, xq, k, L, logd):
    tp, inside = piece(p0, xq, k, L, logd)
    return (xc * L + tp) * 4 if inside else OUTSIDE


def write_address(comp, xc, xq, i):
    """Float index in a chunk image of product comp, pair i of the quad (one ds_write_b32)."""
    return comp * XCOMP + (4 * xq + i) * XS + xc


def old_tap(p0, j, k, L, logd):
    """The sample the 4-byte staging takes for tap k of pair p0 + j, or None outside the clip."""
    tp = first_output(p0 + j, logd) + (k - 1) * (1 << logd)
    return tp if 0 <= tp < L else None
