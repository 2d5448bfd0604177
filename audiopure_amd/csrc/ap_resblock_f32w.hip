// AP_PREC_F32, shipped shape (res = skip = 256 channels): fused Residual_block.forward (WaveNet.py:75-97) with the dilated k = 3
// conv (WaveNet.py:87) in F(2,3) minimal-filtering form over the dilation pair.
//
// Outputs t and t + d of the conv share the taps u[t-d], u[t], u[t+d], u[t+2d] (u = h + part_t, zero outside the clip), so the
// pair is four [2C x C] products instead of six:
//     m1 = W0 (u0 - u2)    m2 = (W0+W1+W2)/2 (u1 + u2)    m3 = (W0-W1+W2)/2 (u2 - u1)    m4 = W2 (u3 - u1)
//     y[t] = (m1 + m2) + m3 + b        y[t+d] = (m2 - m3) + m4 + b
// GEMM1 is 8.39 GFLOP per clip instead of 12.58, the block 12.58 instead of 16.78 -- on the exact-fp32 matrix instruction
// (v_mfma_f32_32x32x2_f32), whose rate bounds this kernel.  Transformed weights are computed in double and rounded once at load;
// the oracle restates the same operation order (oracle/diffwave_oracle.py::winograd_dilated_conv) and holds the reference's
// golden vectors at the fp32 tolerances (tests/test_oracle_golden.py).
//
// Pairing: sample t is a pair's first output when floor(t / d) is even, its second otherwise; pair p has first output
// tf(p) = ((p >> log2 d) << (log2 d + 1)) + (p & (d - 1)).  A tile is 32 consecutive pairs = 64 outputs: for d < 32 one 64-sample
// window, for d >= 32 two 32-sample runs d apart.
//
// Machine shape: one persistent workgroup per CU, FOUR waves -- one per SIMD, each with the SIMD's whole register file: wave w
// owns the tanh and sigmoid rows of gate channels [64w, 64w + 64) = 128 GEMM1 rows x 32 pair columns x 4 products = 256
// accumulator registers; every LDS B fragment (one ds_read_b128 = four k-steps) feeds 16 MFMAs, every 16-byte weight fragment
// four.  Per chunk of 32 channels: 16 raw 4-byte loads per thread (4 taps x 4 channels of one pair), FiLM add, zero padding,
// the four input differences, four ds_write_b128 into a [product][column][k] image (144-byte rows: conflict-free 16-byte reads
// and writes) -- in the 16-byte forms four 16-byte loads per thread (one channel, four pairs: DIET_QUAD_ below); weights stream L2 -> registers through a ring one k-group (64 MFMAs) deep, requested after the unit that frees
// their registers so that no wait on them includes the HBM-latency activation loads issued at the chunk's top.
// Then: output transform + gate in registers -> g image [column][channel] (1040-byte rows) -> GEMM2 [(C + S) x C].[C x 64]
// (res rows and skip rows of the wave's 64 channels) -> h' = (h + part_t + res) sqrt(1/2), skip += by memory-side float atomics
// (one adder per element per launch: deterministic).
#include "ap_common.h"

#include <type_traits>

namespace ap {

namespace {

constexpr int WC_ = 256;                 // res = skip channels
constexpr int NP_ = BLOCK_NP;            // pairs per tile
constexpr int KCW_ = 32;                 // channels per staged chunk
constexpr int NCH_ = WC_ / KCW_;         // 8 chunks
constexpr int XS_ = KCW_ + 4;            // floats per (product, column) row of the X image
constexpr int XCOMP_ = NP_ * XS_;        // one product's image
constexpr int XBUF_ = 4 * XCOMP_;        // one chunk's image (18 KB)
constexpr int GS_ = WC_ + 4;             // floats per column row of the g image
constexpr int GOFF_ = 2 * XBUF_;
constexpr int POFF_ = GOFF_ + 64 * GS_;         // Q16: output patches, [wave 4][2][32 rows][36] floats (36.9 KB)
constexpr int PS_ = 36;
constexpr int LDS_FLOATS_ = GOFF_ + 64 * GS_;   // 103,424 B
constexpr int LDS_FLOATS_Q16_ = POFF_ + 4 * 2 * 32 * PS_;   // 140,288 B
constexpr int NCONST_ = 5 * WC_;           // b1 (2C) | b2 (2C) | part_t (C): the launch constants' LDS copy (5 KB)
// What the kernel leaves out that the result never needed (bits of the DIET template argument; tools builds instantiate each alone
// for tools/ab_f32w.py, the product both -- profiles/f32w_diet_ab.txt has the A/B.  A third item, a four-deep X ring with one
// barrier per chunk pair, measured null there and is not in this source):
constexpr int DIET_CARRY_ = 2;           // the last k-group's wrapped weight loads ARE the next tile's first units; no X request past chunk 7
constexpr int DIET_CONST_ = 4;           // b1, b2, part_t copied to LDS once per launch: the accumulator inits read LDS, not memory
// What runs under MFMAs that used to run between them (one more bit, the same A/B: profiles/f32w_edges_ab.txt).  The split is by ROW
// tiles, so every accumulator keeps its own MFMA sequence and none lives longer than before.  (Bit 8, the last chunk by rows with
// half of the gate in its second pass, measured slower there and is not in this source: v_mfma_f32_32x32x2_f32 hides LDS and
// memory instructions but no VALU work -- profiles/f32w_edges_gap_budget.txt.)
constexpr int DIET_ROWS_ = 16;           // GEMM2: the res rows, then the skip rows with the h' epilogue in their gaps
// Fewer vector-ALU issue slots (beside v_mfma_f32_32x32x2_f32 every one is paid in full; the A/B: profiles/f32w_pk_ab.txt):
constexpr int DIET_PK_ = 32;             // 16-byte forms: output transform and gate on register pairs (v_pk_add/mul/fma_f32: the matrix pipe is idle there)
// (Bit 64, staging with out-of-clip taps loaded as +0 and u = fma(pt, 1 or 0, x) in place of add + select, gained 0.23 .. 0.45 % but
// stayed inside mask 22's min-max band in one of the six cells and is not in this source: docs/HISTORY.md.)
constexpr int DIET_ZERO_ = 128;          // m1, m3, m4 are not zeroed: chunk 0, peeled, starts them from the instruction's constant 0
// (with chunk 0 peeled the allocator also stops giving three product tiles other registers in the last chunk than in the chunk loop,
// which mask 22 pays per tile with 32 v_accvgpr_mov, 80 reads and 80 writes in the last chunk's MFMA gaps: docs/HISTORY.md I.13)
// MFMAs through the chunk turn (the 16-byte forms; the A/B: profiles/f32w_seam_ab.txt, the budget: profiles/f32w_seam_gap_budget.txt):
constexpr int DIET_SEAM_ = 1024;         // the chunk's barrier in its last unit, the next chunk's first fragment behind it; X requested in unit 13's gaps
// (Bit 512, every B fragment pinned a unit ahead of its use, measured 0.04 .. 0.24 % slower in all six cells -- a read one MFMA ahead
// is already free -- and bit 2048, the staging on channel pairs as 8 v_pk_fma_f32 + 8 v_pk_add_f32 without selects, gained 0.01 ..
// 0.20 % and stayed inside mask 182's band; neither is in this source: docs/HISTORY.md I.14.)
// Fewer and wider memory instructions in the main loop (the 16-byte forms; the A/B: profiles/f32w_quad_ab.txt):
constexpr int DIET_QUAD_ = 4096;         // X staged by (channel, quad of four pairs): four 16-byte loads per chunk in place of sixteen 4-byte ones and part_t's
// (Bit 8192, a unit's MFMAs by row tile with one weight load behind every fourth, was slower than mask 1206 in three of eight cells --
// the budget had priced the four loads behind the 16th MFMA at 0.7 cycles a unit -- and is not in this source: docs/HISTORY.md I.15.)
#ifndef AP_F32W_DIET
#define AP_F32W_DIET 5302
#endif
// the 4-byte epilogue form (ragged clip lengths) holds 64 residual values across GEMM2 and has no registers to spare: no item
constexpr int DIET4_ = 0;
constexpr unsigned UNIT_BYTES_ = 4 * 64 * 16;   // one (k-group, product) unit of a wave's GEMM1 image: 4 row tiles x 64 lanes x 16 B
constexpr unsigned W1W_WAVE_BYTES_ = NCH_ * 4 * 4 * UNIT_BYTES_;   // 512 KB per wave and layer
constexpr unsigned W2W_WAVE_BYTES_ = (WC_ / 8) * UNIT_BYTES_;      // 128 KB per wave and layer

}  // namespace

// GEMM1 image: [wave 4][chunk 8][k-group 4][product 4][row tile 4][lane 64][4]; lane (i, hh), element e = k-step e of the group:
// channel 32 chunk + 8 kg + 4 hh + e (the k a lane's ds_read_b128 B fragment holds for that step); row tiles interleave the tanh
// (even) and sigmoid (odd) halves as in pack_w1_kernel.
__global__ void pack_w1w_kernel(const float *__restrict__ w1f, float *__restrict__ out) {
  constexpr int C = WC_;
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 4u * NCH_ * 4 * 4 * 4 * 64 * 4) return;
  const int e = idx & 3, lane = (idx >> 2) & 63, rt = (idx >> 8) & 3, comp = (idx >> 10) & 3, kg = (idx >> 12) & 3,
            ch = (idx >> 14) & 7, w = idx >> 17;
  const int i = lane & 31, hh = lane >> 5;
  const int c = 32 * ch + 8 * kg + 4 * hh + e;
  const int o = (rt & 1) * C + 64 * w + 32 * (rt >> 1) + i;
  const float *p = w1f + ((size_t)o * C + c) * 3;
  const double w0 = p[0], w1 = p[1], w2 = p[2];
  const double v = comp == 0 ? w0 : comp == 1 ? (w0 + w1 + w2) * 0.5 : comp == 2 ? (w0 - w1 + w2) * 0.5 : w2;
  out[idx] = (float)v;
}

// GEMM2 image: [wave 4][k-group 32][row tile 4][lane 64][4]; channel 8 kg + 4 hh + e; row tiles 0,1 = res_conv rows of the wave's
// 64 channels, 2,3 = skip_conv rows of the same channels (w2f = [res rows; skip rows]).
__global__ void pack_w2w_kernel(const float *__restrict__ w2f, float *__restrict__ out) {
  constexpr int C = WC_;
  const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 4u * (C / 8) * 4 * 64 * 4) return;
  const int e = idx & 3, lane = (idx >> 2) & 63, rt = (idx >> 8) & 3, kg = (idx >> 10) & 31, w = idx >> 15;
  const int i = lane & 31, hh = lane >> 5;
  const int c = 8 * kg + 4 * hh + e;
  const int o = (rt >> 1) * C + 64 * w + 32 * (rt & 1) + i;
  out[idx] = w2f[(size_t)o * C + c];
}

int launch_pack_f32w(ap_ctx *ctx, hipStream_t st) {
  const int C = ctx->C, S = ctx->S;
  const size_t n1f = (size_t)2 * C * C * 3, n2 = (size_t)(C + S) * C, n1w = (size_t)4 * 2 * C * C;
  for (int n = 0; n < ctx->NL; n++) {
    pack_w1w_kernel<<<(unsigned)((n1w + 255) / 256), 256, 0, st>>>(ctx->w1f + n * n1f, ctx->w1w + n * n1w);
    pack_w2w_kernel<<<(unsigned)((n2 + 255) / 256), 256, 0, st>>>(ctx->w2f + n * n2, ctx->w2w + n * n2);
  }
  AP_HIP(hipGetLastError());
  return 0;
}

// SAVE (the differentiable path's forward pass, ap_resblock_fwd_save): the pre-gate activations y = DilConv(u) + b are also written
// to aout [B][2C][L] (rows 0..C-1 the tanh half, C..2C-1 the sigmoid half: what ap_resblock_bwd reads).
// Q16 (clip lengths that are multiples of four -- every shipped shape): the epilogue goes through wave-private LDS patches so that
// each 32 x 32 accumulator tile leaves as 1 row x 4 samples per lane -- 16-byte stores, the residual's h patch and the running skip
// rows as 16-byte loads (skip += as a read-modify-write: one workgroup owns a tile within a launch, launches are stream-ordered,
// so the sum is as deterministic as the float atomics of the 4-byte form).  A CU's store path moves a 4-byte-per-lane store
// stream at a fraction of its 16-byte rate: the 4-byte epilogue cost 6.5 % of the launch (tools/ab_f32w.py).
// DCLS (DIET_QUAD_ only): the dilation class of the quad staging -- 1: d = 1, 2: d = 2, 4: d >= 4 -- a template argument so that no
// chunk body branches on the dilation.
template <bool NOH, bool SAVE = false, bool Q16 = false, int DIET = AP_F32W_DIET, int DCLS = 4>
__global__ __launch_bounds__(256, 1) void resblock_f32w_kernel(
    const float *__restrict__ hin, const float *__restrict__ pt, float *__restrict__ hout, float *__restrict__ skip,
    const float *__restrict__ w1w, const float *__restrict__ b1, const float *__restrict__ w2w,
    const float *__restrict__ b2, int L, int logd, int accumulate, int ntiles, int nblk, float *__restrict__ aout) {
  constexpr int C = WC_;
  constexpr bool CARRY = (DIET & DIET_CARRY_) != 0, CONST = (DIET & DIET_CONST_) != 0;
  constexpr bool ROWS = Q16 && !NOH && (DIET & DIET_ROWS_) != 0;                        // every 16-byte form that writes h'
  constexpr bool PK = Q16 && (DIET & DIET_PK_) != 0;
  constexpr bool ZERO = Q16 && (DIET & DIET_ZERO_) != 0;
  constexpr bool SEAM = Q16 && (DIET & DIET_SEAM_) != 0;
  constexpr bool QUAD = Q16 && (DIET & DIET_QUAD_) != 0;
  static_assert(!SEAM || (CARRY && ZERO), "DIET_SEAM_ is written for the peeled first and last chunk");
  static_assert(!QUAD || (SEAM && CONST), "DIET_QUAD_ takes part_t from the LDS copy and its place in the chunk from DIET_SEAM_");
  // LDS map (floats): X sub-buffers 0, 1 | g image | Q16: output patches | CONST: b1, b2, part_t
  constexpr int COFF_ = Q16 ? LDS_FLOATS_Q16_ : LDS_FLOATS_;
  __shared__ __attribute__((aligned(16))) float lds[COFF_ + (CONST ? NCONST_ : 0)];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, hh = lane >> 5;
  const int sq = tid >> 5;                                       // staging: channel quad of the chunk (0..7); j = the pair
  // QUAD staging: channel xc of the chunk's 32, pairs 4 xq .. 4 xq + 3 of the tile's 32.  A wave is 16 channels x 4 quads with the
  // quad as the fast lane index: four neighbouring lanes load 64 consecutive bytes, which a 16-byte load per MFMA gap needs to be free
  // (with the channel fast it costs 256 cycles: profiles/f32w_quad_gap_budget.txt); a ds_write_b32 of one (product, pair of the quad)
  // goes to bank (16 quad + channel + const) mod 32 -- two lanes per bank in a 32-lane group, which costs this write nothing
  const int xc = 16 * (wave & 1) + (lane >> 2), xq = 4 * (wave >> 1) + (lane & 3);
  const int d = 1 << logd;

  // ---- tile walk: each XCD (workgroups g, g + 8, ... share one) takes a contiguous run of (clip, tile) work, its CUs walking
  // it side by side, so neighbouring tiles -- which share half their taps -- meet in one L2.  Placement only.
  int t_first, t_step, t_end;
  {
    const int g = blockIdx.x, G = gridDim.x;
    if (G >= 8 && (G & 7) == 0) {
      const int xcd = g & 7, idx = g >> 3, q = nblk >> 3, r = nblk & 7;
      const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
      t_first = base + idx;
      t_step = G >> 3;
      t_end = base + q + (xcd < r ? 1 : 0);
    } else {
      t_first = g;
      t_step = G;
      t_end = nblk;
    }
  }
  if (t_first >= t_end) return;
  if constexpr (CONST) {                                         // (a whole workgroup leaves above or none does: the barrier is uniform)
    for (int i = tid; i < NCONST_; i += 256) lds[COFF_ + i] = i < 2 * C ? b1[i] : i < 4 * C ? b2[i - 2 * C] : pt[i - 4 * C];
    __syncthreads();
  }

  auto uni_rsrc = [&](const void *base, unsigned bytes) {
    const uint64_t hb = (uint64_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)hb);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(hb >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), 0, (int)bytes, 0x00020000);
  };
  const unsigned clip_bytes = (unsigned)C * (unsigned)L * 4u;
  const __amdgpu_buffer_rsrc_t w1rs = uni_rsrc(reinterpret_cast<const char *>(w1w) + (size_t)wave * W1W_WAVE_BYTES_, W1W_WAVE_BYTES_);
  const __amdgpu_buffer_rsrc_t w2rs = uni_rsrc(reinterpret_cast<const char *>(w2w) + (size_t)wave * W2W_WAVE_BYTES_, W2W_WAVE_BYTES_);
  const unsigned lane16 = (unsigned)lane * 16u;
  // biases and part_t through buffer loads as well: as plain pointer loads these loop-invariant per-lane values are hoisted out of the
  // persistent loop and spilled; laundered pointers lose their address space and become flat loads, which force vmcnt(0) waits
  const __amdgpu_buffer_rsrc_t b1rs = uni_rsrc(b1, 2u * C * 4u), b2rs = uni_rsrc(b2, 2u * C * 4u), ptrs = uni_rsrc(pt, C * 4u);
  auto ld4 = [&](const __amdgpu_buffer_rsrc_t &rs, int idx) {    // four consecutive floats at element idx (16-byte aligned)
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)idx * 4u, 0, 0));
  };
  // the launch constants for the accumulator inits.  CONST: from their LDS copy -- as buffer loads they queue behind the previous
  // tile's skip stores (vmcnt retires in order) at every tile's top and again before GEMM2
  // (ROWS: through one opaque per-lane base.  The copy lies past byte 65 535, the reach of a DS instruction's offset field, so
  // from the array's own address every read gets an address register of its own -- thirty of them, hoisted out of the tile loop)
  // (the index is what is opaque: an opaque pointer would lose its address space)
  int cbase = COFF_ + 64 * wave + 4 * hh;
  if constexpr (CONST && ROWS) asm volatile("" : "+v"(cbase));
  auto ld_c = [&](int idx) {
    if constexpr (ROWS) return *reinterpret_cast<const f32x4 *>(lds + cbase + (idx - 64 * wave - 4 * hh));
    else return *reinterpret_cast<const f32x4 *>(lds + COFF_ + idx);
  };
  auto ld_b1 = [&](int idx) { if constexpr (CONST) return ld_c(idx); else return ld4(b1rs, idx); };
  auto ld_b2 = [&](int idx) { if constexpr (CONST) return ld_c(2 * C + idx); else return ld4(b2rs, idx); };
  auto ld_pt = [&](int idx) { if constexpr (CONST) return ld_c(4 * C + idx); else return ld4(ptrs, idx); };
  int cptx = COFF_ + 4 * C + xc;                                 // QUAD: this thread's part_t of chunk 0 in the LDS copy (opaque, as cbase)
  if constexpr (QUAD) asm volatile("" : "+v"(cptx));

  auto load_a1 = [&](f32x4(&a)[4], unsigned unit) {             // one (k-group, product) unit of GEMM1 weights: 4 row tiles
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
      a[rt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w1rs, lane16 + rt * 1024u, unit * UNIT_BYTES_, 0));
  };
  auto load_a2 = [&](f32x4(&a)[4], unsigned kg) {
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
      a[rt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w2rs, lane16 + rt * 1024u, kg * UNIT_BYTES_, 0));
  };

  // g image column of a pair's first / second output: sample order inside the tile (d < 32: one 64-sample window; else two runs)
  const int col0 = d >= 32 ? j : (((j >> logd) << (logd + 1)) + (j & (d - 1)));
  const int col1 = d >= 32 ? 32 + j : col0 + d;

  // ---- per-tile state, set one tile ahead (the next tile's first loads are requested before this tile's epilogue)
  int b, p0;
  __amdgpu_buffer_rsrc_t hrs;
  unsigned voff[4];
  bool tok[4];
  auto set_tile = [&](int tile) {
    b = __builtin_amdgcn_readfirstlane(tile / ntiles);
    p0 = __builtin_amdgcn_readfirstlane((tile % ntiles) * NP_);
    hrs = uni_rsrc(hin + (size_t)b * C * L, clip_bytes);
    // staging geometry of this thread's pair.  QUAD (L % 4 == 0): of its four pairs.  d >= 4: their first outputs are tf .. tf + 3,
    // tf % 4 == 0, so tap k of the quad is the aligned 16-byte piece at tf + (k - 1) d; d = 1, 2: tf % 8 == 0 and all sixteen taps lie
    // in the four aligned pieces of [tf - 4, tf + 12).  Every piece is wholly inside the clip or wholly outside; an outside piece gets
    // the offset no descriptor reaches (the load answers +0) and never a clamped or wrapped address
    const int p = QUAD ? p0 + 4 * xq : p0 + j;
    const int tf = ((p >> logd) << (logd + 1)) + (p & (d - 1));
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int tp = tf + (k - 1) * (QUAD && DCLS < 4 ? 4 : d);
      tok[k] = (tp >= 0) && (tp < L);
      if constexpr (QUAD) voff[k] = tok[k] ? ((unsigned)tp + (unsigned)xc * (unsigned)L) * 4u : 0x80000000u;
      else voff[k] = ((unsigned)min(max(tp, 0), L - 1) + (unsigned)(4 * sq) * (unsigned)L) * 4u;
    }
  };
    float xr[4][4];                                              // [channel of the quad][tap]
    f32x4 ptq;
    f32x4 xv[4];                                                 // QUAD: the four pieces (d >= 4: [tap][pair of the quad])
    float ptc;
    f32x2 su[8], sc[8];                                          // QUAD: u = x + part_t on sample pairs; the products (live in unit 12 only)
    float ptm[4], sc0[4], sc3[4];
    auto issue_x = [&](int ch) {
      if constexpr (QUAD) {
#pragma unroll
        for (int k = 0; k < 4; k++)
          xv[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(hrs, voff[k], ch * KCW_ * L * 4, 0));
        ptc = lds[cptx + ch * KCW_];
        return;
      }
      ptq = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ptrs, (unsigned)(16 * sq), ch * KCW_ * 4, 0));
#pragma unroll
      for (int cc = 0; cc < 4; cc++)
#pragma unroll
        for (int k = 0; k < 4; k++)
          xr[cc][k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(hrs, voff[k], (ch * KCW_ + cc) * L * 4, 0));
    };
    // QUAD: the staging in sixteen steps, one per MFMA gap of unit 12 (all of them in a row at the tile top).  u = x + part_t is the
    // same add as below inside the clip; outside it x = +0 and the masked part_t is 0: 0 + 0 = +0 whatever part_t's sign.  Sample
    // pairs run as v_pk_add_f32, written as instructions: in an MFMA's shadow the compiler splits the ones it selects itself.  Step
    // 0: the four selects; 1..3: u (w = sample pair of the window: d >= 4 piece w / 2 = tap, else pairs 1..6 of [tf - 4, tf + 12));
    // 4..7: the products; 8..15: two ds_write_b32 each into the unchanged [product][column][k] image.
    //   d >= 4: pairs (2h, 2h + 1) have tap k in pair 2k + h;     d = 2: the same pairs have tap k in pair 1 + 2h + k;
    //   d = 1: pair i has its taps at samples 2i + 3 .. 2i + 6 of the window: m2, m3 from sample pair i + 2 alone, m1, m4 one-wide
    auto stage = [&](float *dst, int g) __attribute__((always_inline)) {
      auto pk_add = [](f32x2 x, f32x2 y) { f32x2 r; asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y)); return r; };
      auto pk_sub = [](f32x2 x, f32x2 y) { f32x2 r; asm volatile("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(x), "v"(y)); return r; };
      auto pk_bc = [](f32x2 x, float y) {                        // x + (y, y): the second operand's low half twice, its high half is not read
        f32x2 r;
        f32x2 y2 = __builtin_nondeterministic_value(r);
        y2[0] = y;
        asm volatile("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(r) : "v"(x), "v"(y2));
        return r;
      };
      auto pk_sumdiff = [](f32x2 x) {                             // (x0 + x1, x1 - x0)
        f32x2 r;
        asm volatile("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(x));
        return r;
      };
      auto half = [&](int w) { return w & 1 ? f32x2{xv[w >> 1][2], xv[w >> 1][3]} : f32x2{xv[w >> 1][0], xv[w >> 1][1]}; };
      constexpr int W0 = DCLS == 4 ? 0 : 1, NW = DCLS == 4 ? 8 : 6;   // the sample pairs that are used
      if (g == 0) {
        asm volatile("" : "+v"(xv[0]), "+v"(xv[1]), "+v"(xv[2]), "+v"(xv[3]), "+v"(ptc));   // (pins the wait for the loads here, as below)
#pragma unroll
        for (int k = 0; k < 4; k++) ptm[k] = tok[k] ? ptc : 0.f;
      } else if (g <= 3) {
#pragma unroll
        for (int w = W0 + 3 * (g - 1); w < W0 + 3 * g && w < W0 + NW; w++) su[w] = pk_bc(half(w), ptm[w >> 1]);
      } else if (g <= 7) {
        if constexpr (DCLS == 1) {
          const int i = g - 4;
          sc[i] = pk_sumdiff(su[i + 2]);
          sc0[i] = su[i + 1][1] - su[i + 2][1];
          sc3[i] = su[i + 3][0] - su[i + 2][0];
        } else {
          const int h = (g - 4) >> 1;
          auto tap = [&](int k) { return DCLS == 4 ? su[2 * k + h] : su[1 + 2 * h + k]; };
          if (((g - 4) & 1) == 0) sc[4 * h + 0] = pk_sub(tap(0), tap(2)), sc[4 * h + 1] = pk_add(tap(1), tap(2));
          else sc[4 * h + 2] = pk_sub(tap(2), tap(1)), sc[4 * h + 3] = pk_sub(tap(3), tap(1));
        }
      } else {
        float *q = dst + 4 * xq * XS_ + xc;
        const int w = g - 8;
        if constexpr (DCLS == 1) {
          const int i = w >> 1;
          if ((w & 1) == 0) q[i * XS_] = sc0[i], q[i * XS_ + XCOMP_] = sc[i][0];
          else q[i * XS_ + 2 * XCOMP_] = sc[i][1], q[i * XS_ + 3 * XCOMP_] = sc3[i];
        } else {
          const int h = w >> 2, comp = w & 3;
          q[2 * h * XS_ + comp * XCOMP_] = sc[4 * h + comp][0];
          q[(2 * h + 1) * XS_ + comp * XCOMP_] = sc[4 * h + comp][1];
        }
      }
    };
    auto store_x = [&](float *dst) {                             // FiLM add (WaveNet.py:84), zero padding (:26-27), input differences
      if constexpr (QUAD) {
#pragma unroll
        for (int g = 0; g < 16; g++) stage(dst, g);
        return;
      }
      // (the loaded values pass through an empty asm: it pins this arithmetic -- and the wait for the loads -- HERE; instruction
      // selection would otherwise place it right behind the loads, half a chunk early)
      asm volatile("" : "+v"(xr[0][0]), "+v"(xr[0][1]), "+v"(xr[0][2]), "+v"(xr[0][3]), "+v"(xr[1][0]), "+v"(xr[1][1]), "+v"(xr[1][2]),
                   "+v"(xr[1][3]), "+v"(xr[2][0]), "+v"(xr[2][1]), "+v"(xr[2][2]), "+v"(xr[2][3]), "+v"(xr[3][0]), "+v"(xr[3][1]),
                   "+v"(xr[3][2]), "+v"(xr[3][3]), "+v"(ptq));
      f32x4 c0, c1, c2, c3;
#pragma unroll
      for (int cc = 0; cc < 4; cc++) {
        const float u0 = tok[0] ? xr[cc][0] + ptq[cc] : 0.f;
        const float u1 = tok[1] ? xr[cc][1] + ptq[cc] : 0.f;
        const float u2 = tok[2] ? xr[cc][2] + ptq[cc] : 0.f;
        const float u3 = tok[3] ? xr[cc][3] + ptq[cc] : 0.f;
        c0[cc] = u0 - u2;
        c1[cc] = u1 + u2;
        c2[cc] = u2 - u1;
        c3[cc] = u3 - u1;
      }
      float *q = dst + j * XS_ + 4 * sq;
      *reinterpret_cast<f32x4 *>(q) = c0;
      *reinterpret_cast<f32x4 *>(q + XCOMP_) = c1;
      *reinterpret_cast<f32x4 *>(q + 2 * XCOMP_) = c2;
      *reinterpret_cast<f32x4 *>(q + 3 * XCOMP_) = c3;
    };

    // ---- the first tile's first weights and first chunk of X (later tiles: requested at the end of the tile before)
    f32x4 a[4][4];                                               // [product][row tile]: a ring one k-group (four units, 64 MFMAs) deep
    set_tile(t_first);
#pragma unroll
    for (int u = 0; u < 4; u++) load_a1(a[u], (unsigned)u);
    issue_x(0);

#pragma unroll 1
  for (int tile = t_first; tile < t_end; tile += t_step) {
    f32x16 acc[4][4];                                            // [product][row tile]; the dilated conv's bias rides on m2 (in both outputs)
    const float *xfrag = lds + j * XS_ + 4 * hh;
    f32x4 bqc[2];                                                // SEAM: the B fragments, carried from chunk to chunk
    if constexpr (SEAM) {
      // the first fragment is on its way while the bias init below reads LDS and writes its 64 accumulators
      store_x(lds);
      __syncthreads();
      bqc[0] = *reinterpret_cast<const f32x4 *>(xfrag);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int rt = 0; rt < 4; rt++) {
      const int obase = (rt & 1) * C + 64 * wave + 32 * (rt >> 1);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const f32x4 bv = ld_b1(obase + 8 * q + 4 * hh);
        acc[1][rt][4 * q + 0] = bv[0];
        acc[1][rt][4 * q + 1] = bv[1];
        acc[1][rt][4 * q + 2] = bv[2];
        acc[1][rt][4 * q + 3] = bv[3];
      }
      if constexpr (!ZERO) {
#pragma unroll
        for (int r = 0; r < 16; r++) acc[0][rt][r] = acc[2][rt][r] = acc[3][rt][r] = 0.f;
      }
    }
    if constexpr (!SEAM) {
      store_x(lds);
      __syncthreads();
    }

    // ---- GEMM1: 8 chunks x 4 k-groups x 4 products; a unit = 16 MFMAs on one B fragment.  Chunk c + 1 is requested at chunk c's top and
    // staged in its unit 12.  Without CARRY every chunk does so (no branches: the last one re-requests itself, unused); with it the
    // last chunk runs a body that requests and stages nothing.
    constexpr int NSTAGE = CARRY ? NCH_ - 1 : NCH_;
    // SEAM: MFMAs run through the chunk turn.  Chunk c's barrier stands in its unit 15, behind the wait that delivers that unit's
    // own fragment, and chunk c + 1's first fragment is read right behind it, under unit 15's MFMAs.  Two X sub-buffers are still
    // enough: every read of buffer c & 1 is complete before barrier(c) -- the last one is the fragment just waited for -- and the
    // buffer's next writes are chunk c + 1's staging in its unit 12, behind barrier(c); buffer (c + 1) & 1 was written in unit 12
    // of chunk c -- LDS operations retire in order, so the same wait covers the wave's own writes -- before barrier(c) and is first
    // read behind it.  Tile top and g image as before: buffer 0 is last read before chunk 6's barrier.  The X request of chunk
    // c + 2 (17 loads) leaves the chunk top for unit 13 of chunk c, one load behind each MFMA, right behind the staging that frees
    // its registers and in front of the weight loads of units 13..15, whose waits come four units later; chunk 0 also requests
    // chunk 1 at its top as before, chunk 6 re-requests chunk 7, unused (no branch: this kernel spills when a main loop gets one).
    // QUAD: the request is four 16-byte loads in unit 13's first four gaps, and the staging's LDS writes are sixteen ds_write_b32 in
    // gaps 8..15 of unit 12 instead of four ds_write_b128 behind its last MFMA.  The argument above holds as it stands: the writes of
    // chunk c + 1's image still go to buffer (c + 1) & 1, whose last read was waited for before barrier(c - 1) and which nobody reads
    // again before barrier(c); they are all issued in unit 12, three units before barrier(c) in unit 15, and the wait in front of that
    // barrier retires them with the fragment it delivers.  part_t comes from the launch constants' LDS copy, read with the request.
    auto chunk = [&](int ch, auto stage_tag, auto first_tag) __attribute__((always_inline)) {
      constexpr bool STAGE = decltype(stage_tag)::value, FIRST = decltype(first_tag)::value;
      constexpr bool XREQ = SEAM && STAGE;
      const float *xb = xfrag + (ch & 1) * XBUF_;
      if constexpr (STAGE && (!SEAM || FIRST)) issue_x(ch + 1 < NCH_ ? ch + 1 : ch);
      f32x4 bql[2];
      f32x4(&bq)[2] = SEAM ? bqc : bql;
      if constexpr (!SEAM) bq[0] = *reinterpret_cast<const f32x4 *>(xb);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kg = 0; kg < 4; kg++) {
#pragma unroll
        for (int comp = 0; comp < 4; comp++) {
          const int u = 4 * kg + comp;
          if (SEAM && u == 15) {
            __syncthreads();
            if constexpr (STAGE) bq[0] = *reinterpret_cast<const f32x4 *>(xfrag + ((ch + 1) & 1) * XBUF_);
            __builtin_amdgcn_sched_barrier(0);
          }
          if (XREQ && u == 13) issue_x(ch + 2 < NCH_ ? ch + 2 : NCH_ - 1);
          if (u + 1 < 16) bq[(u + 1) & 1] = *reinterpret_cast<const f32x4 *>(xb + ((u + 1) & 3) * XCOMP_ + ((u + 1) >> 2) * 8);
          // the next chunk's FiLM add / padding / differences / LDS writes ride in the MFMA gaps of unit 12 (the X loads were
          // requested twelve units = 12 k cycles ago)
          if (STAGE && u == 12 && !QUAD) store_x(lds + ((ch + 1) & 1) * XBUF_);
          auto mfma = [&](int rt, int e) __attribute__((always_inline)) {
            if (FIRST && kg == 0 && e == 0 && comp != 1)           // (m2 starts from the bias)
              acc[comp][rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[comp][rt][e], bq[u & 1][e], f32x16{}, 0, 0, 0);
            else
              acc[comp][rt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[comp][rt][e], bq[u & 1][e], acc[comp][rt], 0, 0, 0);
          };
#pragma unroll
          for (int e = 0; e < 4; e++)
#pragma unroll
            for (int rt = 0; rt < 4; rt++) {
              mfma(rt, e);
              if (QUAD && STAGE && u == 12) {                      // one step of the staging behind each MFMA, in this order
                stage(lds + ((ch + 1) & 1) * XBUF_, 4 * e + rt);
                __builtin_amdgcn_sched_barrier(0);
              }
            }
          if (STAGE && u == 12 && !QUAD) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
              __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x200, 4, 0);
          }
          if (XREQ && u == 13) {                                   // (not QUAD: the seventeenth load behind the last MFMA; QUAD: four loads, four gaps)
#pragma unroll
            for (int i = 0; i < (QUAD ? 4 : 16); i++) {
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
              __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
          // the same product's unit of the next k-group takes over this unit's registers (the last k-group wraps to the image's
          // first units: CARRY keeps them for the next tile -- same layer, same image; otherwise unused)
          load_a1(a[comp], (unsigned)((16 * ch + u + 4) & (16 * NCH_ - 1)));
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    };
    if constexpr (ZERO) {
      chunk(0, std::true_type{}, std::true_type{});
      if constexpr (!SEAM) __syncthreads();
    }
#pragma unroll 1
    for (int ch = ZERO ? 1 : 0; ch < NSTAGE; ch++) {
      chunk(ch, std::true_type{}, std::false_type{});
      if constexpr (!SEAM) __syncthreads();
    }
#pragma unroll 1
    for (int ch = NSTAGE; ch < NCH_; ch++) {
      chunk(ch, std::false_type{}, std::false_type{});
      if constexpr (!SEAM) __syncthreads();
    }

    // sample of GEMM2 column (ct, j)
    const int tfirst = ((p0 >> logd) << (logd + 1)) + (p0 & (d - 1));
    int tcol[2];
    tcol[0] = tfirst + j;
    tcol[1] = tfirst + (d >= 32 ? d : 32) + j;
    // SAVE: this lane's pair's two samples as byte offsets into the clip's pre-gate rows (past the clip: dropped by the range check)
    __amdgpu_buffer_rsrc_t ars = hrs;
    unsigned sv0 = 0, sv1 = 0;
    if constexpr (SAVE) {
      ars = uni_rsrc(aout + (size_t)b * 2 * C * L, 2u * clip_bytes);
      const int pj = p0 + j;
      const int s0 = ((pj >> logd) << (logd + 1)) + (pj & (d - 1));
      sv0 = s0 < L ? (unsigned)s0 * 4u : 0x80000000u;
      sv1 = s0 + d < L ? (unsigned)(s0 + d) * 4u : 0x80000000u;
    }
    // ---- output transform, gate (WaveNet.py:90) -> g image [column][channel]
    {
      float *g0 = lds + GOFF_ + col0 * GS_ + 64 * wave + 4 * hh;
      float *g1 = lds + GOFF_ + col1 * GS_ + 64 * wave + 4 * hh;
#pragma unroll
      for (int p = 0; p < 2; p++) {
        // (pins the eight product tiles of this channel half in the accumulator registers up to here: the register allocator
        // would otherwise move all 256 accumulators to VGPRs at the loop's exit -- there is no room -- and spill them)
#pragma unroll
        for (int c4 = 0; c4 < 4; c4++) asm volatile("" : "+a"(acc[c4][2 * p]), "+a"(acc[c4][2 * p + 1]));
#pragma unroll
        for (int q = 0; q < 4; q++) {
          f32x4 v0, v1;
          if constexpr (PK) {
            // the same sums, in the same order, and gate2 = gate element for element, on accumulator registers (r, r + 1): two
            // elements per issue slot, the result pairs the halves of the ds_write_b128 operands
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
              const int r = 4 * q + e;
              auto pr = [&](const f32x16 &t) { return f32x2{t[r], t[r + 1]}; };
              const f32x2 ta = (pr(acc[0][2 * p]) + pr(acc[1][2 * p])) + pr(acc[2][2 * p]);
              const f32x2 sa = (pr(acc[0][2 * p + 1]) + pr(acc[1][2 * p + 1])) + pr(acc[2][2 * p + 1]);
              const f32x2 tb = (pr(acc[1][2 * p]) - pr(acc[2][2 * p])) + pr(acc[3][2 * p]);
              const f32x2 sb = (pr(acc[1][2 * p + 1]) - pr(acc[2][2 * p + 1])) + pr(acc[3][2 * p + 1]);
              const f32x2 ga = gate2(ta, sa), gb = gate2(tb, sb);
              v0[e] = ga[0], v0[e + 1] = ga[1];
              v1[e] = gb[0], v1[e + 1] = gb[1];
              if constexpr (SAVE) {
                const unsigned so = ((unsigned)(64 * wave + 32 * p + 4 * hh) * (unsigned)L) * 4u;
                // (the whole pair, then index: element-wise bit_cast of a vector element mis-folds to a splat)
                const u32x2 tau = __builtin_bit_cast(u32x2, ta), sau = __builtin_bit_cast(u32x2, sa);
                const u32x2 tbu = __builtin_bit_cast(u32x2, tb), sbu = __builtin_bit_cast(u32x2, sb);
#pragma unroll
                for (int i = 0; i < 2; i++) {
                  const int ro = rowoff(r + i, 0) * L * 4;
                  __builtin_amdgcn_raw_buffer_store_b32(tau[i], ars, so + sv0, ro, 0);
                  __builtin_amdgcn_raw_buffer_store_b32(sau[i], ars, so + sv0 + (unsigned)C * (unsigned)L * 4u, ro, 0);
                  __builtin_amdgcn_raw_buffer_store_b32(tbu[i], ars, so + sv1, ro, 0);
                  __builtin_amdgcn_raw_buffer_store_b32(sbu[i], ars, so + sv1 + (unsigned)C * (unsigned)L * 4u, ro, 0);
                }
              }
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; e++) {
              const int r = 4 * q + e;
              const float ta = (acc[0][2 * p][r] + acc[1][2 * p][r]) + acc[2][2 * p][r];
              const float sa = (acc[0][2 * p + 1][r] + acc[1][2 * p + 1][r]) + acc[2][2 * p + 1][r];
              const float tb = (acc[1][2 * p][r] - acc[2][2 * p][r]) + acc[3][2 * p][r];
              const float sb = (acc[1][2 * p + 1][r] - acc[2][2 * p + 1][r]) + acc[3][2 * p + 1][r];
              v0[e] = gate(ta, sa);
              v1[e] = gate(tb, sb);
              if constexpr (SAVE) {                                // channel 64 wave + 32 p + rowoff(r, hh), samples of this lane's pair
                const unsigned so = ((unsigned)(64 * wave + 32 * p + 4 * hh) * (unsigned)L) * 4u;
                const int ro = rowoff(r, 0) * L * 4;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, ta), ars, so + sv0, ro, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, sa), ars, so + sv0 + (unsigned)C * (unsigned)L * 4u, ro, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, tb), ars, so + sv1, ro, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, sb), ars, so + sv1 + (unsigned)C * (unsigned)L * 4u, ro, 0);
              }
            }
          }
          *reinterpret_cast<f32x4 *>(g0 + 32 * p + 8 * q) = v0;   // channels 64 wave + 32 p + 8 q + 4 hh + (0..3)
          *reinterpret_cast<f32x4 *>(g1 + 32 * p + 8 * q) = v1;
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }

    // ---- GEMM2: row tiles 0,1 = res_conv rows, 2,3 = skip_conv rows of this wave's 64 channels; 64 sample columns
    f32x16 acc2[4][2];
    {
#pragma unroll
      for (int rt = 0; rt < 4; rt++) {
        if (NOH && rt < 2) continue;
        const int cb = 64 * wave + 32 * (rt & 1);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int c = cb + 8 * q + 4 * hh;
          f32x4 bv = ld_b2((rt < 2 ? 0 : C) + c);
          if (rt < 2) bv += ld_pt(c);                            // u = h + part_t re-enters the residual (WaveNet.py:84,97)
#pragma unroll
          for (int ct = 0; ct < 2; ct++) {
            acc2[rt][ct][4 * q + 0] = bv[0];
            acc2[rt][ct][4 * q + 1] = bv[1];
            acc2[rt][ct][4 * q + 2] = bv[2];
            acc2[rt][ct][4 * q + 3] = bv[3];
          }
        }
      }
    }
    f32x4 a2[2][4];                                              // ring of two k-groups (64 MFMAs)
    f32x4 a2r[4][2];                                             // ROWS: two row tiles per pass, so the same registers hold four k-groups
    auto load_a2r = [&](f32x4(&a)[2], unsigned soff) {           // soff: k-group kg, row tiles rt0, rt0 + 1 = kg * UNIT_BYTES_ + rt0 * 1024
#pragma unroll
      for (int r = 0; r < 2; r++)
        a[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w2rs, lane16 + r * 1024u, soff, 0));
    };
    if constexpr (ROWS) {
#pragma unroll
      for (int k = 0; k < 4; k++) load_a2r(a2r[k], (unsigned)k * UNIT_BYTES_);
    } else {
#pragma unroll
      for (int k = 0; k < 2; k++) load_a2(a2[k], (unsigned)k);
    }

    // The residual's h patch (this wave's 64 res rows x 64 columns) is requested now -- behind the first weight groups, so that
    // their waits do not include it -- and consumed after GEMM2: the epilogue never waits on memory.
    __builtin_amdgcn_sched_barrier(0);
    float hres[Q16 ? 1 : 2][Q16 ? 1 : 2][16];
    f32x4 hq[Q16 ? 2 : 1][Q16 ? 2 : 1][4];                      // Q16: [res row tile][column tile][row octet p]: row l / 8 + 8 p, samples 4 (l % 8) ..
    unsigned eo4[2] = {0x80000000u, 0x80000000u};
    if constexpr (Q16) {
      const int rowq = lane >> 3, cq = lane & 7;
#pragma unroll
      for (int ct = 0; ct < 2; ct++) {
        const int t = tfirst + (ct ? (d >= 32 ? d : 32) : 0) + 4 * cq;
        eo4[ct] = t < L ? ((unsigned)(64 * wave + rowq) * (unsigned)L + (unsigned)t) * 4u : 0x80000000u;
      }
      if (!NOH) {
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
          for (int ct = 0; ct < 2; ct++)
#pragma unroll
            for (int p = 0; p < 4; p++)
              hq[rt][ct][p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(hrs, eo4[ct], (32 * rt + 8 * p) * L * 4, 2));
      }
    }
    if (!Q16 && !NOH) {
#pragma unroll
      for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int ct = 0; ct < 2; ct++) {
          const unsigned ev = ((unsigned)(64 * wave + 32 * rt + 4 * hh) * (unsigned)L + (unsigned)min(tcol[ct], L - 1)) * 4u;
#pragma unroll
          for (int r = 0; r < 16; r++)
            hres[rt][ct][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(hrs, ev, rowoff(r, 0) * L * 4, 2));
        }
    }
    __syncthreads();                                             // g image complete

    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const float RS = 0.707106781186547524f;   // float(math.sqrt(0.5))
    if constexpr (ROWS) {
      // ---- GEMM2 by rows: k-groups 0..31 on the two res row tiles, then 0..31 on the two skip row tiles -- every accumulator sees
      // its k-groups in the order it always did -- and in the gaps of the second pass the four res tiles leave as they do in the
      // epilogue below (patch write, four ds_read_b128, (hq + v) * RS, 16-byte stores; the patches are wave-private and lie
      // behind the g image).  A tile's hq registers, free once it has left, take that tile's running skip rows: requested here,
      // used after the loop (without `accumulate` from a descriptor of no bytes: zeros, no branch).  g fragments are read twice
      // and a k-group ahead; the weight ring is four k-groups deep (4 k cycles), which also covers the h' stores that are now
      // older than weight loads in the vmcnt queue.
      const __amdgpu_buffer_rsrc_t ors = uni_rsrc(hout + (size_t)b * C * L, clip_bytes);
      const __amdgpu_buffer_rsrc_t sls = uni_rsrc(skip + (size_t)b * C * L, accumulate ? clip_bytes : 0u);
      const float *gfrag = lds + GOFF_ + j * GS_ + 4 * hh;
      float *patch0 = lds + POFF_ + wave * (2 * 32 * PS_);
      const int rowq = lane >> 3, cq = lane & 7;
      f32x4 bq2[2][2];
      bq2[0][0] = *reinterpret_cast<const f32x4 *>(gfrag);
      bq2[0][1] = *reinterpret_cast<const f32x4 *>(gfrag + 32 * GS_);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
      for (int kg4 = 0; kg4 < C / 8; kg4 += 4) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int kn = (kg4 + k + 1) & (C / 8 - 1);            // (the last one wraps: the second pass's first fragments)
          bq2[(k + 1) & 1][0] = *reinterpret_cast<const f32x4 *>(gfrag + 8 * kn);
          bq2[(k + 1) & 1][1] = *reinterpret_cast<const f32x4 *>(gfrag + 32 * GS_ + 8 * kn);
#pragma unroll
          for (int e = 0; e < 4; e++)
#pragma unroll
            for (int rt = 0; rt < 2; rt++)
#pragma unroll
              for (int ct = 0; ct < 2; ct++)
                acc2[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2r[k][rt][e], bq2[k & 1][ct][e], acc2[rt][ct], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          const int nx = kg4 + k + 4;                            // (the last four request the skip rows' first four k-groups)
          load_a2r(a2r[k], nx < C / 8 ? (unsigned)nx * UNIT_BYTES_ : (unsigned)(nx - C / 8) * UNIT_BYTES_ + 2048u);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int t = 0; t < 4; t++) {                              // res tile t = (row tile t >> 1, column tile t & 1) leaves under k-groups 8 t ..
        const int rt = t >> 1, ct = t & 1;
        float *patch = patch0 + (t & 1) * (32 * PS_);
        f32x4 pv[4];
#pragma unroll
        for (int k8 = 0; k8 < 8; k8++) {
          const int kg = 8 * t + k8, k = kg & 3;
          if (kg + 1 < C / 8) {
            bq2[(kg + 1) & 1][0] = *reinterpret_cast<const f32x4 *>(gfrag + 8 * (kg + 1));
            bq2[(kg + 1) & 1][1] = *reinterpret_cast<const f32x4 *>(gfrag + 32 * GS_ + 8 * (kg + 1));
          }
          if (k8 == 0) {
#pragma unroll
            for (int r = 0; r < 16; r++) patch[rowoff(r, hh) * PS_ + j] = acc2[rt][ct][r];
          }
          if (k8 == 1) {
#pragma unroll
            for (int p = 0; p < 4; p++) pv[p] = *reinterpret_cast<const f32x4 *>(patch + (rowq + 8 * p) * PS_ + 4 * cq);
          }
          if (k8 == 2) {
#pragma unroll
            for (int p = 0; p < 4; p++) {
              const f32x4 o = (hq[rt][ct][p] + pv[p]) * RS;
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ors, eo4[ct], (32 * rt + 8 * p) * L * 4, 2);
            }
          }
#pragma unroll
          for (int e = 0; e < 4; e++)
#pragma unroll
            for (int r2 = 0; r2 < 2; r2++)
#pragma unroll
              for (int c2 = 0; c2 < 2; c2++)
                acc2[2 + r2][c2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2r[k][r2][e], bq2[kg & 1][c2][e], acc2[2 + r2][c2], 0, 0, 0);
          if (k8 == 0) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
              __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
              __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
            }
          }
          if (k8 == 2) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
              __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x040, 4, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
          load_a2r(a2r[k], (unsigned)((kg + 4) & (C / 8 - 1)) * UNIT_BYTES_ + 2048u);   // (the last four wrap: unused)
          if (k8 == 3) {                                         // behind this k-group's weights: their wait does not include these
#pragma unroll
            for (int p = 0; p < 4; p++)
              hq[rt][ct][p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(sls, eo4[ct], (32 * rt + 8 * p) * L * 4, 2));
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    } else {
      const float *gfrag = lds + GOFF_ + j * GS_ + 4 * hh;
#pragma unroll 1
      for (int kg4 = 0; kg4 < C / 8; kg4 += 4) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int kg = kg4 + k;
          f32x4 bq2[2];
          bq2[0] = *reinterpret_cast<const f32x4 *>(gfrag + 8 * kg);
          bq2[1] = *reinterpret_cast<const f32x4 *>(gfrag + 32 * GS_ + 8 * kg);
#pragma unroll
          for (int e = 0; e < 4; e++)
#pragma unroll
            for (int rt = NOH ? 2 : 0; rt < 4; rt++)
#pragma unroll
              for (int ct = 0; ct < 2; ct++)
                acc2[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[k & 1][rt][e], bq2[ct][e], acc2[rt][ct], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          load_a2(a2[k & 1], (unsigned)((kg + 2) & (C / 8 - 1)));
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }

    const __amdgpu_buffer_rsrc_t ors = uni_rsrc((NOH ? skip : hout) + (size_t)b * C * L, clip_bytes);
    const __amdgpu_buffer_rsrc_t srs = uni_rsrc(skip + (size_t)b * C * L, clip_bytes);     // S == C
    if constexpr (Q16) {
      // ---- 16-byte epilogue (WaveNet.py:97, :133).  Order: the running skip rows are requested, the res tiles leave (h'), the NEXT
      // tile's first weights and X chunk are requested, the skip tiles leave -- so the next tile's first wait has only the 16 skip
      // stores behind its loads (vmcnt retires in order).
      f32x4 sk4[2][2][4];
      if constexpr (ROWS) {                                      // (requested inside GEMM2, into the hq registers)
      } else if (accumulate) {
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
          for (int ct = 0; ct < 2; ct++)
#pragma unroll
            for (int p = 0; p < 4; p++)
              sk4[rt][ct][p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srs, eo4[ct], (32 * rt + 8 * p) * L * 4, 2));
      } else {
#pragma unroll
        for (int i = 0; i < 16; i++) (&sk4[0][0][0])[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      float *patch0 = lds + POFF_ + wave * (2 * 32 * PS_);
      const int rowq = lane >> 3, cq = lane & 7;
      auto leave = [&](int k, const f32x16 &tile, auto &&out4) {  // accumulator tile -> patch k & 1 -> 4 x (row, 4 samples) per lane
        float *patch = patch0 + (k & 1) * (32 * PS_);
#pragma unroll
        for (int r = 0; r < 16; r++) patch[rowoff(r, hh) * PS_ + j] = tile[r];
#pragma unroll
        for (int p = 0; p < 4; p++) out4(p, *reinterpret_cast<const f32x4 *>(patch + (rowq + 8 * p) * PS_ + 4 * cq));
      };
      {
        if (!NOH && !ROWS) {
#pragma unroll
          for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int ct = 0; ct < 2; ct++)
              leave(2 * rt + ct, acc2[rt][ct], [&](int p, f32x4 v) {
                const f32x4 o = (hq[rt][ct][p] + v) * RS;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ors, eo4[ct], (32 * rt + 8 * p) * L * 4, 2);
              });
        }
      }
      {
        set_tile(tile + t_step < t_end ? tile + t_step : tile);  // (the last tile re-requests itself, unused)
        if constexpr (!CARRY) {
#pragma unroll
          for (int u = 0; u < 4; u++) load_a1(a[u], (unsigned)u);
        }
        issue_x(0);
      }
      __builtin_amdgcn_sched_barrier(0);
      {
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
          for (int ct = 0; ct < 2; ct++)
            leave(2 * rt + ct, acc2[2 + rt][ct], [&](int p, f32x4 v) {
              f32x4 o;
              if constexpr (ROWS) o = hq[rt][ct][p] + v; else o = sk4[rt][ct][p] + v;
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), srs, eo4[ct], (32 * rt + 8 * p) * L * 4, 2);
            });
      }
      continue;
    }
    // ---- the NEXT tile's first weights and first chunk of X are requested here, ahead of this tile's stores: vmcnt retires in
    // order, so requested after them their wait would include the 64 float atomics (thousands of cycles each to retire with every
    // CU issuing them); requested before, it includes at most the plain h' stores (the counter holds 63: the wait for these loads
    // lets the youngest 63 operations -- the atomics -- stay outstanding)
    {
      set_tile(tile + t_step < t_end ? tile + t_step : tile);    // (the last tile re-requests itself, unused)
      if constexpr (!CARRY) {
#pragma unroll
        for (int u = 0; u < 4; u++) load_a1(a[u], (unsigned)u);
      }
      issue_x(0);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- epilogue (WaveNet.py:97, :133): buffer stores / memory-side float atomics -- one VGPR offset per 32 x 32 tile, the row
    // stride in SGPR offsets, columns past the clip's end dropped by the range check (no address arithmetic, no branches)
    {
      typedef unsigned u32x16 __attribute__((ext_vector_type(16)));
      const float RS = 0.707106781186547524f;   // float(math.sqrt(0.5))
#pragma unroll
      for (int rt = NOH ? 2 : 0; rt < 4; rt++) {
#pragma unroll
        for (int ct = 0; ct < 2; ct++) {
          const int t = tcol[ct];
          const unsigned eo = t < L ? ((unsigned)(64 * wave + 32 * (rt & 1) + 4 * hh) * (unsigned)L + (unsigned)t) * 4u : 0x80000000u;
          if (rt < 2) {
#pragma unroll
            for (int r = 0; r < 16; r++)
              // nt (also the skip store below): once-written streams must not displace the h rows in the XCD's L2, which
              // neighbouring tiles' taps and the residual read again
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (hres[rt & 1][ct][r] + acc2[rt][ct][r]) * RS), ors, eo,
                                                    rowoff(r, 0) * L * 4, 2);
          } else if (accumulate) {
#pragma unroll
            for (int r = 0; r < 16; r++)
              (void)__builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(acc2[rt][ct][r], srs, (int)eo, rowoff(r, 0) * L * 4, 0);
          } else {
            const u32x16 av = __builtin_bit_cast(u32x16, acc2[rt][ct]);   // (the whole vector, then index: element-wise bit_cast of a vector element mis-folds to a splat)
#pragma unroll
            for (int r = 0; r < 16; r++)
              __builtin_amdgcn_raw_buffer_store_b32(av[r], srs, eo, rowoff(r, 0) * L * 4, 2);
          }
        }
      }
    }
    // the next tile's staging writes X buffer 0 (last read before chunk 6's barrier) and its gate writes the g image only after
    // eight more barriers: no extra barrier needed here
  }
}

#ifdef AP_TOOLS
// the DIET masks the tools build instantiates beside the product's (each item alone on top of its predecessor's product mask)
#define AP_F32W_AB_MASKS(X) X(0) X(2) X(4) X(6) X(22) X(54) X(150) X(182) X(1206)
#endif

// one 16-byte form at DIET mask M; with DIET_QUAD_ the instantiation of the layer's dilation class
template <bool NOH, bool SAVE, int M, class... A>
static void launch_q16(unsigned grid, unsigned wg, hipStream_t st, int dcls, A... args) {
  if constexpr ((M & DIET_QUAD_) != 0) {
    if (dcls == 1) return resblock_f32w_kernel<NOH, SAVE, true, M, 1><<<grid, wg, 0, st>>>(args...);
    if (dcls == 2) return resblock_f32w_kernel<NOH, SAVE, true, M, 2><<<grid, wg, 0, st>>>(args...);
  }
  resblock_f32w_kernel<NOH, SAVE, true, M><<<grid, wg, 0, st>>>(args...);
}

// BLOCK_F32_F23: NOH / SAVE / 16-byte / quad-class / DIET mask as planned
int launch_block_f32w(ap_ctx *ctx, const BlockPlan &p, int layer, const float *hin, const float *pt, float *hout, float *skip, int accumulate, int L,
                      hipStream_t st, float *aout) {
  const int C = ctx->C, S = ctx->S, logd = p.logd, ntiles = p.ntiles, nblk = (int)p.nblk;
  const float *w1w = ctx->w1w + (size_t)layer * 4 * 2 * C * C, *w2w = ctx->w2w + (size_t)layer * (C + S) * C;
  const float *b1 = ctx->b1 + (size_t)layer * 2 * C, *b2 = ctx->b2 + (size_t)layer * (C + S);
  float *const none = nullptr;
  if (p.save && p.q16) launch_q16<false, true, AP_F32W_DIET>(p.grid, p.wg, st, p.dcls, hin, pt, hout, skip, w1w, b1, w2w, b2, L, logd, accumulate, ntiles, nblk, aout);
  else if (p.save) resblock_f32w_kernel<false, true, false, DIET4_><<<p.grid, p.wg, 0, st>>>(hin, pt, hout, skip, w1w, b1, w2w, b2, L, logd, accumulate, ntiles, nblk, aout);
#ifdef AP_TOOLS
#define AP_F32W_AB(M) else if (p.diet == M) launch_q16<false, false, M>(p.grid, p.wg, st, p.dcls, hin, pt, hout, skip, w1w, b1, w2w, b2, L, logd, accumulate, ntiles, nblk, none);
  AP_F32W_AB_MASKS(AP_F32W_AB)
#undef AP_F32W_AB
#endif
  else if (!p.noh && p.q16) launch_q16<false, false, AP_F32W_DIET>(p.grid, p.wg, st, p.dcls, hin, pt, hout, skip, w1w, b1, w2w, b2, L, logd, accumulate, ntiles, nblk, none);
  else if (!p.noh) resblock_f32w_kernel<false, false, false, DIET4_><<<p.grid, p.wg, 0, st>>>(hin, pt, hout, skip, w1w, b1, w2w, b2, L, logd, accumulate, ntiles, nblk, nullptr);
  else if (p.q16) launch_q16<true, false, AP_F32W_DIET>(p.grid, p.wg, st, p.dcls, hin, pt, hout, skip, w1w, b1, w2w, b2, L, logd, accumulate, ntiles, nblk, none);
  else resblock_f32w_kernel<true, false, false, DIET4_><<<p.grid, p.wg, 0, st>>>(hin, pt, hout, skip, w1w, b1, w2w, b2, L, logd, accumulate, ntiles, nblk, nullptr);
  AP_HIP(hipGetLastError());
  return 0;
}

}  // namespace ap

#ifdef AP_TOOLS
extern "C" int ap_debug_f32w_q16(int on) {
  ap::g_block_tune.no_q16 = on ? 0 : 1;
  return 0;
}
// the block's launch as the chains call it: h_out NULL = the last layer's form (no per-block entry point of include/audiopure.h reaches
// it), pre_gate non-NULL = the SAVE form; 1: this context's block is not the minimal-filtering one
extern "C" int ap_debug_resblock_f32w(ap_ctx *ctx, int layer, const float *h_in, const float *part_t_layer, float *h_out, float *skip,
                                      int accumulate, int B, int L, void *stream, float *pre_gate) {
  if (!ap::block_f32w_serves(ap::block_ask(ctx, layer, B, L))) return 1;
  return ap::launch_resblock(ctx, layer, h_in, part_t_layer, h_out, skip, accumulate, B, L, (hipStream_t)stream, pre_gate);
}
// the h'-writing 16-byte form (what the headline runs 175 of 180 launches on) with the product's DIET mask or one of AP_F32W_AB_MASKS
// (54 = 22 + pairs, 150 = 22 + no zeroing, 182 = both: the product before the seamless chunk turn); every other form keeps
// the product's mask
extern "C" int ap_debug_f32w_diet(int mask) {
  bool known = mask == AP_F32W_DIET;
#define AP_F32W_KNOWN(M) known = known || mask == M;
  AP_F32W_AB_MASKS(AP_F32W_KNOWN)
#undef AP_F32W_KNOWN
  if (!known) return -22;
  ap::g_block_tune.diet = mask == AP_F32W_DIET ? -1 : mask;
  return 0;
}
#endif
