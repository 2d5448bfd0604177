// AP_PREC_BF16, persistent form: fused Residual_block.forward (WaveNet.py:75-97) with bf16 MFMA operands, fp32 accumulate,
// fp32 activations in HBM -- the same arithmetic and the same packed weight images as tools/csrc/ap_resblock_bf16.hip (outputs are
// bit-identical: tools/cmp_bf16_kernels.py), every dilation (d <= 32 stages one 192-column window per chunk for the three taps), restructured
// around what the round-2 ablations measured (docs/HISTORY.md):
//
//   * with GEMM1 emptied the old kernel still took 52 % of its time, and 60 % of THAT was the residual / skip
//     read-modify-write traffic (262 KB of loads + 262 KB of stores per 128-sample tile) issued in two bursts at the very
//     end of a workgroup's life: every CU alternated between a phase that used no memory bandwidth and a phase that used
//     nothing else, then paid a store drain (s_endpgm waits for vmcnt = 0), a workgroup launch and a cold first load.
//
// Here one workgroup per CU walks its tiles in a loop (XCD-local order), and the memory traffic of a tile is spread over
// the tile and into the next one:
//   - the h patch the residual needs is requested before and during the gate, the running skip rows during the gate and the
//     first epilogue (the GEMM1 accumulators free up as they are gated);
//   - the first X chunk of the NEXT tile is requested before GEMM2's second pass and packed -- with that tile's first
//     weight fragments and second chunk requested -- before the last epilogue's stores, so the stores of a tile drain
//     behind the next tile's GEMM1 (vmcnt retires in order: a load issued after a store cannot be waited for without
//     waiting for the store);
//   - the next chunk's FiLM add / bf16 pack / ds_write sit between the MFMAs of a chunk's fourth k-step (two X buffers
//     instead of three), so the chunk has no VALU-only tail;
//   - no register is spilled: a scratch reload inside the tile loop is a vector-memory load whose wait (vmcnt(0)) drains
//     every request in flight.  Lane geometry that is needed once per chunk / tile is re-derived from the lane id there
//     instead of being kept (x_geom, pack_ptv), the GEMM1 fragments are a ring of three k-steps (24 registers).
// Layout notes: X image [column][k] bf16, 208-B rows (conflict-free ds_read_b128 B fragments); g image [column][channel],
// 528-B rows; wave-private 32 x 32 fp32 output patch with 128-B rows (with the 16-lane groups of ds_read_b128 a padded
// 144-B row was 2-way conflicted, the unpadded one is conflict-free for both the column writes and the row reads).
#include <type_traits>

#include "ap_common.h"

namespace ap {

namespace {

constexpr int PT_ = BLOCK_PT;            // time tile
constexpr int KC_ = 32;                  // channels per staged chunk -> 96 K rows = 6 k-steps of 16
constexpr int PS_ = 32;                  // fp32 per row of the wave-private output patch (128 B)

}  // namespace

// ---- weight images -------------------------------------------------------------------------------------------
// GEMM1: [wave C/32][chunk C/32][kstep 6][rowtile 2][lane 64][8]; wave w owns gate channels [32w, 32w+32):
// row tile 0 = tanh rows, 1 = sigmoid rows; k-step ks of a chunk = tap ks/2, channels ch*32 + (ks&1)*16 + 8h + jj.
// perm (AP_PREC_BF16_STORE): the K order inside a chunk follows the channel order of the u image's rows -- position p holds the
// chunk's channel (p with bits 2 and 3 swapped), the order of a 32 x 32 accumulator tile's registers (ap_resblock_bf16u.hip).
__global__ void pack_w1_bf16_kernel(const float *__restrict__ w1f, __bf16 *__restrict__ out, int C, int perm) {
  const int NW = C / 32, NCH = C / KC_;
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)NW * NCH * 6 * 2 * 64 * 8;
  if (idx >= total) return;
  int jj = idx & 7;
  int lane = (idx >> 3) & 63;
  int rt = (idx >> 9) & 1;
  size_t rest = idx >> 10;
  int ks = rest % 6; rest /= 6;
  int ch = rest % NCH;
  int w = rest / NCH;
  int i = lane & 31, hh = lane >> 5;
  int tap = ks >> 1;
  int pos = (ks & 1) * 16 + 8 * hh + jj;
  if (perm) pos = (pos & ~12) | ((pos & 4) << 1) | ((pos & 8) >> 1);
  int c = ch * KC_ + pos;
  int o = rt * C + 32 * w + i;
  out[idx] = (__bf16)w1f[((size_t)o * C + c) * 3 + tap];
}

// GEMM2: [wave][rowtile 2][kstep C/16][lane][8]; row tile 0 = res_conv rows of the wave's channels, 1 = skip rows.
__global__ void pack_w2_bf16_kernel(const float *__restrict__ w2f, __bf16 *__restrict__ out, int C) {
  const int NW = C / 32, NKS = C / 16;
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)NW * NKS * 2 * 64 * 8;
  if (idx >= total) return;
  int jj = idx & 7;
  int lane = (idx >> 3) & 63;
  size_t rest = idx >> 9;
  int ks = rest % NKS; rest /= NKS;
  int rt = rest & 1;
  int w = rest >> 1;
  int i = lane & 31, hh = lane >> 5;
  int k = ks * 16 + 8 * hh + jj;
  int o = rt * C + 32 * w + i;          // w2f = [res rows (C); skip rows (C)]
  out[idx] = (__bf16)w2f[(size_t)o * C + k];
}

// final conv's first 1x1: [wave S/64][rowtile 2][kstep S/16][lane 64][8]; wave w owns output rows [64w, 64w+64)
__global__ void pack_wf1_bf16_kernel(const float *__restrict__ wf1f, __bf16 *__restrict__ out, int S) {
  const int NKS = S / 16;
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)S * S) return;
  int jj = idx & 7;
  int lane = (idx >> 3) & 63;
  size_t rest = idx >> 9;
  int ks = rest % NKS; rest /= NKS;
  int rt = rest & 1;
  int w = rest >> 1;
  int k = ks * 16 + 8 * (lane >> 5) + jj;
  int o = 64 * w + 32 * rt + (lane & 31);
  out[idx] = (__bf16)wf1f[(size_t)o * S + k];
}

int launch_pack_bf16(ap_ctx *ctx, hipStream_t st) {
  const int C = ctx->C, S = ctx->S, NL = ctx->NL;
  for (int n = 0; n < NL; n++) {
    size_t n1 = (size_t)2 * C * C * 3, n2 = (size_t)(C + S) * C;
    pack_w1_bf16_kernel<<<(unsigned)((n1 + 255) / 256), 256, 0, st>>>(ctx->w1f + n * n1, (__bf16 *)ctx->w1p_bf + n * n1, C,
                                                                             ctx->cfg.precision == AP_PREC_BF16_STORE ? 1 : 0);
    pack_w2_bf16_kernel<<<(unsigned)((n2 + 255) / 256), 256, 0, st>>>(ctx->w2f + n * n2, (__bf16 *)ctx->w2p_bf + n * n2, C);
  }
  if (ctx->wf1p_bf && S % 64 == 0)
    pack_wf1_bf16_kernel<<<(unsigned)(((size_t)S * S + 255) / 256), 256, 0, st>>>(ctx->wf1f, (__bf16 *)ctx->wf1p_bf, S);
  AP_HIP(hipGetLastError());
  return 0;
}

// Instantiated: 7 staging forms (WS = 0, 1, 2, -1 for clip lengths that are a multiple of four; 1, 2, -1 ragged) x 5 block forms
// (fused, DS, DS + NOH, DS + SAVEF, DS + NOH + SAVEF) = 35 kernels, all picked in launch_resblock_bf16p.  The timing-only masks, the
// 16x16x32 GEMM1 and the operand-image chain this kernel once carried are recorded, with their results, in docs/HISTORY.md.
// RAG: clip lengths that are not a multiple of four.  Channel rows are then only 4-byte aligned (16-byte accesses at 4-byte
// aligned addresses are exact on this chip: tools/micro/unaligned_b128.hip), the clip's last column quad is partly outside
// it: staged samples are zeroed one by one (the quad's count of valid samples instead of one mask), and the epilogue stores
// of that quad are one to three dwords.
// DS (round 4, "deferred skip"): the block writes h' (fp32) and the gate output g as the bf16 image GEMM2 consumes anyway --
// [clip][sample][256 channels], 512 B per sample, lossless for the skip sum because skip_conv only ever sees bf16(g) -- and does
// NOT run the skip half of GEMM2 or its read-modify-write of `skip`.  skipgemm_bf16_kernel (ap_skipgemm_bf16.hip) adds
// sum_n W_skip,n g_n for a group of layers into `skip` in one K-concatenated GEMM.  h' is bit-identical to the fused form
// (same pass-0 code); per tile and layer the block moves 131 KB in + 131 KB + 64 KB out instead of 262 + 262 KB.
// NOH (with DS): the net's LAST layer -- its h' is never read (WaveNet.py:131-135 returns only the skip sum), so res_conv, the
// residual's re-read of h and the h' store are left out: GEMM1, the gate and the g image only.
// SAVEF (with DS; the differentiable purifier's forward pass, ap_resblock_fwd_gate_save): the gate's two derivative factors are also
// written, as an fp16 pair per (channel, sample), in the ORDER THE ACCUMULATORS HOLD THEM -- [clip][tile][wave 8][column tile 4][q 4][lane 64]
// x 16 bytes (128 KB per tile): one 16-byte store per lane and (column tile, q), 1 KB contiguous per wave; the backward's gate kernel has
// the same wave / lane / register geometry and reads them back the same way (ap_resblock_bwd_bf16.hip).  h' and the g image are
// bit-identical to the launch without it.
template <int WS, bool RAG, bool DS = false, bool NOH = false, bool SAVEF = false>   // WS >= 0: window staging (d <= 32); WS = d mod 4 as far as the code needs it: 0, 1 (d = 1), 2 (d = 2)
__global__ __launch_bounds__(512, 2) void resblock_bf16p_kernel(
    const float *__restrict__ hin, const float *__restrict__ pt, float *__restrict__ hout, float *__restrict__ skip,
    const void *__restrict__ wbase, unsigned wbytes, unsigned w1_off, unsigned w2_off,        // bf16 weight images (one slab)
    const void *__restrict__ bbase, unsigned bbytes, unsigned b1_off, unsigned b2_off,        // fp32 bias vectors (one slab)
    int L, int d, int accumulate, int ntiles, int nblk,
    void *__restrict__ fout,                                                                    // SAVEF: the gate's derivative factors
    void *__restrict__ gout) {                                                                  // DS: this layer's g image [clip][L][256] bf16 (last: next to nblk
                                                                                                // its kernarg load is merged with nblk's and the prologue's SGPRs renumbered)
  constexpr int C = 256, NW = 8, NCH = C / KC_, NKS = C / 16;
  static_assert(!SAVEF || DS, "SAVEF: a form of the deferred-skip block");
  static_assert(!NOH || DS, "NOH: a form of the deferred-skip block");
  // cache policy: nt (aux bit 1) on the once-touched streams (the running skip rows in, both outputs out) and on the residual's
  // re-read of h (it hits what is still there and allocates nothing on a miss).  Only the tap loads and the weights allocate in
  // the XCD's L2, so h rows stay until the neighbouring tiles' taps and the residual have read them again: L2-miss reads 27.2 ->
  // 19.4 GB per 512-clip launch (traffic 1.31 -> 1.08 x algorithmic), -3 % time.
  constexpr int NT = 2;
  constexpr bool WIN = WS >= 0;
  constexpr int XBYTES = (PT_ + (WIN ? 4 : 0)) * BF_XS * 2;     // 26,624 B per X buffer (WIN: + a scratch column quad), two buffers
  constexpr int GOFF = 2 * XBYTES;
  constexpr int POFF = GOFF + PT_ * BF_GS * 2;                   // output patches: 8 waves x 32 x 32 fp32
  constexpr int PTOFF = POFF + NW * 32 * PS_ * 4;              // part_t (C floats)
  constexpr int BOFF = PTOFF + C * 4;                          // b1 (2C floats: filter | gate rows), b2 (2C: res | skip rows)
  constexpr int LDS_BYTES = BOFF + 4 * C * 4;
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, hh = lane >> 5;

  // ---- tile walk: workgroups g, g+8, g+16, ... share an XCD (round-robin dispatch); each XCD takes a contiguous run of
  // (clip, tile) work and its workgroups interleave inside that run, so at any moment the CUs of an XCD hold neighbouring
  // tiles of one clip and the +-d taps / the residual patch are re-read from that XCD's L2.  Placement only affects speed.
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

  const unsigned clip_bytes = (unsigned)C * (unsigned)L * 4u;
  auto clip_rsrc = [&](const float *base, int b) {
    const uint64_t hb = (uint64_t)(base + (size_t)b * C * L);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)hb);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(hb >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), 0, (int)clip_bytes, 0x00020000);
  };

  // ---- X staging geometry (fixed per thread): (tap = wave/2, column quad cg, channel octet oct); lane bits (low to high)
  // cg&3, oct, cg>>2 so a load covers whole 64-B runs per channel row.  Waves 6, 7 repeat tap 2.
  const int xtap = min(wave >> 1, 2);
  const int cg = ((wave & 1) * 4 + (lane >> 4)) * 4 + (lane & 3), oct = (lane >> 2) & 3;
  const int xcol = 4 * cg, xk = (xtap * KC_ + oct * 8) ^ ((__builtin_popcount(cg & 7) & 1) << 4);   // ^: the X image's 32-byte swizzle (below)

  if (tid < C) reinterpret_cast<float *>(lds + PTOFF)[tid] = pt[tid];
  // the bias vectors live in LDS for the whole kernel: fetched per tile from memory they sat behind the previous tile's
  // stores in the in-order vmcnt queue, kept in registers they spilled
  {
    const unsigned char *bb = static_cast<const unsigned char *>(bbase);
    reinterpret_cast<float *>(lds + BOFF)[tid] = reinterpret_cast<const float *>(bb + b1_off)[tid];
    reinterpret_cast<float *>(lds + BOFF)[2 * C + tid] = reinterpret_cast<const float *>(bb + b2_off)[tid];
  }

  float xr[32];
  // walk order inside a clip: for d >= 2 tiles the +-d taps of a tile are the centre columns of tiles s = d / PT_ away, and the
  // 32 tiles an XCD holds at a time are 32 consecutive walk positions.  Position p -> tile r + k s (residue classes r = 0..s-1
  // in turn, s capped at 16), so that a window of 32 positions holds whole runs ..., j - s, j, j + s, ...: L2-miss reads of
  // the d = 1024 / 2048 layers 28.5 / 31.9 -> see profiles/r2_bf16_fetch_by_layer.txt.  Placement only: results unchanged.
  const int wstep = __builtin_amdgcn_readfirstlane(min(max(d / PT_, 1), 16));
  const int wq = ntiles / wstep, wrem = ntiles % wstep;
  auto tile_bt = [&](int tile, int &b, int &t0) {
    b = __builtin_amdgcn_readfirstlane(tile / ntiles);
    int p = tile % ntiles;
    if (wstep > 1) {
      const int cut = wrem * (wq + 1);
      const int r = p < cut ? p / (wq + 1) : wrem + (p - cut) / wq;
      const int k = p < cut ? p % (wq + 1) : (p - cut) % wq;
      p = r + k * wstep;
    }
    t0 = __builtin_amdgcn_readfirstlane(p * PT_);
  };
  // zero padding (WaveNet.py:26-27) as an AND mask on the packed values: a column quad is inside the clip or outside it as a
  // whole (L % 4 == 0), the address is clamped.
  // WIN (d <= 32): the three taps of a tile are the same 128 + 2d columns, so a chunk stages ONE window of 192 columns
  // [t0 - 32, t0 + 160) -- 24.6 KB of loads instead of 64 KB -- converts every value once and writes it to the up to three
  // (column, tap) places of the X image it belongs to (ds_write_b64: four channels of one column).  A staging unit is
  // (column quad sq of 48, channel quad wc4 of 8): waves 0-5, lane bits (low to high) wc4, sq & 7, so a load covers eight
  // channel rows x 128 B and the sixteen lanes of a ds_write_b64 group cover all 32 banks.  The four samples of a unit land,
  // per tap, in one image quad (d % 4 == 0) or in two neighbouring ones (d = 1, 2): one address register per (tap, quad),
  // the sample's place inside the quad is an immediate.  A quad outside columns 0..127 is the scratch quad 128..131.
  struct Keep { unsigned m[1]; };
  Keep keep;
  const int sq = min(wave, 5) * 8 + (lane >> 3), wc4 = lane & 7;
  unsigned xwb[WIN ? 3 : 1][WIN ? 2 : 1];                      // [tap][first / second image quad of the unit's samples]
  auto calc_xwb = [&](int sq_, int wc4_) {                     // (a lambda with by-value arguments: written inline, the prologue's VALU order changes)
    if constexpr (WIN) {
#pragma unroll
      for (int T = 0; T < 3; T++) {
        const int qa = sq_ - 8 + ((T == 2 && WS != 0) ? -1 : 0) - (WS == 0 ? (T - 1) * (d >> 2) : 0);   // image quad of sample 0
#pragma unroll
        for (int h2 = 0; h2 < 2; h2++) {
          const int q = qa + h2;
          const int qc = (q >= 0 && q < PT_ / 4) ? q : PT_ / 4;
          xwb[T][h2] = (unsigned)(4 * qc * (BF_XS * 2) + ((T * 2 * KC_ + wc4_ * 8) ^ ((__builtin_popcount(qc & 7) & 1) << 5)));
        }
      }
    }
  };
  calc_xwb(sq, wc4);
  auto x_geom = [&](int t0, unsigned &voff, Keep &k) {
    // the lane's geometry is re-derived from a lane id read here (volatile asm: not hoisted out of the tile loop): kept from
    // the prologue it was spilled, and a scratch reload waits with vmcnt(0) -- here, behind the first epilogue's stores
    int ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    if constexpr (WIN) {
      const int tq = t0 - 32 + 4 * (min(wave, 5) * 8 + (ln >> 3));
      if constexpr (RAG) {                                       // (tq < 0: the whole quad is outside -- tile starts and the window's
        k.m[0] = tq >= 0 ? (unsigned)min(max(L - tq, 0), 4) : 0u;     //  left edge are multiples of four)
        voff = ((unsigned)min(max(tq, 0), L - 1) + (unsigned)((ln & 7) * 4) * (unsigned)L) * 4u;
      } else {
        k.m[0] = (tq >= 0 && tq < L) ? 0xffffffffu : 0u;
        voff = ((unsigned)min(max(tq, 0), L - 4) + (unsigned)((ln & 7) * 4) * (unsigned)L) * 4u;
      }
    } else {
      const int cg = ((wave & 1) * 4 + (ln >> 4)) * 4 + (ln & 3), oct = (ln >> 2) & 3;
      const int tp = t0 + 4 * cg + (xtap - 1) * d;
      if constexpr (RAG) {
        k.m[0] = tp >= 0 ? (unsigned)min(max(L - tp, 0), 4) : 0u;
        voff = ((unsigned)min(max(tp, 0), L - 1) + (unsigned)(oct * 8) * (unsigned)L) * 4u;
      } else {
        k.m[0] = (tp >= 0 && tp < L) ? 0xffffffffu : 0u;
        voff = ((unsigned)min(max(tp, 0), L - 4) + (unsigned)(oct * 8) * (unsigned)L) * 4u;
      }
    }
  };
  (void)clip_rsrc(hin, 0);                                       // (unused; kept: without it the prologue's scalar instructions come out in another order)
  auto issue_x1 = [&](const __amdgpu_buffer_rsrc_t &rs, unsigned voff, int ch, int e) {          // channel e of chunk ch
    // (bit_cast the whole vector: element-wise bit_cast of the builtin's int vector is mis-folded to a splat)
    const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, (ch * KC_ + e) * L * 4, 0));
#pragma unroll
    for (int i = 0; i < 4; i++) xr[e * 4 + i] = v[i];
  };
  auto issue_x = [&](const __amdgpu_buffer_rsrc_t &rs, unsigned voff, int ch) {
    if constexpr (WIN) {
      if (wave < 6) {                                            // wave-uniform
#pragma unroll
        for (int e = 0; e < 4; e++) issue_x1(rs, voff, ch, e);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++) issue_x1(rs, voff, ch, e);
    }
  };
  float ptv8[8];
  u32x4 pkq;
  auto pack_ptv = [&](int ch) {
    int ln;                                                     // (lane id read here, not kept: see x_geom)
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    if constexpr (WIN) {
      const float4 p0 = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(lds + PTOFF) + (ln & 7) * 4 + ch * KC_);
      ptv8[0] = p0.x; ptv8[1] = p0.y; ptv8[2] = p0.z; ptv8[3] = p0.w;
    } else {
      const float *ptc = reinterpret_cast<const float *>(lds + PTOFF) + ((ln >> 2) & 3) * 8 + ch * KC_;
      const float4 p0 = *reinterpret_cast<const float4 *>(ptc);
      const float4 p1 = *reinterpret_cast<const float4 *>(ptc + 4);
      ptv8[0] = p0.x; ptv8[1] = p0.y; ptv8[2] = p0.z; ptv8[3] = p0.w;
      ptv8[4] = p1.x; ptv8[5] = p1.y; ptv8[6] = p1.z; ptv8[7] = p1.w;
    }
  };
  // one eighth of a chunk's staging.  FiLM add (WaveNet.py:84), zero padding (:26-27) as an AND with the in-range mask.
  //   !WIN: sample i, channel pairs 2hf, 2hf+1 -> 4 adds, 2 cvt_pk, 2 and; the ds_write_b128 follows a sample's second piece.
  //   WIN:  sample i: piece 0 = 4 adds, 2 cvt_pk, 2 and (four channels); piece 1 = its three ds_write_b64 (taps -d, 0, +d).
  auto pack_piece = [&](unsigned char *dst, const Keep &keep, auto i_tag, auto hf_tag) {
    constexpr int i = decltype(i_tag)::value, hf = decltype(hf_tag)::value;
    // RAG: keep.m[0] counts the quad's valid samples -> all ones for sample i iff i < count
    const unsigned km = RAG ? (unsigned)(((int)i - (int)keep.m[0]) >> 31) : keep.m[0];
    if constexpr (WIN) {
      if (wave < 6) {                                            // wave-uniform
        if constexpr (hf == 0) {
#pragma unroll
          for (int e2 = 0; e2 < 2; e2++)
            pkq[e2] = __builtin_bit_cast(unsigned, __builtin_convertvector(
                                                       f32x2{xr[(2 * e2) * 4 + i] + ptv8[2 * e2],
                                                             xr[(2 * e2 + 1) * 4 + i] + ptv8[2 * e2 + 1]}, bf16x2)) & km;
        } else {
#pragma unroll
          for (int T = 0; T < 3; T++) {
            // place of sample 0 inside its image quad: tap -d: d mod 4; centre: 0; tap +d: (-d) mod 4
            const int a0 = WS == 0 || T == 1 ? 0 : (T == 0 ? WS : 4 - WS);
            const int pos = a0 + i;
            *reinterpret_cast<uint2 *>(dst + xwb[T][pos >> 2] + (pos & 3) * (BF_XS * 2)) = make_uint2(pkq[0], pkq[1]);
          }
        }
      }
    } else {
#pragma unroll
      for (int e2 = 2 * hf; e2 < 2 * hf + 2; e2++)
        pkq[e2] = __builtin_bit_cast(unsigned, __builtin_convertvector(
                                                   f32x2{xr[(2 * e2) * 4 + i] + ptv8[2 * e2],
                                                         xr[(2 * e2 + 1) * 4 + i] + ptv8[2 * e2 + 1]}, bf16x2)) & km;
      if constexpr (hf == 1) *reinterpret_cast<u32x4 *>(dst + ((xcol + i) * BF_XS + xk) * 2) = pkq;
    }
  };
  auto pack_all = [&](unsigned char *dst, const Keep &keep, int ch) {
    pack_ptv(ch);
    pack_piece(dst, keep, I0{}, I0{}); pack_piece(dst, keep, I0{}, I1{});
    pack_piece(dst, keep, I1{}, I0{}); pack_piece(dst, keep, I1{}, I1{});
    pack_piece(dst, keep, I2{}, I0{}); pack_piece(dst, keep, I2{}, I1{});
    pack_piece(dst, keep, I3{}, I0{}); pack_piece(dst, keep, I3{}, I1{});
  };

  // ---- weight fragment streams (this wave's 64 GEMM1 rows / 2 x 32 GEMM2 rows), L2 -> registers.  Buffer loads with the
  // fragment index in the scalar offset: one VGPR (lane * 16) addresses every fragment (64-bit per-lane pointers, one pair
  // per fragment slot, were hoisted out of the tile loop by the compiler and spilled).
  auto uni_rsrc = [&](const void *base, unsigned bytes) {
    const uint64_t hb = (uint64_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)hb);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(hb >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), 0, (int)bytes, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t wrs = uni_rsrc(wbase, wbytes);
  (void)bbytes;
  const unsigned lane16 = (unsigned)lane * 16u;
  // GEMM1 image [wave][chunk][kstep 6][rowtile 2][lane][8 bf16]: fragment f of this wave = f KB from the wave's base
  auto ld_w1 = [&](int frag) {
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, lane16, w1_off + (wave * NCH * 12 + frag) * 1024, 0));
  };
  // GEMM2 image [wave][rowtile 2][kstep 16][lane][8 bf16]; gks runs over pass 0's then pass 1's k-steps
  auto ld_w2 = [&](int gks) {
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, lane16, w2_off + (wave * 2 * NKS + gks) * 1024, 0));
  };
  // X image swizzle: columns whose bits 2..4 have odd parity keep the two 32-byte halves of every 64 bytes of k swapped
  // (k-step s of such a column sits where k-step s ^ 1 would).  A ds_write_b128 is served in groups of 8 consecutive lanes
  // = column quads cg..cg+3 x 2 octets; the 832-byte quad stride puts quads cg and cg+2 on the same banks (2-way); with
  // the swap the four quads of a group have parities 0,1,1,0 and land on four different bank octets.  The 16-lane groups
  // of ds_read_b128 ({0-3,12-15,20-27}, {4-11,16-19,28-31}: MI355X_MICROARCH.md, LDS) each hold rows of ONE parity, so the
  // reads stay the conflict-free permutation they were (a swap keyed on a single column bit made them 2-way: measured).
  // Cost: one VGPR (a base for even and one for odd k-steps).
  const int rdoff = (j * BF_XS + 8 * hh) * 2;                     // this lane's B-fragment byte offset inside an X buffer
  const int rdsw = (__builtin_popcount((j >> 2) & 7) & 1) * 32;
  const unsigned char *gb = lds + GOFF + (j * BF_GS + 8 * hh) * 2;
  float *patch = reinterpret_cast<float *>(lds + POFF) + wave * 32 * PS_;
  const float RS = 0.707106781186547524f;

  // ---- first tile: parameters and chunk-0 request
  int b_cur, t0_cur;
  tile_bt(t_first, b_cur, t0_cur);
  __amdgpu_buffer_rsrc_t hrs = clip_rsrc(hin, b_cur);
  unsigned xvoff;
  x_geom(t0_cur, xvoff, keep);
  // a tile's first X chunk and first weight fragments are requested at the END of the previous tile, ahead of that tile's
  // last stores (here for the first tile): a request issued after a store cannot be waited for without waiting for the
  // store (vmcnt retires in order)
  constexpr int RING = 3, PK = 3;                                // fragment ring depth (k-steps), k-step that carries the pack (a ring of
                                                                 // six with the pack in k-step 5 -- a chunk of lead for X -- measured +2 %)
  bf16x8 w[RING][2];                                                // GEMM1 fragment ring: k-step ks of a chunk uses w[ks % RING][row tile]
  auto tile_head = [&]() {
#pragma unroll
    for (int ks = 0; ks < RING; ks++)
#pragma unroll
      for (int rt = 0; rt < 2; rt++) w[ks][rt] = ld_w1(ks * 2 + rt);
    pack_all(lds, keep, 0);
    issue_x(hrs, xvoff, 1);                                   // chunk 1: packed in chunk 0's fourth k-step
  };
  issue_x(hrs, xvoff, 0);
  __syncthreads();                                               // part_t, biases visible
  tile_head();

#pragma unroll 1
  for (int tile = t_first; tile < t_end; tile += t_step) {
    const int t0 = t0_cur;
    const int ntile = tile + t_step;
    // ================================================ GEMM1 =========================================================
    f32x16 acc[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const f32x4 bv4 = *reinterpret_cast<const f32x4 *>(lds + BOFF + (rt * C + 32 * wave + 8 * q + 4 * hh) * 4);
#pragma unroll
        for (int ct = 0; ct < 4; ct++) {                        // (128 v_mov per wave and tile: entering the bias as the C operand of
          acc[rt][ct][4 * q + 0] = bv4[0];                      //  each tile's first MFMA instead measured the same -- hidden work)
          acc[rt][ct][4 * q + 1] = bv4[1];
          acc[rt][ct][4 * q + 2] = bv4[2];
          acc[rt][ct][4 * q + 3] = bv4[3];
        }
      }
    __syncthreads();

    auto mf = [&](const bf16x8 &a, const bf16x8 &bq, int rt, int ct) {
      acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bq, acc[rt][ct], 0, 0, 0);
    };
    auto rdb = [&](bf16x8 &dst, const unsigned char *xbe, const unsigned char *xbo, int ct, int ks) {   // ks: k-step 0..5 of the chunk
      dst = *reinterpret_cast<const bf16x8 *>(((ks & 1) ? xbo : xbe) + (32 * ct) * (BF_XS * 2) + ks * 32);
    };
    float pre[4][16];
    unsigned evoff[4];                                          // E4 mapping: lane = (row lane>>3 (+8 per step), column quad lane&7)
    auto calc_evoff = [&]() {                                   // called after GEMM1 (t0 made opaque there: computed before the
      int t0o = t0;                                             // chunk loop the four offsets sat in registers through GEMM1)
      asm volatile("" : "+s"(t0o));
#pragma unroll
      for (int ct = 0; ct < 4; ct++) {
        const int t = t0o + 32 * ct + 4 * (lane & 7);
        evoff[ct] = t < L ? ((unsigned)(32 * wave + (lane >> 3)) * (unsigned)L + (unsigned)t) * 4u : 0x80000000u;
      }                                                         // 0x80000000: outside the clip -> loads 0, store dropped
    };
    auto load_pre = [&](const __amdgpu_buffer_rsrc_t &rs, auto ct_tag) {
      constexpr int ct = decltype(ct_tag)::value;
#pragma unroll
      for (int p = 0; p < 4; p++) {
        const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, evoff[ct], 8 * p * L * 4, NT));
#pragma unroll
        for (int i = 0; i < 4; i++) pre[ct][4 * p + i] = v[i];
      }
    };
    // One chunk = six k-steps of eight MFMAs in explicit order (pinned with sched_barrier): column-tile-major pairs share one
    // B fragment, which is re-read for the next k-step right after its pair.  Global requests of a chunk and wave:
    //   * a k-step's two weight fragments are replaced right behind their last MFMA by those of the k-step three on (a ring
    //     of three k-steps, 24 registers: two k-steps = 16 MFMAs of lead, as the two half-chunk sets had at their tightest);
    //   * k-step 3: FiLM add / bf16 pack / ds_write of the next chunk (eight pieces, one per MFMA gap);
    //   * behind the last MFMA: the X rows of the chunk after next (the staging registers are free from the pack on, but
    //     every weight request issued before the next pack has to be OLDER than the X request -- vmcnt retires in order, so
    //     a wait for a younger fragment would be a wait for the X rows).
    // No spilled value may be reloaded inside the tile loop: a scratch reload is a vector-memory load, its wait is
    // s_waitcnt vmcnt(0), and that drains every request in flight (the round's earlier builds had one per chunk).
    // The two waves of a SIMD: the older one (waves 0-3) wins every issue conflict and reached the chunk barrier ~1.2 k cycles
    // ahead of the younger one, which then finished alone with its stalls exposed (profiles/r2_bf16_phase_trace.txt): the
    // younger wave gets the priority in k-steps 0-2, the older one (by age) in 3-5.
    auto chunk = [&](const unsigned char *xbe, const unsigned char *xbo, int ch, unsigned char *pdst, auto kind_tag) {
      constexpr int KIND = decltype(kind_tag)::value;            // 0: chunks 0..NCH-3, 1: NCH-2 (no X request), 2: NCH-1
      constexpr bool LAST = KIND == 2, WITH_X = KIND == 0;
      bf16x8 bv[4];
#pragma unroll
      for (int ct = 0; ct < 4; ct++) rdb(bv[ct], xbe, xbo, ct, 0);
      if (wave >= 4) __builtin_amdgcn_s_setprio(1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ks = 0; ks < 6; ks++) {
        const bool reload = ks + RING < 6 || !LAST;                  // (ring 3) k-steps 3-5 fetch the next chunk's first three
        const int nfrag = ks + RING < 6 ? ch * 12 + (ks + RING) * 2 : (ch + 1) * 12 + (ks + RING - 6) * 2;
        if (ks == 3) __builtin_amdgcn_s_setprio(0);
        if (ks == PK) {
          if constexpr (!LAST) pack_ptv(ch + 1);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int ct = 0; ct < 4; ct++) {
          mf(w[ks % RING][0], bv[ct], 0, ct);
          if constexpr (!LAST) {
            if (ks == PK && ct == 0) pack_piece(pdst, keep, I0{}, I0{});
            if (ks == PK && ct == 1) pack_piece(pdst, keep, I1{}, I0{});
            if (ks == PK && ct == 2) pack_piece(pdst, keep, I2{}, I0{});
            if (ks == PK && ct == 3) pack_piece(pdst, keep, I3{}, I0{});
          }
          if (ct == 3 && reload) w[ks % RING][0] = ld_w1(nfrag);
          __builtin_amdgcn_sched_barrier(0);
          mf(w[ks % RING][1], bv[ct], 1, ct);
          if (ks < 5) rdb(bv[ct], xbe, xbo, ct, ks + 1);
          if constexpr (!LAST) {
            if (ks == PK && ct == 0) pack_piece(pdst, keep, I0{}, I1{});
            if (ks == PK && ct == 1) pack_piece(pdst, keep, I1{}, I1{});
            if (ks == PK && ct == 2) pack_piece(pdst, keep, I2{}, I1{});
            if (ks == PK && ct == 3) pack_piece(pdst, keep, I3{}, I1{});
          }
          if (ct == 3 && reload) w[ks % RING][1] = ld_w1(nfrag + 1);
          if constexpr (WITH_X) {
            if (ks == 5 && ct == 3) issue_x(hrs, xvoff, ch + 2);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    };

#pragma unroll 1
    for (int ch = 0; ch < NCH - 2; ch++) {
      const unsigned char *xbe = lds + (ch & 1) * XBYTES + rdoff + rdsw, *xbo = xbe - 2 * rdsw;
      chunk(xbe, xbo, ch, lds + ((ch + 1) & 1) * XBYTES, I0{});
      __syncthreads();
    }
    {
      const unsigned char *xbe = lds + ((NCH - 2) & 1) * XBYTES + rdoff + rdsw, *xbo = xbe - 2 * rdsw;
      chunk(xbe, xbo, NCH - 2, lds + ((NCH - 1) & 1) * XBYTES, I1{});
      __syncthreads();
    }
    {
      const unsigned char *xbe = lds + ((NCH - 1) & 1) * XBYTES + rdoff + rdsw, *xbo = xbe - 2 * rdsw;
      chunk(xbe, xbo, NCH - 1, nullptr, I2{});
    }

    // ================================================ gate ==========================================================
    // GEMM2's first requests go out ahead of the gate: the CU's memory pipe serves in order and vmcnt retires in order.
    bf16x8 p0[4], p1[4];
    auto load_a4 = [&](bf16x8(&a)[4], int gks) {                 // gks = k-step over both passes, clamped to the last set
      const int g0 = gks <= 2 * NKS - 4 ? gks : 2 * NKS - 4;
#pragma unroll
      for (int s = 0; s < 4; s++) a[s] = ld_w2(g0 + s);
    };
    float4 bias[4];
    auto fetch_bias = [&](auto pass_tag) {
      constexpr int pass = decltype(pass_tag)::value;
      int ln;                                                    // (lane id read here, not kept: see x_geom)
      asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
      const int hh = ln >> 5;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int c = 32 * wave + 8 * q + 4 * hh;
        const f32x4 v4 = *reinterpret_cast<const f32x4 *>(lds + BOFF + (2 * C + pass * C + 32 * wave + 8 * q + 4 * hh) * 4);
        float4 v = make_float4(v4[0], v4[1], v4[2], v4[3]);
        if (pass == 0) {                                         // u = h + part_t re-enters the residual (alias semantics)
          const float4 pv = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(lds + PTOFF) + c);
          v.x += pv.x; v.y += pv.y; v.z += pv.z; v.w += pv.w;
        }
        bias[q] = v;
      }
    };
    if constexpr (!NOH) {
      calc_evoff();
      load_a4(p0, 0);
      load_pre(hrs, I0{});                                       // the residual's h patch, first half (what fits beside the accumulators)
      load_pre(hrs, I1{});
    }
    __builtin_amdgcn_sched_barrier(0);

    const __amdgpu_buffer_rsrc_t srs = clip_rsrc(skip, b_cur);
    const __amdgpu_buffer_rsrc_t ors = clip_rsrc(hout, b_cur);
    float pre1[4][16];                                           // the running skip rows pass 1 adds into
    auto load_pre1 = [&](auto ct_tag) {
      constexpr int ct = decltype(ct_tag)::value;
      if (!accumulate) {
#pragma unroll
        for (int r = 0; r < 16; r++) pre1[ct][r] = 0.f;
      } else {
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srs, evoff[ct], 8 * p * L * 4, NT));
#pragma unroll
          for (int i = 0; i < 4; i++) pre1[ct][4 * p + i] = v[i];
        }
      }
    };
    auto gate_ct = [&](auto ct_tag) {
      constexpr int ct = decltype(ct_tag)::value;
      int ln;                                                    // (lane id read here, not kept: see x_geom)
      asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
      const int j = ln & 31, hh = ln >> 5;
#pragma unroll
      for (int qq = 0; qq < 4; qq++) {
        unsigned pk[2];
        u32x4 fq;
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          const f32x2 a2 = {acc[0][ct][4 * qq + e], acc[0][ct][4 * qq + e + 1]};
          const f32x2 b2 = {acc[1][ct][4 * qq + e], acc[1][ct][4 * qq + e + 1]};
          f32x2 g2;
          if constexpr (SAVEF) {
            typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
            f32x2 f1, f2;
            g2 = gate_fast2_save(a2, b2, f1, f2);
            fq[e] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{f1[0], f2[0]}, f16x2));       // (tanh factor, sigmoid factor) of element e
            fq[e + 1] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{f1[1], f2[1]}, f16x2));
          } else {
            g2 = gate_fast2(a2, b2);
          }
          pk[e >> 1] = __builtin_bit_cast(unsigned, __builtin_convertvector(g2, bf16x2));
        }
        *reinterpret_cast<uint2 *>(lds + GOFF + ((32 * ct + j) * BF_GS + 32 * wave + 8 * qq + 4 * hh) * 2) = make_uint2(pk[0], pk[1]);
        if constexpr (SAVEF) {
          const uint64_t fb = (uint64_t)fout + (uint64_t)b_cur * ((uint64_t)ntiles * 131072u);
          const uint32_t flo = __builtin_amdgcn_readfirstlane((uint32_t)fb), fhi = __builtin_amdgcn_readfirstlane((uint32_t)(fb >> 32));
          const __amdgpu_buffer_rsrc_t frs =
              __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)fhi << 32) | flo), 0, (int)((unsigned)ntiles * 131072u), 0x00020000);
          // (the whole offset in the VGPR, soffset = 0: a >8-byte buffer store with an SGPR soffset reads its data late and the compiler
          //  does not guard the next write of those VGPRs -- the torn lanes of round 1, seen again here in the window-staging instantiations)
          __builtin_amdgcn_raw_buffer_store_b128(fq, frs, (unsigned)ln * 16u + (unsigned)((((t0 / PT_) * 8 + wave) * 16 + ct * 4 + qq) * 1024), 0, NT);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    // every gated column tile frees 32 accumulator registers: the rest of the h patch, then the first half of the skip rows
    gate_ct(I0{});
    if constexpr (!NOH) load_pre(hrs, I2{});
    __builtin_amdgcn_sched_barrier(0);
    gate_ct(I1{});
    if constexpr (!NOH) load_pre(hrs, I3{});
    __builtin_amdgcn_sched_barrier(0);
    gate_ct(I2{});
    if constexpr (!DS) load_pre1(I0{});
    __builtin_amdgcn_sched_barrier(0);
    gate_ct(I3{});
    if constexpr (!DS) load_pre1(I1{});
    if constexpr (!NOH) {
      fetch_bias(I0{});
      load_a4(p1, 4);
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();

    // ================================================ GEMM2 =========================================================
    // two passes of 32 rows x 128 columns: pass 0 = res_conv rows -> h', pass 1 = skip_conv rows -> skip (WaveNet.py:93-97,:133)
    auto gemm2_loop = [&](f32x16(&ac)[4], int pass) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const float4 v = bias[q];
#pragma unroll
        for (int ct = 0; ct < 4; ct++) {
          ac[ct][4 * q + 0] = v.x;
          ac[ct][4 * q + 1] = v.y;
          ac[ct][4 * q + 2] = v.z;
          ac[ct][4 * q + 3] = v.w;
        }
      }
      // B fragments (g image) are read one k-step ahead into the other of two register sets: the LDS latency of a k-step's
      // four reads hides behind the previous k-step's four MFMAs (read just before use it was exposed 32 times per tile)
      bf16x8 ba[4], bb[4];
      auto rdg = [&](bf16x8(&bq)[4], int ks) {
#pragma unroll
        for (int ct = 0; ct < 4; ct++) bq[ct] = *reinterpret_cast<const bf16x8 *>(gb + (32 * ct) * (BF_GS * 2) + (ks & (NKS - 1)) * 32);
      };
      auto step = [&](const bf16x8 &a, const bf16x8(&use)[4], bf16x8(&nxt)[4], int ks) {
        rdg(nxt, ks + 1);
#pragma unroll
        for (int ct = 0; ct < 4; ct++) {
          ac[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, use[ct], ac[ct], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      };
      rdg(ba, 0);
#pragma unroll 1
      for (int ks = 0; ks < NKS; ks += 8) {
        step(p0[0], ba, bb, ks + 0); step(p0[1], bb, ba, ks + 1); step(p0[2], ba, bb, ks + 2); step(p0[3], bb, ba, ks + 3);
        if (!DS || ks + 8 < NKS) load_a4(p0, pass * NKS + ks + 8);      // (DS: one pass -- nothing to prefetch past its last k-steps)
        __builtin_amdgcn_sched_barrier(0);
        step(p1[0], ba, bb, ks + 4); step(p1[1], bb, ba, ks + 5); step(p1[2], ba, bb, ks + 6); step(p1[3], bb, ba, ks + 7);
        if (!DS || ks + 12 < NKS) load_a4(p1, pass * NKS + ks + 12);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    // epilogue of a pass: MFMA layout (4 rows x 1 column per lane) -> wave-private LDS patch -> 1 row x 4 columns per lane,
    // so the stores (like the operand loads) are 16 B per lane
    auto epilogue = [&](const f32x16(&ac)[4], const float(&add)[4][16], const __amdgpu_buffer_rsrc_t &dst, float scale,
                        auto first_tag) {
#pragma unroll
      for (int ct = 0; ct < 4; ct++) {
        if constexpr (decltype(first_tag)::value && !DS) {      // pass 0: the h-patch registers of tiles 0, 1 are free again
          if (ct == 2) load_pre1(I2{});
          if (ct == 3) load_pre1(I3{});
        }
#pragma unroll
        for (int r = 0; r < 16; r++) patch[rowoff(r, hh) * PS_ + j] = ac[ct][r];
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const float4 v = *reinterpret_cast<const float4 *>(patch + ((lane >> 3) + 8 * p) * PS_ + 4 * (lane & 7));
          f32x4 o;
          o[0] = (add[ct][4 * p + 0] + v.x) * scale;
          o[1] = (add[ct][4 * p + 1] + v.y) * scale;
          o[2] = (add[ct][4 * p + 2] + v.z) * scale;
          o[3] = (add[ct][4 * p + 3] + v.w) * scale;
          // row step in the VGPR offset, soffset = 0: a >8-byte buffer store with an SGPR soffset reads its data late and
          // the compiler does not guard the next write of those VGPRs (observed in round 1: torn lanes)
          if constexpr (RAG) {
            const int nv = L - (t0 + 32 * ct + 4 * (lane & 7));  // valid samples of this lane's column quad (>= 4: all)
            const unsigned so = evoff[ct] + (unsigned)(8 * p * L * 4);
            const u32x4 ou = __builtin_bit_cast(u32x4, o);       // (whole-vector bit_cast: element-wise it is mis-folded to a splat)
            if (nv >= 4) __builtin_amdgcn_raw_buffer_store_b128(ou, dst, so, 0, NT);
            else {
              if (nv >= 1) __builtin_amdgcn_raw_buffer_store_b32(ou[0], dst, so, 0, NT);
              if (nv >= 2) __builtin_amdgcn_raw_buffer_store_b32(ou[1], dst, so + 4u, 0, NT);
              if (nv >= 3) __builtin_amdgcn_raw_buffer_store_b32(ou[2], dst, so + 8u, 0, NT);
            }
          } else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), dst, evoff[ct] + (unsigned)(8 * p * L * 4), 0, NT);
        }
      }
    };

    if constexpr (!DS) {
      f32x16 ac[4];
      gemm2_loop(ac, 0);
      fetch_bias(I1{});                                          // ahead of this pass's stores
      __builtin_amdgcn_sched_barrier(0);
      epilogue(ac, pre, ors, RS, std::true_type{});
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- next tile: parameters, and its first X chunk requested BEFORE the last stores of this tile
    int b_nxt = b_cur, t0_nxt = t0_cur;
    if (ntile < t_end) tile_bt(ntile, b_nxt, t0_nxt);
    // (unconditional from here: after its last tile a workgroup re-requests that tile's first chunk and drops it -- a
    // conditional request would keep the staging and fragment registers live across the whole tile)
    hrs = clip_rsrc(hin, b_nxt);
    x_geom(t0_nxt, xvoff, keep);
    issue_x(hrs, xvoff, 0);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (DS) {
      // the ONE pass of this form (res_conv rows -> h'), in the place and with the request order the fused form gives its
      // last pass: the next tile's first chunk is in flight under the MFMAs, its pack and first fragments go out before the
      // stores, the stores drain behind the next tile's GEMM1
      if constexpr (NOH) {
        tile_head();
        __builtin_amdgcn_sched_barrier(0);
      } else {
        f32x16 ac[4];
        gemm2_loop(ac, 0);
        tile_head();
        __builtin_amdgcn_sched_barrier(0);
        epilogue(ac, pre, ors, RS, std::false_type{});
      }
      // g image -> HBM: 128 columns x 512 B, one 16-byte piece per lane and step (a wave moves two whole columns per step:
      // 1 KB contiguous on both sides; the padded 528-B LDS rows keep the 16-lane groups of ds_read_b128 on distinct banks)
      {
        int ln;                                                  // (lane id read here, not kept: see x_geom)
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
        const uint64_t gb_ = (uint64_t)gout + (uint64_t)b_cur * ((uint64_t)L * 512u);
        const uint32_t glo = __builtin_amdgcn_readfirstlane((uint32_t)gb_);
        const uint32_t ghi = __builtin_amdgcn_readfirstlane((uint32_t)(gb_ >> 32));
        const __amdgpu_buffer_rsrc_t grs =
            __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)ghi << 32) | glo), 0, (int)((unsigned)L * 512u), 0x00020000);
        const int colw = 2 * wave + (ln >> 5), q = ln & 31;
        const unsigned char *src = lds + GOFF + colw * (BF_GS * 2) + q * 16;
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const u32x4 v = *reinterpret_cast<const u32x4 *>(src + 16 * i * (BF_GS * 2));
          const int t = t0 + colw + 16 * i;
          const unsigned off = t < L ? (unsigned)t * 512u + (unsigned)q * 16u : 0x80000000u;   // outside the clip: dropped
          __builtin_amdgcn_raw_buffer_store_b128(v, grs, off, 0, NT);
        }
      }
    } else {
      f32x16 ac[4];
      gemm2_loop(ac, 1);
      // no barrier here: the X buffers have been free since the gate's barrier, the g image is next written by the next
      // tile's gate (eight barriers on), and the epilogue only touches this wave's own patch
      tile_head();
      __builtin_amdgcn_sched_barrier(0);
      epilogue(ac, pre1, srs, 1.0f, std::false_type{});
    }
    b_cur = b_nxt;
    t0_cur = t0_nxt;
  }
}

// BLOCK_BF16_P: one launch of the planned staging form (WS, RAG) and block form: DS = the deferred-skip form (skip and accumulate unused),
// + NOH (the net's last layer), + SAVEF (the differentiable purifier's forward).  One workgroup per CU.
int launch_block_bf16p(ap_ctx *ctx, const BlockPlan &p, int layer, const float *hin, const float *pt, float *hout, float *skip, int accumulate, int L,
                       hipStream_t st, void *gout, void *fout) {
  const BlockSlabs sl = block_slabs(ctx, layer);
  auto launch = [&](auto ws_tag, auto rag_tag) {
    constexpr int W = decltype(ws_tag)::value;
    constexpr bool R = decltype(rag_tag)::value;
    auto go = [&](auto *kernel) {
      kernel<<<p.grid, p.wg, 0, st>>>(hin, pt, hout, p.ds ? nullptr : skip, sl.wlo, sl.wbytes, sl.w1_off, sl.w2_off, sl.blo, sl.bbytes, sl.b1_off, sl.b2_off,
                                      L, p.d, p.ds ? 0 : accumulate, p.ntiles, (int)p.nblk, fout, gout);
    };
    if (!p.ds) go(resblock_bf16p_kernel<W, R>);
    else if (p.savef && !p.noh) go(resblock_bf16p_kernel<W, R, true, false, true>);
    else if (p.savef) go(resblock_bf16p_kernel<W, R, true, true, true>);
    else if (!p.noh) go(resblock_bf16p_kernel<W, R, true>);
    else go(resblock_bf16p_kernel<W, R, true, true>);
  };
  using std::integral_constant;
  if (p.rag) {                                                   // (ragged: no one-window form at d = 4 .. 32)
    if (p.ws == 1) launch(integral_constant<int, 1>{}, std::true_type{});
    else if (p.ws == 2) launch(integral_constant<int, 2>{}, std::true_type{});
    else launch(integral_constant<int, -1>{}, std::true_type{});
  } else if (p.ws == 0) launch(integral_constant<int, 0>{}, std::false_type{});
  else if (p.ws == 1) launch(integral_constant<int, 1>{}, std::false_type{});
  else if (p.ws == 2) launch(integral_constant<int, 2>{}, std::false_type{});
  else launch(integral_constant<int, -1>{}, std::false_type{});
  AP_HIP(hipGetLastError());
  return 0;
}

}  // namespace ap
