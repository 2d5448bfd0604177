// 2-D ConvNet classifier kernels (audio_models/ConvNets_SpeechCommands/models/*, fed by the
// mel front-end): conv-as-GEMM on the exact-fp32 MFMA, plus the small NCHW kernels a lowered network needs
// (per-channel affine = eval-mode BatchNorm, ReLU, add, pooling, channel copies for cat / slices).
//
// conv2d_f32_kernel: implicit GEMM per group,  M = Cout/g, N = B*Ho*Wo, K = (Cin/g)*kh*kw.
// Workgroup tile 64 (M) x 64 (N), 4 waves of 32x32 (v_mfma_f32_32x32x2_f32), K chunks of 16 staged in LDS
// ([k][m] weights pre-transposed at plan time, [k][n] im2col gather), register-prefetched one chunk ahead.
// Epilogue fuses the folded-BN bias, an optional residual tensor and ReLU.
#include "ap_common.h"
#include "ap_conv_plan.h"

namespace ap {

constexpr int CBM = 64, CBN = 64, CBK = 16;

struct ConvArgs {
  const float *x, *wT, *bias, *res;
  float *out;
  int B, Cin, H, W, Cout, Ho, Wo, kh, kw, stride, pad, groups, relu;
  int pad_h, dil_h, dil_w;   // pad applies to W; pad_h / dil_h to H (equal to pad / dil_w except in 1-D mode: 0 / 1)
  int x_cstride;     // channels of the tensor x lives in (>= Cin when x is a channel slice of a wider tensor)
  int x_coff;        // first channel of the slice
  int splits;        // > 1: split-K (groups == 1): blockIdx.z = slice of the chunk range, raw partial sums go to `part`
  float *part;       // [splits][B][Cout][Ho][Wo]
  int o_cstride;     // channels of the tensor `out` lives in (ap_conv2d_fwd_slice: out is a channel slice; Cout otherwise)
  int o_coff;        // first channel of that slice (streamed-weight kernel and its split-K reduce only)
};

__global__ __launch_bounds__(256) void conv2d_f32_kernel(ConvArgs a) {
  __shared__ float As[2][CBK][CBM];
  __shared__ float Bs[2][CBK][CBN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int j = lane & 31, hh = lane >> 5;
  const int Mg = a.Cout / a.groups, Cg = a.Cin / a.groups, KK = a.kh * a.kw, Kg = Cg * KK;
  const int HoWo = a.Ho * a.Wo, N = a.B * HoWo;
  const int g = blockIdx.z, m0 = blockIdx.y * CBM, n0 = blockIdx.x * CBN;

  // B (im2col) loader: thread -> column n = tid & 63, k rows (tid >> 6) + 4 i
  const int nl = tid & 63, kq = tid >> 6;
  const int n = n0 + nl;
  const bool nvalid = n < N;
  const int bb = nvalid ? n / HoWo : 0, pp = nvalid ? n % HoWo : 0;
  const int iy0 = (pp / a.Wo) * a.stride - a.pad_h, ix0 = (pp % a.Wo) * a.stride - a.pad;
  const float *xb = a.x + ((size_t)bb * a.x_cstride + a.x_coff + (size_t)g * Cg) * a.H * a.W;
  // A loader: thread -> row m = tid & 63, k rows (tid >> 6) + 4 i ; wT is [groups][Kg][Mg]
  const float *wg = a.wT + (size_t)g * Kg * Mg;
  const bool mvalid = (m0 + nl) < Mg;

  float ar[4], br[4];
  auto load_chunk = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int k = k0 + kq + 4 * i;
      float av = 0.f, bv = 0.f;
      if (k < Kg) {
        if (mvalid) av = wg[(size_t)k * Mg + m0 + nl];
        const int ci = k / KK, r = k - ci * KK, ky = r / a.kw, kx = r - ky * a.kw;
        const int iy = iy0 + ky * a.dil_h, ix = ix0 + kx * a.dil_w;
        if (nvalid && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) bv = xb[((size_t)ci * a.H + iy) * a.W + ix];
      }
      ar[i] = av;
      br[i] = bv;
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      As[buf][kq + 4 * i][nl] = ar[i];
      Bs[buf][kq + 4 * i][nl] = br[i];
    }
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;

  const int nchunk = (Kg + CBK - 1) / CBK;
  load_chunk(0);
  store_chunk(0);
  __syncthreads();
  for (int c = 0; c < nchunk; c++) {
    if (c + 1 < nchunk) load_chunk((c + 1) * CBK);
    const int buf = c & 1;
#pragma unroll
    for (int s = 0; s < CBK / 2; s++)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[buf][2 * s + hh][32 * wm + j], Bs[buf][2 * s + hh][32 * wn + j], acc, 0,
                                                 0, 0);
    if (c + 1 < nchunk) store_chunk(buf ^ 1);
    __syncthreads();
  }

  // epilogue: lane (j, hh) holds column n0 + 32 wn + j, rows m0 + 32 wm + rowoff(r, hh)
  const int nn = n0 + 32 * wn + j;
  if (nn < N) {
    const int ob = nn / HoWo, op = nn % HoWo;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int m = m0 + 32 * wm + rowoff(r, hh);
      if (m < Mg) {
        const int co = g * Mg + m;
        const size_t off = ((size_t)ob * a.Cout + co) * HoWo + op;
        float v = acc[r];
        if (a.bias) v += a.bias[co];
        if (a.res) v += a.res[off];
        if (a.relu) v = fmaxf(v, 0.f);
        a.out[off] = v;
      }
    }
  }
}

// Cout <= 4 (the UNet's output convolution, unet.py:432-436: 128 -> 1 channels at 32 x 32): an M = 1 "GEMM" leaves 63 of the 64
// rows of an MFMA tile empty (the generic kernel ran it at 0.8 TFLOP/s).  One thread per output pixel instead, the whole
// filter in LDS ([k][m], k = ci kh kw + ky kw + kx as packed for the generic kernel), an fp32 fma chain in k order; reads are
// coalesced along W and the taps re-read L1 / L2.  Same contract as conv2d_f32_kernel (groups = 1).
// K3 (3 x 3 taps, dilation 1 -- the UNet's layer): the nine taps' offsets and validity once per thread, then nine unconditional
// loads per channel (clamped address, value selected) with four channels unrolled = 36 loads in flight; with run-time tap loops
// every load was waited for before the next was issued (0.31 ms per launch at B = 256; same fma order, same result).
template <int MO, bool K3 = false>
__global__ __launch_bounds__(256) void conv2d_few_kernel(ConvArgs a) {
  extern __shared__ float wsm[];
  const int KK = a.kh * a.kw, Kg = a.Cin * KK, HoWo = a.Ho * a.Wo, N = a.B * HoWo, HW = a.H * a.W;
  for (int i = threadIdx.x; i < Kg * MO; i += 256) wsm[i] = a.wT[i];
  __syncthreads();
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int bb = n / HoWo, pp = n % HoWo;
  const int iy0 = (pp / a.Wo) * a.stride - a.pad_h, ix0 = (pp % a.Wo) * a.stride - a.pad;
  const float *xb = a.x + ((size_t)bb * a.x_cstride + a.x_coff) * HW;
  float acc[MO];
#pragma unroll
  for (int m = 0; m < MO; m++) acc[m] = 0.f;
  if constexpr (K3) {
    int off[9];
    bool ok[9];
#pragma unroll
    for (int t = 0; t < 9; t++) {
      const int iy = iy0 + t / 3, ix = ix0 + t % 3;
      ok[t] = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      off[t] = ok[t] ? iy * a.W + ix : 0;
    }
    float v[2][9];                                             // channel ci + 1 is requested before channel ci's fma chain runs
#pragma unroll
    for (int t = 0; t < 9; t++) v[0][t] = xb[off[t]];
#pragma unroll 2
    for (int ci = 0; ci < a.Cin; ci++) {
      const float *xn = xb + (size_t)(ci + 1 < a.Cin ? ci + 1 : ci) * HW;
      const float *wk = wsm + (size_t)ci * 9 * MO;
#pragma unroll
      for (int t = 0; t < 9; t++) v[(ci + 1) & 1][t] = xn[off[t]];
#pragma unroll
      for (int t = 0; t < 9; t++) {
        const float vt = ok[t] ? v[ci & 1][t] : 0.f;
#pragma unroll
        for (int m = 0; m < MO; m++) acc[m] = fmaf(wk[t * MO + m], vt, acc[m]);
      }
    }
  } else
#pragma unroll 4                                                // (four channels' taps in flight: the loop is load-latency bound)
  for (int ci = 0; ci < a.Cin; ci++) {
    const float *xc = xb + (size_t)ci * HW;
    const float *wk = wsm + (size_t)ci * KK * MO;
    for (int ky = 0; ky < a.kh; ky++) {
      const int iy = iy0 + ky * a.dil_h;
      for (int kx = 0; kx < a.kw; kx++) {
        const int ix = ix0 + kx * a.dil_w;
        const float v = (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) ? xc[iy * a.W + ix] : 0.f;
#pragma unroll
        for (int m = 0; m < MO; m++) acc[m] = fmaf(wk[(ky * a.kw + kx) * MO + m], v, acc[m]);
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MO; m++) {
    const size_t off = ((size_t)bb * a.Cout + m) * HoWo + pp;
    float v = acc[m];
    if (a.bias) v += a.bias[m];
    if (a.res) v += a.res[off];
    if (a.relu) v = fmaxf(v, 0.f);
    a.out[off] = v;
  }
}

// 128 x 128 tile variant for wide layers (Cout/g >= 128: UNet, ResNeXt stages 2-3, VGG 128+): 4 waves x (64 x 64 =
// 2 x 2 accumulators), so each staged element feeds 4x the MFMAs of the 64 x 64 kernel, and the im2col index (ci, r)
// of every element a thread stages advances incrementally by the chunk size instead of being re-derived by division
// (kh, kw <= 3).  Same contract as conv2d_f32_kernel.
__global__ __launch_bounds__(256) void conv2d_f32_big_kernel(ConvArgs a) {
  constexpr int BM = 128, BN = 128, BK = 16;
  __shared__ float As[2][BK][BM];
  __shared__ float Bs[2][BK][BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int j = lane & 31, hh = lane >> 5;
  const int Mg = a.Cout / a.groups, Cg = a.Cin / a.groups, KK = a.kh * a.kw, Kg = Cg * KK;
  const int HoWo = a.Ho * a.Wo, N = a.B * HoWo;
  const int g = blockIdx.z, m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int nl = tid & 127, kq = tid >> 7;             // element i of a thread: k row kq + 2 i, column / row nl
  const int n = n0 + nl;
  const bool nvalid = n < N;
  const int bb = nvalid ? n / HoWo : 0, pp = nvalid ? n % HoWo : 0;
  const int iy0 = (pp / a.Wo) * a.stride - a.pad_h, ix0 = (pp % a.Wo) * a.stride - a.pad;
  const float *xb = a.x + ((size_t)bb * a.x_cstride + a.x_coff + (size_t)g * Cg) * a.H * a.W;
  const float *wg = a.wT + (size_t)g * Kg * Mg;
  const bool mvalid = (m0 + nl) < Mg;
  const int HW = a.H * a.W;
  const int dci = BK / KK, dr = BK % KK;               // (ci, r) += (dci, dr) per chunk, with carry
  int ci[8], rr[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int k = kq + 2 * i;
    ci[i] = k / KK;
    rr[i] = k % KK;
  }
  float ar[8], br[8];
  auto load_chunk = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int k = k0 + kq + 2 * i;
      float av = 0.f, bv = 0.f;
      if (k < Kg) {
        if (mvalid) av = wg[(size_t)k * Mg + m0 + nl];
        const int r = rr[i];
        const int ky = (r >= a.kw) + (r >= 2 * a.kw), kx = r - ky * a.kw;
        const int iy = iy0 + ky * a.dil_h, ix = ix0 + kx * a.dil_w;
        if (nvalid && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) bv = xb[(size_t)ci[i] * HW + iy * a.W + ix];
      }
      ar[i] = av;
      br[i] = bv;
      int r2 = rr[i] + dr, c2 = ci[i] + dci;
      if (r2 >= KK) { r2 -= KK; c2++; }
      rr[i] = r2;
      ci[i] = c2;
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      As[buf][kq + 2 * i][nl] = ar[i];
      Bs[buf][kq + 2 * i][nl] = br[i];
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int x_ = 0; x_ < 2; x_++)
#pragma unroll
    for (int y_ = 0; y_ < 2; y_++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[x_][y_][r] = 0.f;

  const int nchunk = (Kg + BK - 1) / BK;
  load_chunk(0);
  store_chunk(0);
  __syncthreads();
  for (int c = 0; c < nchunk; c++) {
    if (c + 1 < nchunk) load_chunk((c + 1) * BK);
    const int buf = c & 1;
#pragma unroll
    for (int s = 0; s < BK / 2; s++) {
      float af[2], bf[2];
#pragma unroll
      for (int t = 0; t < 2; t++) {
        af[t] = As[buf][2 * s + hh][64 * wm + 32 * t + j];
        bf[t] = Bs[buf][2 * s + hh][64 * wn + 32 * t + j];
      }
#pragma unroll
      for (int x_ = 0; x_ < 2; x_++)
#pragma unroll
        for (int y_ = 0; y_ < 2; y_++)
          acc[x_][y_] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[x_], bf[y_], acc[x_][y_], 0, 0, 0);
    }
    if (c + 1 < nchunk) store_chunk(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int y_ = 0; y_ < 2; y_++) {
    const int nn = n0 + 64 * wn + 32 * y_ + j;
    if (nn < N) {
      const int ob = nn / HoWo, op = nn % HoWo;
#pragma unroll
      for (int x_ = 0; x_ < 2; x_++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int m = m0 + 64 * wm + 32 * x_ + rowoff(r, hh);
          if (m < Mg) {
            const int co = g * Mg + m;
            const size_t off = ((size_t)ob * a.Cout + co) * HoWo + op;
            float v = acc[x_][y_][r];
            if (a.bias) v += a.bias[co];
            if (a.res) v += a.res[off];
            if (a.relu) v = fmaxf(v, 0.f);
            a.out[off] = v;
          }
        }
    }
  }
}

// 128 x 128 tiles with the weights streamed (layers with Cin/g % 16 == 0, i.e. everything past a network's stem).
// Two things bounded conv2d_f32_big_kernel at ~36 % of the MFMA peak: every K chunk each thread fetched, range-checked
// and LDS-staged 8 weights and 8 gathered activations with per-element (ci, ky, kx) bookkeeping.  Here
//  * K runs tap-major, k' = (ky kw + kx) Cg + ci, so a 16-row chunk is ONE tap over 16 consecutive channels: one
//    range check and one base address per thread per chunk, elements HW apart;
//  * the weights are pre-packed in the MFMA A-operand layout ([group][32-row tile][k'/8][lane][4]) and go L2 ->
//    registers as dwordx4, one chunk ahead: no LDS, no stores, no bank traffic for them (LDS holds only the 16 KB
//    double-buffered im2col tile, so more workgroups fit a CU).
// BUF (round 3; tensors and weight image below 2 GB each, which the host checks): every global access is a buffer load with a
// 32-bit VGPR offset computed once per chunk and the row / fragment step in the SCALAR offset, padding taps read through an
// out-of-range offset (returns 0) -- the 64-bit per-load address arithmetic and the selects of the pointer form were 2.9 VALU
// + 2 SALU instructions per MFMA, and the chip held 1.95 GHz under them against 2.38 under the fused block.
// P1 (1 x 1, stride 1, no padding, H W % 4 == 0: the attention qkv / proj convolutions, skip connections, ResNeXt's pointwise
// layers): the "gather" is a plain row of pixels, so a thread stages four consecutive pixels of a channel with ONE 16-byte
// load and one ds_write_b128 -- two loads per thread and chunk instead of eight.
template <int BM, int BN, bool BUF = true, bool P1 = false>
__global__ __launch_bounds__(256, 5) void conv2d_f32_big2_kernel(ConvArgs a, const float *__restrict__ afrag, unsigned x_bytes,
                                                                 unsigned a_bytes) {
  // 2 x 2 waves, each (BM/2 rows x BN/2 columns): BM x BN = 128 x 128, 128 x 64 (layers with few tiles), 64 x 128
  // (64 <= Cout/g < 128: ResNeXt's grouped 3x3)
  constexpr int BK = 16, NX = BM / 64, NY = BN / 64, EPT = BK * BN / 256, KSTEP = 256 / BN;
  // im2col tile: P1 keeps [k'][column] (its staging writes four pixels of one k' at once, 4-byte fragment reads); the gather form
  // keeps [column][k'] with 80-byte rows (conflict-free 16-byte writes of a thread's EPT consecutive k' and 16-byte fragment reads)
  constexpr int RS = BK + 4;
  // (at least 4 x 32 x 32 floats: the epilogue's four wave-private output patches alias it)
  constexpr int BS_FLOATS = (P1 ? 2 * BK * BN : 2 * BN * RS) > 4096 ? (P1 ? 2 * BK * BN : 2 * BN * RS) : 4096;
  __shared__ __attribute__((aligned(16))) float Bs_[BS_FLOATS];
  auto Bs = [&](int buf, int k, int col) -> float & { return Bs_[P1 ? (buf * BK + k) * BN + col : (buf * BN + col) * RS + k]; };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int j = lane & 31, hh = lane >> 5;
  const int Mg = a.Cout / a.groups, Cg = a.Cin / a.groups, KK = a.kh * a.kw, Kg = Cg * KK;
  const int HoWo = a.Ho * a.Wo, N = a.B * HoWo;
  const int g = a.splits > 1 ? 0 : blockIdx.z, zs = a.splits > 1 ? blockIdx.z : 0;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int nl = tid & (BN - 1), kq = (tid / BN) * (P1 ? 1 : EPT);   // gather form: a thread stages k' = kq .. kq + EPT - 1 of column nl
  const int n = n0 + nl;
  const bool nvalid = n < N;
  const int bb = nvalid ? n / HoWo : 0, pp = nvalid ? n % HoWo : 0;
  const int iy0 = (pp / a.Wo) * a.stride - a.pad_h, ix0 = (pp % a.Wo) * a.stride - a.pad;
  const int HW = a.H * a.W;
  const float *xb = a.x + ((size_t)bb * a.x_cstride + a.x_coff + (size_t)g * Cg + kq) * HW;
  const int MT = (Mg + 31) / 32, KQ = Kg / 8, CPT = Cg / BK;   // row tiles, k' quads per row tile, chunks per tap
  const f32x4 *af[NX];
#pragma unroll
  for (int x_ = 0; x_ < NX; x_++) {
    const int mt = min((m0 >> 5) + NX * wm + x_, MT - 1);      // a tile past the end re-reads the last one (never stored)
    af[x_] = reinterpret_cast<const f32x4 *>(afrag) + ((size_t)g * MT + mt) * KQ * 64 + lane;
  }
  const int nchunk = KK * CPT;
  float br[EPT];
  auto uni_rsrc = [&](const void *base, unsigned bytes) {
    const uint64_t hb = (uint64_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)hb);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(hb >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), 0, (int)bytes, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t xrs = uni_rsrc(a.x, BUF ? x_bytes : 0u);
  const __amdgpu_buffer_rsrc_t ars = uni_rsrc(afrag, BUF ? a_bytes : 0u);
  const unsigned xb_off = (unsigned)(((size_t)bb * a.x_cstride + a.x_coff + (size_t)g * Cg + kq) * HW);   // elements (BUF: < 2^29)
  unsigned af_off[NX];
#pragma unroll
  for (int x_ = 0; x_ < NX; x_++) {
    const int mt = min((m0 >> 5) + NX * wm + x_, MT - 1);
    af_off[x_] = (unsigned)((((size_t)g * MT + mt) * KQ * 64 + lane) * 16);
  }
  // P1 staging geometry: thread = (pixel quad nq of BN / 4, chunk row kq1 of R1 = 1024 / BN), NP1 = 16 / R1 passes
  constexpr int R1 = 1024 / BN, NP1 = BK / R1;
  f32x4 br4[P1 ? NP1 : 1];
  const int nq1 = tid % (BN / 4), kq1 = tid / (BN / 4);
  unsigned voff1 = 0x80000000u;
  if constexpr (P1) {
    const int n4 = n0 + 4 * nq1;                                // four pixels of one image (H W % 4 == 0), inside N or outside as a whole
    if (n4 < N) {
      const int b4 = n4 / HoWo, p4 = n4 - b4 * HoWo;
      voff1 = (unsigned)((((size_t)b4 * a.x_cstride + a.x_coff + (size_t)g * Cg + kq1) * HW + p4) * 4);
    }
  }
  auto load_b = [&](int c) {                                   // chunk c = (tap r, channels c0 .. c0+15)
    if constexpr (P1) {
#pragma unroll
      for (int i = 0; i < NP1; i++)
        br4[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, voff1, (c * BK + R1 * i) * HW * 4, 0));
      return;
    }
    const int r = c / CPT, c0 = (c - r * CPT) * BK;
    const int ky = r / a.kw, kx = r - ky * a.kw;
    const int iy = iy0 + ky * a.dil_h, ix = ix0 + kx * a.dil_w;
    const bool ok = nvalid && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
    if constexpr (BUF) {
      const unsigned voff = ok ? (xb_off + (unsigned)(c0 * HW + iy * a.W + ix)) * 4u : 0x80000000u;   // out of range -> 0
#pragma unroll
      for (int i = 0; i < EPT; i++)
        br[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, voff, i * HW * 4, 0));
    } else {
      const float *p = xb + (size_t)c0 * HW + (ok ? iy * a.W + ix : 0);
#pragma unroll
      for (int i = 0; i < EPT; i++) {
        const float v = p[(size_t)i * HW];
        br[i] = ok ? v : 0.f;
      }
    }
  };
  auto load_a = [&](f32x4(&aa)[NX][2], int c) {
#pragma unroll
    for (int x_ = 0; x_ < NX; x_++)
#pragma unroll
      for (int q = 0; q < 2; q++) {
        if constexpr (BUF)
          aa[x_][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ars, af_off[x_], (2 * c + q) * 1024, 0));
        else
          aa[x_][q] = af[x_][(size_t)(2 * c + q) * 64];
      }
  };
  auto store_b = [&](int buf) {
    if constexpr (P1) {
#pragma unroll
      for (int i = 0; i < NP1; i++) *reinterpret_cast<f32x4 *>(&Bs(buf, kq1 + R1 * i, 4 * nq1)) = br4[i];
      return;
    }
#pragma unroll
    for (int v = 0; v < EPT / 4; v++)
      *reinterpret_cast<f32x4 *>(&Bs(buf, kq + 4 * v, nl)) = f32x4{br[4 * v], br[4 * v + 1], br[4 * v + 2], br[4 * v + 3]};
  };
  f32x16 acc[NX][NY];
#pragma unroll
  for (int x_ = 0; x_ < NX; x_++)
#pragma unroll
    for (int y_ = 0; y_ < NY; y_++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[x_][y_][r] = 0.f;
  // step (q, e) of a chunk: k' = 8 q + 4 hh + e (the order of the fragment image)
  auto compute = [&](const f32x4(&aa)[NX][2], int buf) {
#pragma unroll
    for (int q = 0; q < BK / 8; q++) {
      if constexpr (!P1) {                                      // one column tile at a time: four operand registers live, eight MFMAs per read
#pragma unroll
        for (int y_ = 0; y_ < NY; y_++) {
          const f32x4 bq = *reinterpret_cast<const f32x4 *>(&Bs(buf, 8 * q + 4 * hh, 32 * NY * wn + 32 * y_ + j));
#pragma unroll
          for (int e = 0; e < 4; e++)
#pragma unroll
            for (int x_ = 0; x_ < NX; x_++)
              acc[x_][y_] = __builtin_amdgcn_mfma_f32_32x32x2f32(aa[x_][q][e], bq[e], acc[x_][y_], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++) {
          float bf[NY];
#pragma unroll
          for (int t = 0; t < NY; t++) bf[t] = Bs(buf, 8 * q + 4 * hh + e, 32 * NY * wn + 32 * t + j);
#pragma unroll
          for (int x_ = 0; x_ < NX; x_++)
#pragma unroll
            for (int y_ = 0; y_ < NY; y_++)
              acc[x_][y_] = __builtin_amdgcn_mfma_f32_32x32x2f32(aa[x_][q][e], bf[y_], acc[x_][y_], 0, 0, 0);
        }
      }
    }
  };

  // split-K (low-resolution layers, too few output tiles for 256 CUs): this workgroup sums chunks [cb, ce) only
  const int cb = a.splits > 1 ? (int)((long long)nchunk * zs / a.splits) : 0;
  const int ce = a.splits > 1 ? (int)((long long)nchunk * (zs + 1) / a.splits) : nchunk;
  f32x4 a0[NX][2], a1[NX][2];
  load_a(a0, cb);
  load_b(cb);
  store_b(0);
  __syncthreads();
#pragma unroll 1
  for (int c = cb; c < ce; c++) {
    const int cn = c + 1 < ce ? c + 1 : c;                      // the last trip re-fetches its own chunk (unused)
    load_b(cn);
    load_a(a1, cn);
    compute(a0, (c - cb) & 1);
    store_b((c - cb + 1) & 1);
#pragma unroll
    for (int x_ = 0; x_ < NX; x_++)
#pragma unroll
      for (int q = 0; q < 2; q++) a0[x_][q] = a1[x_][q];
    __syncthreads();
  }
  // Epilogue.  The accumulator layout is 4 rows x 1 column per lane: stored as it is, a tile costs every thread 64 four-byte stores
  // (+ 64 residual loads), as many memory instructions as ~16 chunks of the main loop -- the fixed cost that held the short-K
  // layers (128 -> 128 3x3: 72 chunks) at 0.74 of the peak while K = 2 304 reached 0.85.  Where an image's pixel count is a
  // multiple of four (every layer but the 1 x 1 maps) each 32 x 32 tile goes through a wave-private LDS patch (aliasing the
  // im2col tile, free behind the loop's last barrier) and leaves as 1 row x 4 pixels per lane: 16-byte stores and residual loads.
  if ((HoWo & 3) == 0) {
    int ln;                                                     // (lane id read here: lane-derived values kept across the chunk loop for
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));   //  the epilogue's sake were spilled)
    const int ej = ln & 31, ehh = ln >> 5, erow = ln >> 3, eq = ln & 7;
    float *patch = Bs_ + wave * 1024;                           // [32 rows][32 columns], 128-byte rows (conflict-free both ways)
    const size_t part_base = (size_t)zs * ((size_t)a.B * a.Cout * HoWo);
#pragma unroll
    for (int y_ = 0; y_ < NY; y_++) {
      const int nn = n0 + 32 * NY * wn + 32 * y_ + 4 * eq;      // this lane's pixel quad (inside N or outside it as a whole)
      const int ob = nn < N ? nn / HoWo : 0, op = nn < N ? nn - ob * HoWo : 0;
#pragma unroll
      for (int x_ = 0; x_ < NX; x_++) {
        // the tile's bias and residual operands are requested BEFORE its transposes: their latency runs under the LDS round trip
        // instead of being exposed once per 32 x 32 tile
        // (not for the first of four tiles: all 64 accumulator registers are still live there and the operands would be spilled)
        const bool early = NX * NY < 4 || x_ + y_ > 0;
        f32x4 rv[4];
        float bv[4];
        const bool fin = a.splits <= 1;
        auto fetch_operands = [&]() {
#pragma unroll
          for (int p = 0; p < 4; p++) {
            const int m = m0 + 32 * NX * wm + 32 * x_ + erow + 8 * p;
            const bool ok = nn < N && m < Mg;
            const int co = g * Mg + (ok ? m : 0);
            bv[p] = (fin && a.bias && ok) ? a.bias[co] : 0.f;
            rv[p] = (fin && a.res && ok) ? *reinterpret_cast<const f32x4 *>(a.res + ((size_t)ob * a.Cout + co) * HoWo + op) : f32x4{0.f, 0.f, 0.f, 0.f};
          }
        };
        if (early) fetch_operands();
        asm volatile("" ::: "memory");
#pragma unroll
        for (int r = 0; r < 16; r++) patch[rowoff(r, ehh) * 32 + ej] = acc[x_][y_][r];
        asm volatile("" ::: "memory");
        if (!early) fetch_operands();
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const int row = erow + 8 * p;
          const int m = m0 + 32 * NX * wm + 32 * x_ + row;
          f32x4 v = *reinterpret_cast<const f32x4 *>(patch + row * 32 + 4 * eq);
          if (nn < N && m < Mg) {
            const int co = g * Mg + m;
            const size_t off = ((size_t)ob * a.Cout + co) * HoWo + op;
            if (!fin) {                                         // raw partial sum; conv_splitk_reduce_kernel adds bias / residual / ReLU
              *reinterpret_cast<f32x4 *>(a.part + part_base + off) = v;
            } else {
              v[0] += bv[p]; v[1] += bv[p]; v[2] += bv[p]; v[3] += bv[p];          // (bias, then residual: the order of the scalar path)
              v[0] += rv[p][0]; v[1] += rv[p][1]; v[2] += rv[p][2]; v[3] += rv[p][3];
              if (a.relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
              *reinterpret_cast<f32x4 *>(a.out + ((size_t)ob * a.o_cstride + a.o_coff + co) * HoWo + op) = v;
            }
          }
        }
      }
    }
    return;
  }
#pragma unroll
  for (int y_ = 0; y_ < NY; y_++) {
    const int nn = n0 + 32 * NY * wn + 32 * y_ + j;
    if (nn < N) {
      const int ob = nn / HoWo, op = nn % HoWo;
#pragma unroll
      for (int x_ = 0; x_ < NX; x_++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int m = m0 + 32 * NX * wm + 32 * x_ + rowoff(r, hh);
          if (m < Mg) {
            const int co = g * Mg + m;
            const size_t off = ((size_t)ob * a.Cout + co) * HoWo + op;
            float v = acc[x_][y_][r];
            if (a.splits > 1) {                                 // raw partial sum; conv_splitk_reduce_kernel adds bias / residual / ReLU
              a.part[(size_t)zs * ((size_t)a.B * a.Cout * HoWo) + off] = v;
            } else {
              if (a.bias) v += a.bias[co];
              if (a.res) v += a.res[off];
              if (a.relu) v = fmaxf(v, 0.f);
              a.out[((size_t)ob * a.o_cstride + a.o_coff + co) * HoWo + op] = v;
            }
          }
        }
    }
  }
}

// out = [ReLU](sum over the K slices in slice order (deterministic) + bias + residual); four consecutive outputs per thread
__global__ void conv_splitk_reduce_kernel(ConvArgs a, size_t total) {
  const size_t i4 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i4 >= total) return;
  const int HoWo = a.Ho * a.Wo;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  const int nv = (int)(total - i4 < 4 ? total - i4 : 4);
  for (int z = 0; z < a.splits; z++)
    for (int e = 0; e < nv; e++) v[e] += a.part[(size_t)z * total + i4 + e];
  for (int e = 0; e < nv; e++) {
    const size_t off = i4 + e;
    float r = v[e];
    if (a.bias) r += a.bias[(off / HoWo) % a.Cout];
    if (a.res) r += a.res[off];
    if (a.relu) r = fmaxf(r, 0.f);
    const size_t per = (size_t)a.Cout * HoWo, ob = off / per;
    a.out[(ob * a.o_cstride + a.o_coff) * HoWo + (off - ob * per)] = r;
  }
}

// ---- the same kernel on the bf16 matrix pipe at fp32 accuracy (flags bit 8, AP_CONV_SPLIT) -----------------------
// Operands split exactly into three bf16 parts, the six partial products >= 2^-16 of each product on
// v_mfma_f32_32x32x16_bf16, fp32 accumulate (the arithmetic of ap_resblock_f32s.hip): 24 MFMAs of 32 cycles per
// 16-row chunk and wave instead of 32 of 64.  Weights come pre-split as A fragments ([group][row tile][k'/16][split]
// [lane][8 bf16]); a thread stages 8 consecutive k' of one column (8 gathers HW apart -> 3 ds_write_b128 into the
// [column][k'] bf16 images, 48-B rows: conflict-free b128 fragment reads).

typedef _Float16 ch16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 ch16x2 __attribute__((ext_vector_type(2)));
// AP_CONV_SPLIT_F16 (flags bit 10; not fp32-class: the residual-block mode with this arithmetic was removed in round 5) -- operands as two fp16 parts (22 significant
// bits), three partial products on v_mfma_f32_32x32x16_f16, weights x 2^4 at pack time and activations x 2^4 at staging
// (exact; the epilogue multiplies by 2^-8), scaled values clamped to +-60000.
constexpr float CWSC = 16.0f, CXSC = 16.0f;

template <int BM, int BN, bool H16 = false>
__global__ __launch_bounds__(256, 3) void conv2d_split_kernel(ConvArgs a, const void *__restrict__ afrag) {
  constexpr int BK = 16, NX = BM / 64, NY = BN / 64, RS = 48;   // RS: bytes per column row of a B image
  constexpr int IMG = BN * RS;
  constexpr int NS = H16 ? 2 : 3;                               // parts per operand
  static_assert(BN == 128, "staging map: 256 threads = 128 columns x 2 k' octets");
  __shared__ __attribute__((aligned(16))) unsigned char Bs[2][NS][IMG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int j = lane & 31, hh = lane >> 5;
  const int Mg = a.Cout / a.groups, Cg = a.Cin / a.groups, KK = a.kh * a.kw, Kg = Cg * KK;
  const int HoWo = a.Ho * a.Wo, N = a.B * HoWo;
  const int g = blockIdx.z, m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int nl = tid & (BN - 1), ko = tid / BN;        // this thread stages k' = 8 ko .. 8 ko + 7 of column nl
  const int n = n0 + nl;
  const bool nvalid = n < N;
  const int bb = nvalid ? n / HoWo : 0, pp = nvalid ? n % HoWo : 0;
  const int iy0 = (pp / a.Wo) * a.stride - a.pad_h, ix0 = (pp % a.Wo) * a.stride - a.pad;
  const int HW = a.H * a.W;
  const float *xb = a.x + ((size_t)bb * a.x_cstride + a.x_coff + (size_t)g * Cg + 8 * ko) * HW;
  const int MT = (Mg + 31) / 32, KS = Kg / 16, CPT = Cg / BK;
  const u32x4 *af[NX];
#pragma unroll
  for (int x_ = 0; x_ < NX; x_++) {
    const int mt = min((m0 >> 5) + NX * wm + x_, MT - 1);
    af[x_] = reinterpret_cast<const u32x4 *>(afrag) + ((size_t)g * MT + mt) * KS * NS * 64 + lane;
  }
  const int nchunk = KK * CPT;
  float br[8];
  auto load_b = [&](int c) {
    const int r = c / CPT, c0 = (c - r * CPT) * BK;
    const int ky = r / a.kw, kx = r - ky * a.kw;
    const int iy = iy0 + ky * a.dil_h, ix = ix0 + kx * a.dil_w;
    const bool ok = nvalid && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
    const float *p = xb + (size_t)c0 * HW + (ok ? iy * a.W + ix : 0);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const float v = p[(size_t)i * HW];
      br[i] = ok ? v : 0.f;
    }
  };
  auto load_a = [&](u32x4(&aa)[NX][NS], int c) {
#pragma unroll
    for (int x_ = 0; x_ < NX; x_++)
#pragma unroll
      for (int sp = 0; sp < NS; sp++) aa[x_][sp] = af[x_][(size_t)(NS * c + sp) * 64];
  };
  auto store_b = [&](int buf) {
    u32x4 pk[NS];
#pragma unroll
    for (int pr = 0; pr < 4; pr++) {
      float v0 = br[2 * pr], v1 = br[2 * pr + 1];
      if constexpr (H16) {
        const f32x2 v = {__builtin_amdgcn_fmed3f(v0 * CXSC, -60000.0f, 60000.0f),
                          __builtin_amdgcn_fmed3f(v1 * CXSC, -60000.0f, 60000.0f)};
        const ch16x2 hi = __builtin_convertvector(v, ch16x2);
        const ch16x2 lo = __builtin_convertvector(v - __builtin_convertvector(hi, f32x2), ch16x2);
        pk[0][pr] = __builtin_bit_cast(unsigned, hi);
        pk[1][pr] = __builtin_bit_cast(unsigned, lo);
      } else {
#pragma unroll
        for (int sp = 0; sp < 3; sp++) {
          const unsigned w = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v0, v1}, bf16x2));
          pk[sp][pr] = w;
          if (sp < 2) {
            v0 -= __builtin_bit_cast(float, w << 16);
            v1 -= __builtin_bit_cast(float, w & 0xffff0000u);
          }
        }
      }
    }
#pragma unroll
    for (int sp = 0; sp < NS; sp++) *reinterpret_cast<u32x4 *>(&Bs[buf][sp][nl * RS + ko * 16]) = pk[sp];
  };
  f32x16 acc[NX][NY];
#pragma unroll
  for (int x_ = 0; x_ < NX; x_++)
#pragma unroll
    for (int y_ = 0; y_ < NY; y_++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[x_][y_][r] = 0.f;
  auto compute = [&](const u32x4(&aa)[NX][NS], int buf) {
#pragma unroll
    for (int y_ = 0; y_ < NY; y_++) {
      u32x4 bv[NS];
#pragma unroll
      for (int sp = 0; sp < NS; sp++)
        bv[sp] = *reinterpret_cast<const u32x4 *>(&Bs[buf][sp][(32 * NY * wn + 32 * y_ + j) * RS + hh * 16]);
#pragma unroll
      for (int x_ = 0; x_ < NX; x_++) {
        if constexpr (H16) {
#define AP_CT(i, jx)                                                                                                    \
  acc[x_][y_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(ch16x8, aa[x_][i]), __builtin_bit_cast(ch16x8, bv[jx]), \
                                                       acc[x_][y_], 0, 0, 0);
          AP_CT(0, 0) AP_CT(0, 1) AP_CT(1, 0)
#undef AP_CT
        } else {
#define AP_CT(i, jx)                                                                                                       \
  acc[x_][y_] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, aa[x_][i]), __builtin_bit_cast(bf16x8, bv[jx]), \
                                                        acc[x_][y_], 0, 0, 0);
          AP_CT(0, 0) AP_CT(0, 1) AP_CT(1, 0) AP_CT(0, 2) AP_CT(2, 0) AP_CT(1, 1)
#undef AP_CT
        }
      }
    }
  };
  u32x4 a0[NX][NS], a1[NX][NS];
  load_a(a0, 0);
  load_b(0);
  store_b(0);
  __syncthreads();
#pragma unroll 1
  for (int c = 0; c < nchunk; c++) {
    const int cn = c + 1 < nchunk ? c + 1 : c;
    load_b(cn);
    load_a(a1, cn);
    compute(a0, c & 1);
    store_b((c + 1) & 1);
#pragma unroll
    for (int x_ = 0; x_ < NX; x_++)
#pragma unroll
      for (int sp = 0; sp < NS; sp++) a0[x_][sp] = a1[x_][sp];
    __syncthreads();
  }
#pragma unroll
  for (int y_ = 0; y_ < NY; y_++) {
    const int nn = n0 + 32 * NY * wn + 32 * y_ + j;
    if (nn < N) {
      const int ob = nn / HoWo, op = nn % HoWo;
#pragma unroll
      for (int x_ = 0; x_ < NX; x_++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int m = m0 + 32 * NX * wm + 32 * x_ + rowoff(r, hh);
          if (m < Mg) {
            const int co = g * Mg + m;
            const size_t off = ((size_t)ob * a.Cout + co) * HoWo + op;
            float v = acc[x_][y_][r];
            if constexpr (H16) v *= 1.0f / (CWSC * CXSC);
            if (a.bias) v += a.bias[co];
            if (a.res) v += a.res[off];
            if (a.relu) v = fmaxf(v, 0.f);
            a.out[off] = v;
          }
        }
    }
  }
}

// w -> 3-way split A fragments of v_mfma_f32_32x32x16_bf16, tap-major K: [group][row tile][k'/16][split][lane][8]
__global__ void conv_pack_split_kernel(const float *__restrict__ w, const float *__restrict__ scale,
                                       __bf16 *__restrict__ out, int Cout, int Cg, int KK, int groups) {
  const int Mg = Cout / groups, MT = (Mg + 31) / 32, Kg = Cg * KK, KS = Kg / 16;
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;          // one thread per (.., lane, jj), all 3 splits
  const size_t total = (size_t)groups * MT * KS * 64 * 8;
  if (idx >= total) return;
  const int jj = idx & 7, lane = (idx >> 3) & 63;
  size_t rest = idx >> 9;
  const int q = rest % KS; rest /= KS;
  const int mt = rest % MT, g = rest / MT;
  const int i = lane & 31, h = lane >> 5;
  const int kp = 16 * q + 8 * h + jj;
  const int r = kp / Cg, ci = kp - r * Cg;
  const int m = 32 * mt + i;
  float v = 0.f;
  if (m < Mg) {
    const int co = g * Mg + m;
    v = w[((size_t)co * Cg + ci) * KK + r];
    if (scale) v *= scale[co];
  }
  __bf16 p[3];
  split3(v, p);
  const size_t frag = (((size_t)g * MT + mt) * KS + q) * 3;
#pragma unroll
  for (int sp = 0; sp < 3; sp++) out[((frag + sp) * 64 + lane) * 8 + jj] = p[sp];
}

// w x 2^4 -> two fp16 parts as A fragments of v_mfma_f32_32x32x16_f16: [group][row tile][k'/16][split][lane][8]
__global__ void conv_pack_splith_kernel(const float *__restrict__ w, const float *__restrict__ scale,
                                        _Float16 *__restrict__ out, int Cout, int Cg, int KK, int groups) {
  const int Mg = Cout / groups, MT = (Mg + 31) / 32, Kg = Cg * KK, KS = Kg / 16;
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)groups * MT * KS * 64 * 8;
  if (idx >= total) return;
  const int jj = idx & 7, lane = (idx >> 3) & 63;
  size_t rest = idx >> 9;
  const int q = rest % KS; rest /= KS;
  const int mt = rest % MT, g = rest / MT;
  const int i = lane & 31, h = lane >> 5;
  const int kp = 16 * q + 8 * h + jj;
  const int r = kp / Cg, ci = kp - r * Cg;
  const int m = 32 * mt + i;
  float v = 0.f;
  if (m < Mg) {
    const int co = g * Mg + m;
    v = w[((size_t)co * Cg + ci) * KK + r];
    if (scale) v *= scale[co];
  }
  v = fminf(fmaxf(v * CWSC, -60000.0f), 60000.0f);
  const _Float16 p0 = (_Float16)v, p1 = (_Float16)(v - (float)p0);
  const size_t frag = (((size_t)g * MT + mt) * KS + q) * 2;
  out[((frag + 0) * 64 + lane) * 8 + jj] = p0;
  out[((frag + 1) * 64 + lane) * 8 + jj] = p1;
}

// w [Cout][Cin/g][kh][kw] (* scale) -> A-operand fragments of v_mfma_f32_32x32x2_f32 in tap-major K order:
// [group][row tile MT][k'/8][lane 64][4], lane = (row i, half h), element e of octet q: k' = 8 q + 4 h + e -- MFMA step (q, e) takes
// k' = 8q + e from lane half 0 and 8q + 4 + e from half 1, so that a lane's B operands of four consecutive steps are four
// CONSECUTIVE k' of its column: one ds_read_b128 from a [column][k'] image (every LDS read that lands in VGPRs costs the matrix
// pipe 10-19 cycles on its SIMD; four steps per read instead of one: tools/micro/mfma_f32_lds.hip, 0.85 -> 0.95 of peak)
__global__ void conv_pack_frag_kernel(const float *__restrict__ w, const float *__restrict__ scale,
                                      float *__restrict__ out, int Cout, int Cg, int KK, int groups) {
  const int Mg = Cout / groups, MT = (Mg + 31) / 32, Kg = Cg * KK, KQ = Kg / 8;
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)groups * MT * KQ * 256;
  if (idx >= total) return;
  const int e = idx & 3, lane = (idx >> 2) & 63;
  size_t rest = idx >> 8;
  const int q = rest % KQ; rest /= KQ;
  const int mt = rest % MT, g = rest / MT;
  const int i = lane & 31, h = lane >> 5;
  const int kp = 8 * q + 4 * h + e;                             // k' = r Cg + ci
  const int r = kp / Cg, ci = kp - r * Cg;
  const int m = 32 * mt + i;
  float v = 0.f;
  if (m < Mg) {
    const int co = g * Mg + m;
    v = w[((size_t)co * Cg + ci) * KK + r];
    if (scale) v *= scale[co];
  }
  out[idx] = v;
}

// w [Cout][Cin/g][kh][kw] (* per-output-channel scale) -> wT [groups][Kg][Mg]
__global__ void conv_pack_kernel(const float *__restrict__ w, const float *__restrict__ scale, float *__restrict__ wT,
                                 int Cout, int Kg, int groups) {
  const int Mg = Cout / groups;
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)Cout * Kg) return;
  const int m = idx % Mg;
  size_t rest = idx / Mg;
  const int k = rest % Kg, g = rest / Kg;
  const int co = g * Mg + m;
  float v = w[(size_t)co * Kg + k];
  if (scale) v *= scale[co];
  wT[idx] = v;
}

// y = x * scale[c] + shift[c] (eval-mode BatchNorm), optional ReLU; x may be a channel slice of a wider tensor
__global__ void affine_kernel(const float *__restrict__ x, const float *__restrict__ scale, const float *__restrict__ shift,
                              float *__restrict__ y, int C, int HW, int x_cstride, int x_coff, int relu, size_t total) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int p = idx % HW;
  size_t rest = idx / HW;
  const int c = rest % C;
  const size_t b = rest / C;
  float v = x[((size_t)b * x_cstride + x_coff + c) * HW + p];
  if (scale) v = v * scale[c] + shift[c];
  if (relu) v = fmaxf(v, 0.f);
  y[idx] = v;
}

// y = a + b (optionally ReLU); operands may be channel slices
__global__ void add_kernel(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ y, int C, int HW,
                           int a_cs, int a_co, int b_cs, int b_co, int relu, size_t total) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int p = idx % HW;
  size_t rest = idx / HW;
  const int c = rest % C;
  const size_t n = rest / C;
  float v = a[((size_t)n * a_cs + a_co + c) * HW + p] + b[((size_t)n * b_cs + b_co + c) * HW + p];
  if (relu) v = fmaxf(v, 0.f);
  y[idx] = v;
}

// copy C channels of src (slice) into dst at channel offset (torch.cat / slices)
__global__ void copy_channels_kernel(const float *__restrict__ src, float *__restrict__ dst, int C, int HW, int s_cs,
                                     int s_co, int d_cs, int d_co, size_t total) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int p = idx % HW;
  size_t rest = idx / HW;
  const int c = rest % C;
  const size_t n = rest / C;
  dst[((size_t)n * d_cs + d_co + c) * HW + p] = src[((size_t)n * s_cs + s_co + c) * HW + p];
}

// the same slice copy as a 2-D copy: the C channels of one sample are one contiguous run of C HW floats on both sides, moved
// with 16-byte accesses, four per thread (blockIdx.y = the sample)
__global__ __launch_bounds__(256) void copy_rows_kernel(const float *__restrict__ src, float *__restrict__ dst, unsigned row4,
                                                        size_t s_row, size_t d_row) {
  const f32x4 *sp = (const f32x4 *)(src + blockIdx.y * s_row);
  f32x4 *dp = (f32x4 *)(dst + blockIdx.y * d_row);
  const unsigned i0 = blockIdx.x * 1024 + threadIdx.x;
  f32x4 v[4];
#pragma unroll
  for (int u = 0; u < 4; u++)
    if (i0 + u * 256 < row4) v[u] = sp[i0 + u * 256];
#pragma unroll
  for (int u = 0; u < 4; u++)
    if (i0 + u * 256 < row4) dp[i0 + u * 256] = v[u];
}

// max / average pooling (count_include_pad semantics of F.avg_pool2d default; no padding used by the reference nets)
__global__ void pool2d_kernel(const float *__restrict__ x, float *__restrict__ y, int H, int W, int Ho, int Wo, int k,
                              int stride, int pad, int is_max, size_t total) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int ox = idx % Wo;
  size_t rest = idx / Wo;
  const int oy = rest % Ho;
  const size_t bc = rest / Ho;
  const float *xp = x + bc * (size_t)H * W;
  float v = is_max ? -INFINITY : 0.f;
  for (int ky = 0; ky < k; ky++) {
    const int iy = oy * stride - pad + ky;
    for (int kx = 0; kx < k; kx++) {
      const int ix = ox * stride - pad + kx;
      const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
      if (is_max) { if (in) v = fmaxf(v, xp[(size_t)iy * W + ix]); }
      else if (in) v += xp[(size_t)iy * W + ix];
    }
  }
  y[idx] = is_max ? v : v / (float)(k * k);
}

}  // namespace ap

using namespace ap;

// which kernel serves a layer: ap_conv_plan.h (conv_plan), on these thresholds
#ifdef AP_TOOLS
static ConvTune g_conv_tune;
extern "C" int ap_debug_conv_w3(int on, int min_pairs) {
  g_conv_tune.w3 = on & 3; g_conv_tune.w3_split = (on & 4) ? 0 : 1;
  g_conv_tune.w3_min_pairs = min_pairs;
  return 0;
}
extern "C" int ap_debug_conv_p1(int on) { g_conv_tune.p1 = on; return 0; }
extern "C" int ap_debug_conv_splitk(int t2, int cap) { g_conv_tune.splitk_t2 = t2; g_conv_tune.splitk_cap = cap; return 0; }
extern "C" int ap_debug_conv_path(int no_frag) {
  if (no_frag >= 16) g_conv_tune.frag_min_tiles = no_frag;   // >= 16: set the tile-count threshold of the streamed-weight kernel
  else if (no_frag >= 4 && no_frag <= 8) g_conv_tune.force = no_frag == 8 ? 0 : no_frag;
  else if (no_frag == 2 || no_frag == 3) g_conv_tune.wide_1x1 = no_frag == 2;   // 2 / 3: pointwise layers on 128 x 128 tiles / back on 128 x 64
  else g_conv_tune.no_frag = no_frag;
  return 0;
}
#else
static constexpr ConvTune g_conv_tune;
#endif

extern "C" size_t ap_conv2d_packed_elems(int Cout, int Cin_g, int kh, int kw, int groups) {
  if (Cout < 1 || Cin_g < 1 || kh < 1 || kw < 1 || groups < 1 || Cout % groups) return 0;
  return conv_images(Cout, Cin_g, kh, kw, groups).total;
}
extern "C" int ap_conv2d_pack(const float *w, const float *scale, float *wT, int Cout, int Cin_g, int kh, int kw,
                              int groups, void *stream) {
  if (!w || !wT || Cout < 1 || Cin_g < 1 || groups < 1 || Cout % groups) { set_error("ap_conv2d_pack: bad argument"); return -22; }
  const int Kg = Cin_g * kh * kw;
  const size_t n = (size_t)Cout * Kg;
  const ConvImages im = conv_images(Cout, Cin_g, kh, kw, groups);
  conv_pack_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(w, scale, wT, Cout, Kg, groups);
  if (im.has_frag) {
    const unsigned nb = (unsigned)((im.frag_elems + 255) / 256);
    conv_pack_frag_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(w, scale, wT + im.frag, Cout, Cin_g, kh * kw, groups);
    conv_pack_split_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(w, scale, reinterpret_cast<__bf16 *>(wT + im.split), Cout, Cin_g, kh * kw,
                                                                groups);
    conv_pack_splith_kernel<<<nb, 256, 0, (hipStream_t)stream>>>(w, scale, reinterpret_cast<_Float16 *>(wT + im.splith), Cout, Cin_g,
                                                                 kh * kw, groups);
  }
  if (im.has_w3)
    if (const int rc = launch_conv_pack_w3(w, scale, wT + im.w3, Cout, Cin_g, (hipStream_t)stream)) return rc;
  AP_HIP(hipGetLastError());
  return 0;
}

// ---- per-kernel measurement of the conv family (bench.py, BASELINE configs[4]): while enabled every ap_conv2d_fwd launch is
// bracketed by a pair of HIP events on its launch stream and its algorithmic flops (2 N M K) are summed per kernel class.
namespace {
struct ConvProf {
  bool on = false;
  std::vector<hipEvent_t> ev;                 // (start, stop) pairs
  std::vector<double> flop;                   // per recorded launch
  std::vector<int> cls;                       // kernel class per recorded launch: conv_class (ap_conv_plan.h) -- 0 / 1 / 2 streamed-weight
  size_t used = 0;                            //   128x128 / 64x128 / 128x64, 64x64 and split-K, 3 split operands, 4 LDS-staged, 5 generic / few, 6 F(2,3), 7 tools
  std::vector<int> shape;                     // 9 ints per recorded launch: B Cin H W Cout kh kw stride groups
  void reset() { used = 0; flop.clear(); cls.clear(); shape.clear(); }   // (the events are kept and reused)
} g_cprof;
}  // namespace

// Split-K partial sums live in a caller-owned device buffer (no allocation inside the library): without one, or with one
// that is too small for a layer, that layer runs un-split.
// One slot per HIP device, keyed by the device that is current when the buffer is handed over and when a layer is launched:
// a launch on device 1 can never be pointed at device 0's buffer.  A device's buffer serves ONE stream at a time (a split-K
// layer and its reduce own it between them): callers that drive two streams of one device give each its own call sequence
// with ap_conv2d_set_workspace(NULL, 0) (un-split) or serialise them.
namespace {
constexpr int AP_MAX_DEVICES = 64;
struct ConvWs { float *p = nullptr; size_t bytes = 0; } g_conv_ws_tab[AP_MAX_DEVICES];
inline ConvWs conv_ws_here() {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= AP_MAX_DEVICES) return ConvWs{};
  return g_conv_ws_tab[dev];
}
}  // namespace
extern "C" int ap_conv2d_set_workspace(float *ws, size_t bytes) {
  int dev = -1;
  AP_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= AP_MAX_DEVICES) { set_error("ap_conv2d_set_workspace: device index %d out of range", dev); return -22; }
  if (ws) {                                       // the buffer must live on the device it is registered for
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ws) != hipSuccess || at.device != dev) {
      (void)hipGetLastError();
      set_error("ap_conv2d_set_workspace: buffer is not memory of the current device %d", dev);
      return -22;
    }
  }
  g_conv_ws_tab[dev].p = ws;
  g_conv_ws_tab[dev].bytes = ws ? bytes : 0;
  return 0;
}

extern "C" int ap_conv_profile_enable(int enable) {
  g_cprof.on = enable != 0;
  g_cprof.reset();
  return 0;
}

// launch i of the recording (before ap_conv_profile_read resets it): its time, flops and [B Cin H W Cout kh kw stride groups class]
extern "C" int ap_conv_profile_launch(int i, double *ms, double *flop, int *shape10) {
  if (i < 0 || (size_t)i >= g_cprof.flop.size() || !ms || !flop || !shape10) return 1;
  AP_HIP(hipEventSynchronize(g_cprof.ev[2 * i + 1]));
  float t = 0.f;
  AP_HIP(hipEventElapsedTime(&t, g_cprof.ev[2 * i], g_cprof.ev[2 * i + 1]));
  *ms = t;
  *flop = g_cprof.flop[i];
  for (int k = 0; k < 9; k++) shape10[k] = g_cprof.shape[9 * (size_t)i + k];
  shape10[9] = g_cprof.cls[i];
  return 0;
}

extern "C" int ap_conv_profile_read(double *ms_by_class, double *flop_by_class, int64_t *launches_by_class, int n_classes) {
  if (!ms_by_class || !flop_by_class || !launches_by_class || n_classes < 7) { set_error("ap_conv_profile_read: bad argument"); return -22; }
  for (int c = 0; c < n_classes; c++) { ms_by_class[c] = 0; flop_by_class[c] = 0; launches_by_class[c] = 0; }
  for (size_t i = 0; i < g_cprof.flop.size(); i++) {
    AP_HIP(hipEventSynchronize(g_cprof.ev[2 * i + 1]));
    float ms = 0.f;
    AP_HIP(hipEventElapsedTime(&ms, g_cprof.ev[2 * i], g_cprof.ev[2 * i + 1]));
    ms_by_class[g_cprof.cls[i]] += ms;
    flop_by_class[g_cprof.cls[i]] += g_cprof.flop[i];
    launches_by_class[g_cprof.cls[i]] += 1;
  }
  g_cprof.reset();
  return 0;
}

namespace {
// one helper per kernel family: the plan's (tile, form) -> the template instantiation.  Exactly the forms conv_plan asks for are
// listed (the pointer form never stages pointwise; 64-row tiles do so only as a forced tile of the tools build): no others are built.
int launch_big2(const ConvPlan &p, const ConvArgs &a, const float *afrag, dim3 grid, hipStream_t st) {
  const unsigned xb = p.buf ? (unsigned)p.xbytes : 0u, ab = p.buf ? (unsigned)p.abytes : 0u;
#define AP_BIG2(BM_, BN_, BUF_, P1_) \
  case BM_ * 1000 + BN_ * 4 + BUF_ * 2 + P1_: conv2d_f32_big2_kernel<BM_, BN_, BUF_, P1_><<<grid, 256, 0, st>>>(a, afrag, xb, ab); return 0;
  switch (p.BM * 1000 + p.BN * 4 + p.buf * 2 + p.p1) {
    AP_BIG2(128, 128, true, true) AP_BIG2(128, 128, true, false) AP_BIG2(128, 128, false, false)
    AP_BIG2(128, 64, true, true) AP_BIG2(128, 64, true, false) AP_BIG2(128, 64, false, false)
    AP_BIG2(64, 128, true, false) AP_BIG2(64, 128, false, false)
    AP_BIG2(64, 64, true, false) AP_BIG2(64, 64, false, false)
#ifdef AP_TOOLS
    AP_BIG2(64, 128, true, true) AP_BIG2(64, 64, true, true)
#endif
  }
#undef AP_BIG2
  set_error("ap_conv2d_fwd: no streamed-weight kernel %d x %d buf %d p1 %d", p.BM, p.BN, (int)p.buf, (int)p.p1); return -22;
}
void launch_split(const ConvPlan &p, const ConvArgs &a, const float *wT, const ConvImages &im, dim3 grid, hipStream_t st) {
  if (p.family == CONV_SPLITH && p.BM == 128) conv2d_split_kernel<128, 128, true><<<grid, 256, 0, st>>>(a, wT + im.splith);
  else if (p.family == CONV_SPLITH) conv2d_split_kernel<64, 128, true><<<grid, 256, 0, st>>>(a, wT + im.splith);
  else if (p.BM == 128) conv2d_split_kernel<128, 128><<<grid, 256, 0, st>>>(a, wT + im.split);
  else conv2d_split_kernel<64, 128><<<grid, 256, 0, st>>>(a, wT + im.split);
}
void launch_few(const ConvPlan &p, const ConvArgs &a, dim3 grid, hipStream_t st) {
#define AP_FEW(MO_, K3_) case (K3_ ? -MO_ : MO_): conv2d_few_kernel<MO_, K3_><<<grid, 256, p.lds, st>>>(a); break;
  switch (p.k3_nb ? -p.BM : p.BM) { AP_FEW(1, true) AP_FEW(2, true) AP_FEW(3, true) AP_FEW(4, true) AP_FEW(1, false) AP_FEW(2, false) AP_FEW(3, false) AP_FEW(4, false) }
#undef AP_FEW
}
// launches what the plan says (p.family / p.cls are rewritten where the tools build's pointwise kernel took the layer instead)
int conv_launch(ConvPlan &p, const ConvArgs &a, const ConvImages &im, hipStream_t st) {
  const dim3 grid(p.grid[0], p.grid[1], p.grid[2]);
  const bool raw = p.splits > 1;                    // K slices write raw partial sums: bias / residual / ReLU move to the reduce
#ifdef AP_TOOLS
  if (p.try_p1 && conv_p1_serves(a.B, a.Cin, a.H, a.W, a.Cout, a.kh, a.kw, a.stride, a.pad, a.groups)) {
    const int rc = launch_conv_p1(a.x, a.wT + im.frag, a.bias, a.res, a.out, a.B, a.Cin, a.H, a.W, a.Cout, a.relu, a.x_cstride, a.x_coff,
                                  a.o_cstride, a.o_coff, p.abytes, st);
    if (rc != 1) { p.family = CONV_P1; p.cls = conv_class(CONV_P1, 0, 0); return rc; }
  }
#endif
  int rc = 0;
  switch (p.family) {
    case CONV_W3:
      rc = launch_conv_w3(a.x, a.wT + im.w3, raw ? nullptr : a.bias, raw ? nullptr : a.res, a.out, a.B, a.Cin, a.H, a.W, a.Cout,
                          raw ? 0 : a.relu, a.x_cstride, a.x_coff, a.o_cstride, a.o_coff, st, p.splits, a.part); break;
    case CONV_BIG2: rc = launch_big2(p, a, a.wT + im.frag, grid, st); break;
    case CONV_SPLIT: case CONV_SPLITH: launch_split(p, a, a.wT, im, grid, st); break;
    case CONV_FEW: launch_few(p, a, grid, st); break;
    case CONV_BIG: conv2d_f32_big_kernel<<<grid, 256, 0, st>>>(a); break;
    default: conv2d_f32_kernel<<<grid, 256, 0, st>>>(a); break;
  }
  if (rc) return rc;
  if (p.reduce) {                                   // the slices summed in order (deterministic), + bias / residual / ReLU
    const size_t total = (size_t)a.B * a.Cout * a.Ho * a.Wo;
    conv_splitk_reduce_kernel<<<(unsigned)((total / 4 + 255) / 256 + 1), 256, 0, st>>>(a, total);
  }
  AP_HIP(hipGetLastError());
  return 0;
}
int conv2d_fwd_impl(const float *x, const float *wT, const float *bias, const float *res, float *out, int B, int Cin, int H,
                    int W, int Cout, int kh, int kw, int stride, int pad, int groups, int flags, int x_cstride, int x_coff,
                    void *stream, int o_cstride, int o_coff, ConvGeom *g, int *cls) {
  if (!x || !wT || !out || B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1 || kh < 1 || kw < 1 || stride < 1 || pad < 0 ||
      groups < 1 || Cin % groups || Cout % groups || x_cstride < x_coff + Cin) { set_error("ap_conv2d_fwd: bad argument"); return -22; }
  *g = conv_geom(B, Cin, H, W, Cout, kh, kw, stride, pad, groups, flags, x_cstride, o_cstride, o_coff);
  const ConvImages im = conv_images(Cout, Cin / groups, kh, kw, groups);
  const ConvWs ws = conv_ws_here();
  ConvPlan p;
  if (const int rc = conv_plan(*g, im, g_conv_tune, ws.p ? ws.bytes : 0, &p)) { set_error("%s", p.err); return rc; }
  ConvArgs a;
  a.x = x; a.wT = wT; a.bias = bias; a.res = res; a.out = out;
  a.B = B; a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cout; a.Ho = g->Ho; a.Wo = g->Wo; a.kh = kh; a.kw = kw; a.stride = stride; a.pad = pad;
  a.groups = groups; a.relu = g->relu; a.pad_h = g->pad_h; a.dil_h = g->dil_h; a.dil_w = g->dil_w;
  a.x_cstride = x_cstride; a.x_coff = x_coff; a.o_cstride = g->o_cstride; a.o_coff = g->o_coff;
  a.splits = p.splits; a.part = p.splits > 1 ? ws.p : nullptr;
  const int rc = conv_launch(p, a, im, (hipStream_t)stream);
  *cls = p.cls;
  return rc;
}
}  // namespace

static int conv2d_fwd_entry(const float *x, const float *wT, const float *bias, const float *res, float *out, int B,
                            int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int groups, int flags,
                            int x_cstride, int x_coff, void *stream, int o_cstride, int o_coff) {
  ConvGeom g;
  int cls = 5;
  const bool prof = g_cprof.on;
  while (prof && g_cprof.used + 2 > g_cprof.ev.size()) {
    hipEvent_t e;
    AP_HIP(hipEventCreate(&e));
    g_cprof.ev.push_back(e);
  }
  if (prof) AP_HIP(hipEventRecord(g_cprof.ev[g_cprof.used], (hipStream_t)stream));
  const int rc = conv2d_fwd_impl(x, wT, bias, res, out, B, Cin, H, W, Cout, kh, kw, stride, pad, groups, flags, x_cstride, x_coff, stream,
                                 o_cstride, o_coff, &g, &cls);
  if (!prof) return rc;
  AP_HIP(hipEventRecord(g_cprof.ev[g_cprof.used + 1], (hipStream_t)stream));
  if (rc) return rc;
  g_cprof.used += 2;
  g_cprof.flop.push_back(2.0 * (double)g.N * Cout * (double)(Cin / groups) * kh * kw);
  g_cprof.cls.push_back(cls);
  for (int v : {B, Cin, H, W, Cout, kh, kw, stride, groups}) g_cprof.shape.push_back(v);
  return 0;
}

// the same convolution with `out` a channel slice [out_coff, out_coff + Cout) of a tensor of out_cstride channels (torch.cat's
// destination: the producer writes its half in place).  For layers the streamed-weight fp32 kernel serves: that kernel, its split-K
// reduce, or the F(2,3) kernel where conv_plan prefers it.
extern "C" int ap_conv2d_fwd_slice(const float *x, const float *wT, const float *bias, const float *res, float *out, int B,
                                   int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int groups, int relu,
                                   int x_cstride, int x_coff, int out_cstride, int out_coff, void *stream) {
  if (out_cstride < out_coff + Cout || out_coff < 0) { set_error("ap_conv2d_fwd_slice: bad output slice"); return -22; }
  return conv2d_fwd_entry(x, wT, bias, res, out, B, Cin, H, W, Cout, kh, kw, stride, pad, groups, relu, x_cstride, x_coff, stream, out_cstride,
                          out_coff);
}

extern "C" int ap_conv2d_fwd(const float *x, const float *wT, const float *bias, const float *res, float *out, int B,
                             int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int groups, int relu,
                             int x_cstride, int x_coff, void *stream) {
  return conv2d_fwd_entry(x, wT, bias, res, out, B, Cin, H, W, Cout, kh, kw, stride, pad, groups, relu, x_cstride, x_coff, stream, 0, 0);
}

extern "C" int ap_affine_nchw(const float *x, const float *scale, const float *shift, float *y, int B, int C, int HW,
                              int x_cstride, int x_coff, int relu, void *stream) {
  if (!x || !y || B < 1 || C < 1 || HW < 1 || (scale && !shift)) { set_error("ap_affine_nchw: bad argument"); return -22; }
  size_t total = (size_t)B * C * HW;
  affine_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, scale, shift, y, C, HW, x_cstride, x_coff,
                                                                             relu, total);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_add_nchw(const float *a, const float *b, float *y, int B, int C, int HW, int a_cstride, int a_coff,
                           int b_cstride, int b_coff, int relu, void *stream) {
  if (!a || !b || !y || B < 1 || C < 1 || HW < 1) { set_error("ap_add_nchw: bad argument"); return -22; }
  size_t total = (size_t)B * C * HW;
  add_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(a, b, y, C, HW, a_cstride, a_coff, b_cstride,
                                                                          b_coff, relu, total);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_copy_channels(const float *src, float *dst, int B, int C, int HW, int s_cstride, int s_coff, int d_cstride,
                                int d_coff, void *stream) {
  if (!src || !dst || B < 1 || C < 1 || HW < 1) { set_error("ap_copy_channels: bad argument"); return -22; }
  size_t total = (size_t)B * C * HW;
  const size_t row = (size_t)C * HW, s_row = (size_t)s_cstride * HW, d_row = (size_t)d_cstride * HW;
  const float *s0 = src + (size_t)s_coff * HW;
  float *d0 = dst + (size_t)d_coff * HW;
  if (row % 4 == 0 && s_row % 4 == 0 && d_row % 4 == 0 && (((uintptr_t)s0 | (uintptr_t)d0) & 15) == 0 && row / 4 < (1u << 31) && B < 65536) {
    const unsigned row4 = (unsigned)(row / 4);
    copy_rows_kernel<<<dim3((row4 + 1023) / 1024, (unsigned)B), 256, 0, (hipStream_t)stream>>>(s0, d0, row4, s_row, d_row);
    AP_HIP(hipGetLastError());
    return 0;
  }
  copy_channels_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(src, dst, C, HW, s_cstride, s_coff,
                                                                                    d_cstride, d_coff, total);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_pool2d(const float *x, float *y, int BC, int H, int W, int k, int stride, int pad, int is_max, void *stream) {
  if (!x || !y || BC < 1 || H < 1 || W < 1 || k < 1 || stride < 1 || pad < 0) { set_error("ap_pool2d: bad argument"); return -22; }
  const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  if (Ho < 1 || Wo < 1) { set_error("ap_pool2d: empty output"); return -22; }
  size_t total = (size_t)BC * Ho * Wo;
  pool2d_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, y, H, W, Ho, Wo, k, stride, pad, is_max,
                                                                             total);
  AP_HIP(hipGetLastError());
  return 0;
}

// =============================================================================================================
// Improved-Diffusion UNet pieces (improved_diffusion/unet.py, nn.py)
// =============================================================================================================
namespace ap {

// GroupNorm32 (nn.py:17-19,95-102) [+ (1 + scale) * . + shift of use_scale_shift_norm (unet.py:184-190)] [+ SiLU].
// One workgroup per (sample, group); two passes (mean, then centred variance) like ATen's RowwiseMoments.
__global__ __launch_bounds__(256) void groupnorm_kernel(const float *__restrict__ x, const float *__restrict__ gamma,
                                                        const float *__restrict__ beta, const float *__restrict__ ss,
                                                        float *__restrict__ y, int C, int HW, int groups, float eps,
                                                        int act) {
  __shared__ float red[256];
  const int b = blockIdx.x / groups, g = blockIdx.x % groups, cpg = C / groups, n = cpg * HW;
  const float *xp = x + ((size_t)b * C + (size_t)g * cpg) * HW;
  float *yp = y + ((size_t)b * C + (size_t)g * cpg) * HW;
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += xp[i];
  const float mean = block_tree<256>(s, red, SumOp{}) / (float)n;
  __syncthreads();
  float v = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float dlt = xp[i] - mean;
    v = __builtin_fmaf(dlt, dlt, v);
  }
  const float rstd = 1.0f / sqrtf(block_tree<256>(v, red, SumOp{}) / (float)n + eps);
  for (int i = threadIdx.x; i < n; i += 256) {
    const int c = g * cpg + i / HW;
    float o = (xp[i] - mean) * rstd * gamma[c] + beta[c];
    if (ss) o = o * (1.0f + ss[(size_t)b * 2 * C + c]) + ss[(size_t)b * 2 * C + C + c];
    if (act == 2) o = silu(o);
    else if (act == 1) o = fmaxf(o, 0.f);
    yp[i] = o;
  }
}

// One pass over HBM: the (sample, group) slab -- cpg * HW contiguous floats -- is read once with 16-byte loads, stays in
// registers through the two-pass statistics (mean, then the variance of the deviations: the same arithmetic as above) and is
// written once.  T threads serve one slab: a wave when it has <= 1024 floats (four slabs per block), the block otherwise;
// NV = 16-byte vectors per thread.  HBM-bound: 8 bytes per element.
template <int T, int NV>
__global__ __launch_bounds__(256) void groupnorm_reg_kernel(const float *__restrict__ x, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, const float *__restrict__ ss,
                                                            float *__restrict__ y, int C, int HW, int groups, float eps,
                                                            int act, int slabs) {
  __shared__ float red[8];
  const int slab = blockIdx.x * (256 / T) + (int)threadIdx.x / T, lane = (int)threadIdx.x % T;
  const bool live = slab < slabs;
  const int b = slab / groups, g = slab % groups, cpg = C / groups, n = cpg * HW, n4 = n >> 2;
  const f32x4 *xp = (const f32x4 *)(x + (size_t)slab * n);
  f32x4 *yp = (f32x4 *)(y + (size_t)slab * n);
  f32x4 v[NV];
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < NV; u++) {
    const int i = lane + u * T;
    if (live && i < n4) {
      v[u] = xp[i];
      s += (v[u][0] + v[u][1]) + (v[u][2] + v[u][3]);
    }
  }
  auto total = [&](float a, int slot) -> float {
    a = wave_sum(a);
    if (T == 64) return a;
    if ((threadIdx.x & 63) == 0) red[slot * 4 + (threadIdx.x >> 6)] = a;
    __syncthreads();
    return (red[slot * 4] + red[slot * 4 + 1]) + (red[slot * 4 + 2] + red[slot * 4 + 3]);
  };
  const float mean = total(s, 0) / (float)n;
  float q = 0.f;
#pragma unroll
  for (int u = 0; u < NV; u++)
    if (live && lane + u * T < n4)
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const float dlt = v[u][e] - mean;
        q = __builtin_fmaf(dlt, dlt, q);
      }
  const float rstd = 1.0f / sqrtf(total(q, 1) / (float)n + eps);
#pragma unroll
  for (int u = 0; u < NV; u++) {
    const int i = lane + u * T;
    if (live && i < n4) {
      const int c = g * cpg + (i * 4) / HW;                       // HW % 4 == 0: the four elements share a channel
      float ga = rstd * gamma[c], be = beta[c] - mean * ga;
      if (ss) {
        const float sc = 1.0f + ss[(size_t)b * 2 * C + c];
        ga *= sc;
        be = be * sc + ss[(size_t)b * 2 * C + C + c];
      }
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float r = __builtin_fmaf(v[u][e], ga, be);
        if (act == 2) r = silu(r);
        else if (act == 1) r = fmaxf(r, 0.f);
        o[e] = r;
      }
      yp[i] = o;
    }
  }
}

// timestep_embedding (nn.py:103-121): out[b] = [cos(t_b f_j), sin(t_b f_j)]
__global__ void timestep_embedding_kernel(const float *__restrict__ t, const float *__restrict__ freqs,
                                          float *__restrict__ out, int half, int total) {
  int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int b = idx / half, jx = idx % half;
  const float a = t[b] * freqs[jx];
  out[(size_t)b * 2 * half + jx] = cosf(a);
  out[(size_t)b * 2 * half + half + jx] = sinf(a);
}

__global__ void silu_kernel(const float *__restrict__ x, float *__restrict__ y, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = silu(x[i]);
}

// F.interpolate(scale_factor=2, mode="nearest") (unet.py:60-72)
__global__ void upsample2x_kernel(const float *__restrict__ x, float *__restrict__ y, int H, int W, size_t total) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int W2 = 2 * W, H2 = 2 * H;
  const int ox = idx % W2;
  size_t rest = idx / W2;
  const int oy = rest % H2;
  const size_t bc = rest / H2;
  y[idx] = x[(bc * H + (oy >> 1)) * W + (ox >> 1)];
}

// QKVAttention (unet.py:239-252) on the legacy layout qkv [B][heads][3 ch][T]: one workgroup per (sample, head), K and V
// of the head in LDS (broadcast reads), one query per thread, exact two-pass softmax in fp32.
template <int CH>
__global__ __launch_bounds__(256) void attention_kernel(const float *__restrict__ qkv, float *__restrict__ out, int T,
                                                        int heads, float scale2) {
  extern __shared__ float sm[];
  float *ks = sm, *vs = sm + (size_t)CH * T;
  const int bh = blockIdx.x;
  const float *base = qkv + (size_t)bh * 3 * CH * T;
  for (int i = threadIdx.x; i < CH * T; i += 256) {
    ks[i] = base[(size_t)CH * T + i];
    vs[i] = base[(size_t)2 * CH * T + i];
  }
  __syncthreads();
  const bool vec4 = (T % 4) == 0;
  for (int t = threadIdx.x; t < T; t += 256) {
    float q[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) q[c] = base[(size_t)c * T + t] * scale2;
    // single pass with a running maximum (exact softmax: every term is rescaled when the maximum moves);
    // keys are consumed four at a time so each LDS read (ds_read_b128, broadcast) feeds four FMAs
    float acc[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) acc[c] = 0.f;
    float mx = -INFINITY, l = 0.f;
    if (vec4) {
      for (int s = 0; s < T; s += 4) {
        f32x4 w = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < CH; c++) w += q[c] * *reinterpret_cast<const f32x4 *>(ks + c * T + s);
        const float bm = fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3]));
        if (bm > mx) {
          const float corr = expf(mx - bm);       // exp(-inf) = 0 on the first block
          l *= corr;
#pragma unroll
          for (int c = 0; c < CH; c++) acc[c] *= corr;
          mx = bm;
        }
        f32x4 p;
#pragma unroll
        for (int i = 0; i < 4; i++) p[i] = expf(w[i] - mx);
        l += (p[0] + p[1]) + (p[2] + p[3]);
#pragma unroll
        for (int c = 0; c < CH; c++) {
          const f32x4 vv = *reinterpret_cast<const f32x4 *>(vs + c * T + s);
          acc[c] += (p[0] * vv[0] + p[1] * vv[1]) + (p[2] * vv[2] + p[3] * vv[3]);
        }
      }
    } else {
      for (int s = 0; s < T; s++) {
        float w = 0.f;
#pragma unroll
        for (int c = 0; c < CH; c++) w = __builtin_fmaf(q[c], ks[c * T + s], w);
        if (w > mx) {
          const float corr = expf(mx - w);
          l *= corr;
#pragma unroll
          for (int c = 0; c < CH; c++) acc[c] *= corr;
          mx = w;
        }
        const float p = expf(w - mx);
        l += p;
#pragma unroll
        for (int c = 0; c < CH; c++) acc[c] = __builtin_fmaf(p, vs[c * T + s], acc[c]);
      }
    }
    const float inv = 1.0f / l;
    float *op = out + (size_t)bh * CH * T;
#pragma unroll
    for (int c = 0; c < CH; c++) op[(size_t)c * T + t] = acc[c] * inv;
  }
}

// The same attention on the fp32 MFMA for the UNet's shapes (64 channels per head, T = 64 / 256 positions).
// Everything is computed transposed so that nothing ever moves between lanes:
//   S^T[key][query] = sum_c K[c][key] Q[c][query]   A = K from LDS (lane = key), B = Q in registers (lane = query)
//   -> a lane owns ONE query and, in its accumulator registers, its scores against 16 keys per 32-key tile: the
//      softmax maximum / sum run over the lane's own registers plus one xor-32 shuffle;
//   O^T[c][query] = sum_key V[c][key] P[key][query]  B = P straight from those registers (the k-pair of an MFMA step is
//      the pair of keys the two lane halves hold in the same register), A = V from a transposed LDS image (lane = channel).
// One workgroup per (sample, head), one wave per 32-query block.
template <int NT>                                               // NT = T / 32 key tiles (2 or 8)
__global__ __launch_bounds__(NT >= 8 ? 512 : 256) void attention_mfma_kernel(const float *__restrict__ qkv, float *__restrict__ out,
                                                                             float scale2) {
  constexpr int CH = 64, T = 32 * NT, VS = CH + 1, NTHR = NT >= 8 ? 512 : 256;   // T = 256: eight waves, two per SIMD -- one
  // wave's softmax (256 exp per lane) and operand latencies run under the other's MFMAs
  extern __shared__ float sm[];
  float *ks = sm;                                               // [CH][T]
  float *vt = sm + CH * T;                                      // [T][CH + 1]
  const int bh = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, hh = lane >> 5;
  const float *base = qkv + (size_t)bh * 3 * CH * T;
  for (int i = tid; i < CH * T; i += NTHR) {
    ks[i] = base[(size_t)CH * T + i];
    const int c = i / T, t = i - c * T;
    vt[t * VS + c] = base[(size_t)2 * CH * T + i];
  }
  __syncthreads();
  for (int qb = wave; qb < NT; qb += NTHR / 64) {
    float q[CH / 2];
#pragma unroll
    for (int s2 = 0; s2 < CH / 2; s2++) q[s2] = base[(size_t)(2 * s2 + hh) * T + 32 * qb + j] * scale2;
    f32x16 sc[NT];
#pragma unroll
    for (int kt = 0; kt < NT; kt++) {
#pragma unroll
      for (int r = 0; r < 16; r++) sc[kt][r] = 0.f;
#pragma unroll
      for (int s2 = 0; s2 < CH / 2; s2++)
        sc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ks[(2 * s2 + hh) * T + 32 * kt + j], q[s2], sc[kt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);                        // keep the LDS operand reads of later tiles from piling up
    }
    // exact softmax over the keys of this lane's query (weights kept unnormalised; 1 / sum applied to the output)
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; kt++)
#pragma unroll
      for (int r = 0; r < 16; r++) mx = fmaxf(mx, sc[kt][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; kt++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        sc[kt][r] = expf(sc[kt][r] - mx);
        l += sc[kt][r];
      }
    l += __shfl_xor(l, 32);
    f32x16 o[2];
#pragma unroll
    for (int ct = 0; ct < 2; ct++)
#pragma unroll
      for (int r = 0; r < 16; r++) o[ct][r] = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; kt++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int key = 32 * kt + rowoff(r, hh);               // the key this lane half holds in register r
#pragma unroll
        for (int ct = 0; ct < 2; ct++)
          o[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(vt[key * VS + 32 * ct + j], sc[kt][r], o[ct], 0, 0, 0);
        if ((r & 7) == 7) __builtin_amdgcn_sched_barrier(0);
      }
    const float inv = 1.0f / l;
    float *op = out + (size_t)bh * CH * T + 32 * qb + j;
#pragma unroll
    for (int ct = 0; ct < 2; ct++)
#pragma unroll
      for (int r = 0; r < 16; r++) op[(size_t)(32 * ct + rowoff(r, hh)) * T] = o[ct][r] * inv;
  }
}

}  // namespace ap

extern "C" int ap_groupnorm_nchw(const float *x, const float *gamma, const float *beta, const float *scale_shift, float *y,
                                 int B, int C, int HW, int groups, float eps, int act, void *stream) {
  if (!x || !gamma || !beta || !y || B < 1 || C < 1 || HW < 1 || groups < 1 || C % groups) { set_error("ap_groupnorm_nchw: bad argument"); return -22; }
  hipStream_t st = (hipStream_t)stream;
  const int slabs = B * groups, n = (C / groups) * HW, n4 = n / 4;
  const bool vec = HW % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0 && !g_conv_tune.no_frag;
#define AP_GN(T, NV)                                                                                                          \
  groupnorm_reg_kernel<T, NV><<<(unsigned)((slabs + 256 / T - 1) / (256 / T)), 256, 0, st>>>(x, gamma, beta, scale_shift, y, C, HW, \
                                                                                            groups, eps, act, slabs)
  if (vec && n4 <= 64) AP_GN(64, 1);
  else if (vec && n4 <= 128) AP_GN(64, 2);
  else if (vec && n4 <= 256) AP_GN(64, 4);
  else if (vec && n4 <= 512) AP_GN(256, 2);
  else if (vec && n4 <= 1024) AP_GN(256, 4);
  else if (vec && n4 <= 2048) AP_GN(256, 8);
  else if (vec && n4 <= 3072) AP_GN(256, 12);
  else if (vec && n4 <= 4096) AP_GN(256, 16);
  else groupnorm_kernel<<<(unsigned)slabs, 256, 0, st>>>(x, gamma, beta, scale_shift, y, C, HW, groups, eps, act);
#undef AP_GN
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_timestep_embedding(const float *t_dev, const float *freqs_dev, float *out, int B, int dim, void *stream) {
  if (!t_dev || !freqs_dev || !out || B < 1 || dim < 2 || dim % 2) { set_error("ap_timestep_embedding: bad argument (even dim only)"); return -22; }
  const int total = B * (dim / 2);
  timestep_embedding_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(t_dev, freqs_dev, out, dim / 2, total);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_silu(const float *x, float *y, size_t n, void *stream) {
  if (!x || !y || n < 1) { set_error("ap_silu: bad argument"); return -22; }
  silu_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, y, n);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_upsample_nearest2x(const float *x, float *y, int BC, int H, int W, void *stream) {
  if (!x || !y || BC < 1 || H < 1 || W < 1) { set_error("ap_upsample_nearest2x: bad argument"); return -22; }
  size_t total = (size_t)BC * 4 * H * W;
  upsample2x_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, y, H, W, total);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_attention_qkv(const float *qkv, float *out, int B, int C, int T, int heads, void *stream) {
  if (!qkv || !out || B < 1 || C < 1 || T < 1 || heads < 1 || C % heads) { set_error("ap_attention_qkv: bad argument"); return -22; }
  const int ch = C / heads;
  const size_t smem = (size_t)2 * ch * T * sizeof(float);
  if (smem > 160 * 1024) { set_error("ap_attention_qkv: K/V of one head (%zu bytes) exceed the LDS", smem); return -22; }
  const float scale2 = 1.0f / sqrtf((float)ch);          // (1/sqrt(sqrt(ch)))^2, unet.py:247-249
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)(B * heads);
  if (ch == 64 && (T == 64 || T == 256) && !g_conv_tune.no_frag) {   // the UNet's shapes: fp32 MFMA
    const size_t sm2 = (size_t)(64 * T + T * 65) * sizeof(float);
    static bool attr2 = false;
    if (!attr2) {
      AP_HIP(hipFuncSetAttribute((const void *)attention_mfma_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      attr2 = true;
    }
    if (T == 64) attention_mfma_kernel<2><<<grid, 256, sm2, st>>>(qkv, out, scale2);
    else attention_mfma_kernel<8><<<grid, 512, sm2, st>>>(qkv, out, scale2);
    AP_HIP(hipGetLastError());
    return 0;
  }
#define AP_ATT(CHV)                                                                                                  \
  do {                                                                                                               \
    static bool attr = false;                                                                                        \
    if (!attr) {                                                                                                     \
      AP_HIP(hipFuncSetAttribute((const void *)attention_kernel<CHV>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); \
      attr = true;                                                                                                   \
    }                                                                                                                \
    attention_kernel<CHV><<<grid, 256, smem, st>>>(qkv, out, T, heads, scale2);                                      \
  } while (0)
  switch (ch) {
    case 8: AP_ATT(8); break;
    case 16: AP_ATT(16); break;
    case 32: AP_ATT(32); break;
    case 64: AP_ATT(64); break;
    default: set_error("ap_attention_qkv: channels per head %d not built (8, 16, 32, 64)", ch); return -22;
  }
#undef AP_ATT
  AP_HIP(hipGetLastError());
  return 0;
}

namespace ap {
__global__ void axpbyc_kernel(const float *__restrict__ x, const float *__restrict__ y, float *__restrict__ out, float a,
                              float b, float c, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a * x[i] + (y ? b * y[i] : 0.f) + c;
}
}  // namespace ap

extern "C" int ap_axpbyc(const float *x, const float *y, float *out, float a, float b, float c, size_t n, void *stream) {
  if (!x || !out || n < 1) { set_error("ap_axpbyc: bad argument"); return -22; }
  ap::axpbyc_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, y, out, a, b, c, n);
  AP_HIP(hipGetLastError());
  return 0;
}

namespace ap {
// GaussianDiffusion.p_sample with epsilon prediction and a fixed variance (gaussian_diffusion.py:232-387):
// pred_x0 = clamp(r1 x - r2 eps, -1, 1); mean = c1 pred_x0 + c2 x; out = mean + sigma z
__global__ void psample_kernel(const float *__restrict__ x, const float *__restrict__ eps, const float *__restrict__ z,
                               float *__restrict__ out, float r1, float r2, float c1, float c2, float sigma, int clip,
                               size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float p = r1 * x[i] - r2 * eps[i];
  if (clip) p = fminf(fmaxf(p, -1.0f), 1.0f);
  float v = c1 * p + c2 * x[i];
  if (z) v += sigma * z[i];
  out[i] = v;
}
}  // namespace ap

extern "C" int ap_psample_update(const float *x, const float *eps, const float *z, float *out, float r1, float r2, float c1,
                                 float c2, float sigma, int clip, size_t n, void *stream) {
  if (!x || !eps || !out || n < 1) { set_error("ap_psample_update: bad argument"); return -22; }
  ap::psample_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, eps, z, out, r1, r2, c1, c2, sigma, clip, n);
  AP_HIP(hipGetLastError());
  return 0;
}
