// gfx950 (MI355X / CDNA4) kernels of the diffusion-purification hot path.
//
// Dominant kernel: resblock_f32_kernel — one DiffWave Residual_block.forward
// (reference: diffusion_models/DiffWave_Unconditional/WaveNet.py:75-97) fused into a single
// launch: FiLM add, dilated k=3 conv as a [2C x 3C].[3C x Tt] GEMM on the exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32), tanh*sigmoid gate in registers, res/skip 1x1 convs as a second
// [(C+S) x C].[C x Tt] GEMM, residual/skip epilogue.  HBM traffic per layer is the algorithmic
// minimum: read h (+halo), write h', read+write skip.
#include "ap_common.h"

namespace ap {

// ---------------------------------------------------------------------------------------------
// weight-norm fold (WaveNet.py:23-34; nn.utils.weight_norm dim=0) and MFMA operand packing
// ---------------------------------------------------------------------------------------------
__global__ void rownorm_kernel(const float *__restrict__ v, float *__restrict__ norm, int O, int IK) {
  int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (row >= O) return;
  const float *p = v + (size_t)row * IK;
  float s = 0.f;
  for (int i = lane; i < IK; i += 64) s = __builtin_fmaf(p[i], p[i], s);
  s = wave_sum(s);
  if (lane == 0) norm[row] = sqrtf(s);
}

// out[o][i] = v[o][i] * (g[o] / ||v[o]||)
__global__ void fold_kernel(const float *__restrict__ g, const float *__restrict__ v,
                            const float *__restrict__ norm, float *__restrict__ out, int O, int IK) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)O * IK) return;
  int o = idx / IK;
  out[idx] = v[idx] * (g[o] / norm[o]);
}

// GEMM1 A image: [wave][group][rowtile 4][lane 64][4]; k-step s = 4*group + e; lane (i, h) holds
// W1[o(wave, rt, i)][kk = 2s + h], kk -> (chunk, tap, c_local) so that the K order matches the
// staged X rows [tap][c_local] of each 16-channel chunk.  Row tiles interleave tanh / sigmoid halves
// so a wave owns both pre-activations of its 64 gate channels.
__global__ void pack_w1_kernel(const float *__restrict__ w1f, float *__restrict__ out, int C) {
  const int NW = C / 64, NG = C * 3 / 8;
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)NW * NG * 4 * 64 * 4;
  if (idx >= total) return;
  int e = idx & 3;
  int lane = (idx >> 2) & 63;
  int rt = (idx >> 8) & 3;
  size_t rest = idx >> 10;
  int G = rest % NG;
  int w = rest / NG;
  int s = 4 * G + e, hh = lane >> 5, i = lane & 31;
  int kk = 2 * s + hh;
  int chunk = kk / (3 * KC), within = kk % (3 * KC);
  int tap = within / KC, cl = within % KC;
  int c = chunk * KC + cl;
  int o = (rt & 1) * C + 64 * w + 32 * (rt >> 1) + i;
  out[idx] = w1f[((size_t)o * C + c) * 3 + tap];
}

// GEMM2 / final-conv A image: [wave][group][rowtile RT][lane][4], rows o = RT*32*wave + 32 rt + i, k = channel.
// mode 1 (GEMM2, RT = 4): wf = [res rows (M/2); skip rows (M/2)]; wave w owns res rows [64w, 64w+64) in row tiles 0,1
// and the skip rows of the same channels in row tiles 2,3.
__global__ void pack_rows_kernel(const float *__restrict__ wf, float *__restrict__ out, int M, int K, int RT,
                                 int mode) {
  const int NG = K / 8;
  const int NWv = M / (32 * RT);
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)NWv * NG * RT * 64 * 4;
  if (idx >= total) return;
  int e = idx & 3;
  int lane = (idx >> 2) & 63;
  size_t rest = idx >> 8;
  int rt = rest % RT;
  rest /= RT;
  int G = rest % NG;
  int w = rest / NG;
  int s = 4 * G + e, hh = lane >> 5, i = lane & 31;
  int kk = 2 * s + hh;
  int o = 32 * RT * w + 32 * rt + i;
  if (mode == 1) o = (rt >> 1) * (M / 2) + 64 * w + 32 * (rt & 1) + i;
  out[idx] = wf[(size_t)o * K + kk];
}

__global__ void copy_kernel(const float *__restrict__ in, float *__restrict__ out, size_t n) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < n) out[idx] = in[idx];
}

static int fold_one(const float *g, const float *v, float *norms, float *out, int O, int IK, hipStream_t st) {
  rownorm_kernel<<<(O + 3) / 4, 256, 0, st>>>(v, norms, O, IK);
  size_t n = (size_t)O * IK;
  fold_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(g, v, norms, out, O, IK);
  return 0;
}

static void copy_to(const float *in, float *out, size_t n, hipStream_t st) {
  copy_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(in, out, n);
}

int launch_fold_and_pack(ap_ctx *ctx, const float *blob, hipStream_t st) {
  const ap_config &c = ctx->cfg;
  const int C = ctx->C, S = ctx->S, NL = ctx->NL;
  BlobLayout bl = blob_layout(c);
  // init conv (in_channels = 1)
  fold_one(blob + bl.init_g, blob + bl.init_v, ctx->norms, ctx->w0, C, 1, st);
  copy_to(blob + bl.init_b, ctx->b0, C, st);
  copy_to(blob + bl.fc1_w, ctx->fc1_w, (size_t)c.embed_dim_mid * c.embed_dim_in, st);
  copy_to(blob + bl.fc1_b, ctx->fc1_b, c.embed_dim_mid, st);
  copy_to(blob + bl.fc2_w, ctx->fc2_w, (size_t)c.embed_dim_out * c.embed_dim_mid, st);
  copy_to(blob + bl.fc2_b, ctx->fc2_b, c.embed_dim_out, st);
  for (int n = 0; n < NL; n++) {
    const float *b = blob + bl.blk0 + (size_t)n * bl.blk_stride;
    copy_to(b + bl.fct_w, ctx->fct_w + (size_t)n * C * c.embed_dim_out, (size_t)C * c.embed_dim_out, st);
    copy_to(b + bl.fct_b, ctx->fct_b + (size_t)n * C, C, st);
    float *w1f = ctx->w1f + (size_t)n * 2 * C * C * 3;
    float *w2f = ctx->w2f + (size_t)n * (C + S) * C;
    fold_one(b + bl.dil_g, b + bl.dil_v, ctx->norms, w1f, 2 * C, C * 3, st);
    fold_one(b + bl.res_g, b + bl.res_v, ctx->norms, w2f, C, C, st);
    fold_one(b + bl.skip_g, b + bl.skip_v, ctx->norms, w2f + (size_t)C * C, S, C, st);
    copy_to(b + bl.dil_b, ctx->b1 + (size_t)n * 2 * C, 2 * C, st);
    copy_to(b + bl.res_b, ctx->b2 + (size_t)n * (C + S), C, st);
    copy_to(b + bl.skip_b, ctx->b2 + (size_t)n * (C + S) + C, S, st);
    size_t n1 = (size_t)2 * C * C * 3, n2 = (size_t)(C + S) * C;
    pack_w1_kernel<<<(unsigned)((n1 + 255) / 256), 256, 0, st>>>(w1f, ctx->w1p + (size_t)n * n1, C);
    pack_rows_kernel<<<(unsigned)((n2 + 255) / 256), 256, 0, st>>>(w2f, ctx->w2p + (size_t)n * n2, C + S, C, 4, 1);
  }
  fold_one(blob + bl.f1_g, blob + bl.f1_v, ctx->norms, ctx->wf1f, S, S, st);
  copy_to(blob + bl.f1_b, ctx->bf1, S, st);
  copy_to(blob + bl.f2_w, ctx->wf2, S, st);
  copy_to(blob + bl.f2_b, ctx->bf2, 1, st);
  size_t nf = (size_t)S * S;
  pack_rows_kernel<<<(unsigned)((nf + 255) / 256), 256, 0, st>>>(ctx->wf1f, ctx->wf1p, S, S, 2, 0);
  AP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------
// diffusion-step embedding MLP + every block's fc_t   (util.py:68-93; WaveNet.py:82-83,124-126)
// The step is shared by the whole batch in every caller (diffwave_ddpm.py:157,169,177).
// ---------------------------------------------------------------------------------------------
// One workgroup of 8 waves = eight rows of fc_t2 (one per wave).  Every workgroup first recomputes all of fc_t1 into LDS -- 65 k
// multiply-adds, wave-per-row dot products, sixteen rows per pass and wave -- so there is no second launch, no scratch buffer and no grid
// barrier.  Every load is UNCONDITIONAL (indices clamped, the product masked): a load inside `if (row < Emid)` sits in its own basic
// block with its own wait, and the sixteen rows of a pass became sixteen round trips (81-115 us; the one-workgroup form that walked each
// weight row with one thread took 45-60 us per evaluation).
__global__ __launch_bounds__(512) void embed_mlp_kernel(const float *__restrict__ freq, const float *__restrict__ w1,
                                                        const float *__restrict__ b1, const float *__restrict__ w2,
                                                        const float *__restrict__ b2, float step, int Ein, int Emid,
                                                        int Eout, float *__restrict__ emb_out) {
  extern __shared__ float sm[];
  float *e0 = sm, *e1 = sm + Ein;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int half = Ein / 2;
  for (int i = threadIdx.x; i < half; i += blockDim.x) {
    float a = step * freq[i];
    e0[i] = sinf(a);
    e0[half + i] = cosf(a);
  }
  __syncthreads();
  for (int o0 = wave; o0 < Emid; o0 += 8 * 16) {
    float s[16];
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = 0.f;
    for (int kk = 0; kk < Ein; kk += 64) {
      const int k = min(kk + lane, Ein - 1);
      const float ev = kk + lane < Ein ? e0[k] : 0.f;             // (a clamped lane contributes 0)
#pragma unroll
      for (int i = 0; i < 16; i++) s[i] = __builtin_fmaf(w1[(size_t)min(o0 + 8 * i, Emid - 1) * Ein + k], ev, s[i]);
    }
    for (int m = 32; m > 0; m >>= 1) {                           // (wave_sum's order, the sixteen butterflies interleaved step by step)
#pragma unroll
      for (int i = 0; i < 16; i++) s[i] += __shfl_xor(s[i], m);
    }
    float mine = 0.f;                                            // lane i takes row i's sum: ONE swish for the sixteen rows
#pragma unroll
    for (int i = 0; i < 16; i++) mine = lane == i ? s[i] : mine;
    const int o = o0 + 8 * lane;
    if (lane < 16 && o < Emid) e1[o] = silu(mine + b1[o]);
  }
  __syncthreads();
  const int o2 = min((int)blockIdx.x * 8 + wave, Eout - 1);      // (a wave past the last row recomputes it and does not store)
  float s = 0.f;
  for (int kk = 0; kk < Emid; kk += 512) {
    float wv[8];
#pragma unroll
    for (int i = 0; i < 8; i++) wv[i] = w2[(size_t)o2 * Emid + min(kk + 64 * i + lane, Emid - 1)];
#pragma unroll
    for (int i = 0; i < 8; i++) s = kk + 64 * i + lane < Emid ? __builtin_fmaf(wv[i], e1[kk + 64 * i + lane], s) : s;
  }
  s = wave_sum(s);
  if (lane == 0 && (int)blockIdx.x * 8 + wave < Eout) emb_out[o2] = silu(s + b2[o2]);
}

// part_t[row] = fct_w[row] . emb + fct_b[row]; one wave per row, rows = NL*C
__global__ void fct_kernel(const float *__restrict__ w, const float *__restrict__ b, const float *__restrict__ emb,
                           float *__restrict__ out, int rows, int E) {
  int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float *p = w + (size_t)row * E;
  float s = 0.f;
  for (int i0 = 0; i0 < E; i0 += 512) {                          // eight loads per operand out together (clamped; a lane past E adds 0), then the sum in order
    float wv[8], ev[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = min(i0 + 64 * u + lane, E - 1);
      wv[u] = p[i];
      ev[u] = emb[i];
    }
#pragma unroll
    for (int u = 0; u < 8; u++) s = i0 + 64 * u + lane < E ? __builtin_fmaf(wv[u], ev[u], s) : s;
  }
  s = wave_sum(s);
  if (lane == 0) out[row] = s + b[row];
}

int launch_embed(ap_ctx *ctx, float step, float *part_t, hipStream_t st) {
  const ap_config &c = ctx->cfg;
  // emb vector lives at the tail of part_t's buffer: [NL*C] then [Eout]
  float *emb = part_t + (size_t)ctx->NL * ctx->C;
  size_t sm = (size_t)(c.embed_dim_in + c.embed_dim_mid) * sizeof(float);
  embed_mlp_kernel<<<(unsigned)((c.embed_dim_out + 7) / 8), 512, sm, st>>>(ctx->emb_freq, ctx->fc1_w, ctx->fc1_b, ctx->fc2_w, ctx->fc2_b, step,
                                       c.embed_dim_in, c.embed_dim_mid, c.embed_dim_out, emb);
  int rows = ctx->NL * ctx->C;
  fct_kernel<<<(rows + 3) / 4, 256, 0, st>>>(ctx->fct_w, ctx->fct_b, emb, part_t, rows, c.embed_dim_out);
  AP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------
// init conv: h[b][c][t] = max(w0[c] x[b][t] + b0[c], 0)     (WaveNet.py:147,168; ReLU :17-19)
// ---------------------------------------------------------------------------------------------
__global__ void init_conv_kernel(const float *__restrict__ x, const float *__restrict__ w0,
                                 const float *__restrict__ b0, float *__restrict__ h, int C, int L) {
  int b = blockIdx.z, c = blockIdx.y;
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= L) return;
  float v = __builtin_fmaf(w0[c], x[(size_t)b * L + t], b0[c]);
  h[((size_t)b * C + c) * L + t] = fmaxf(v, 0.f);
}

int launch_init_conv(ap_ctx *ctx, const float *x, float *h, int B, int L, hipStream_t st) {
  dim3 grid((L + 255) / 256, ctx->C, B);
  init_conv_kernel<<<grid, 256, 0, st>>>(x, ctx->w0, ctx->b0, h, ctx->C, L);
  AP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------
// fused residual block, exact fp32 MFMA
// ---------------------------------------------------------------------------------------------
template <int C, int TTK>
struct RBGeom {
  static constexpr int NWM = C / 64;           // wave rows: wave (mw, nw) owns gate channels [64mw, 64mw+64) ...
  static constexpr int NWN = TTK / 64;         // ... and time columns [64nw, 64nw+64) of the TTK-sample tile
  static constexpr int NW = NWM * NWN;
  static constexpr int NT = NW * 64;           // 512 threads at C = 256: two waves per SIMD
  static constexpr int ROWS = 3 * KC;          // staged K rows per chunk (3 taps x 16 channels)
  static constexpr int NCHUNK = C / KC;
  static constexpr int GPC = ROWS / 8;         // A groups (4 k-steps of 2) per chunk = 6
  static constexpr int NG1 = NCHUNK * GPC;     // = 3C/8
  static constexpr int NG2 = C / 8;
  static constexpr int EPT = ROWS * TTK / NT;   // staged elements per thread per chunk (12 at C = 256)
  static constexpr int RPI = NT / TTK;         // rows advanced per element index
  static constexpr int NPT = KC / RPI;         // distinct channels per thread per chunk
  static constexpr int XBUF = ROWS * TTK;      // floats per X buffer
  static constexpr int LDS_FLOATS = (2 * XBUF > C * TTK) ? 2 * XBUF : C * TTK;
};

// One workgroup = one (utterance, 128-sample tile).  Per wave: 128 GEMM rows x 64 columns = 8 accumulator tiles of
// 32x32 (128 AGPRs), so two waves share each SIMD and one wave's waits/VALU phases overlap the other's MFMAs.
// SAVE (the differentiable path's forward pass, ap_resblock_fwd_save): the pre-gate activations y = DilConv(u) + b are also
// written to aout [B][2C][L] (rows 0..C-1 the tanh half, C..2C-1 the sigmoid half: the layout ap_gate_bwd reads), so the
// backward pass does not recompute the dilated conv.
template <int C, int TTK, bool SAVE = false>
__global__ __launch_bounds__(C / 64 * TTK, 2) void resblock_f32_kernel(
    const float *__restrict__ hin, const float *__restrict__ pt, float *__restrict__ hout, float *__restrict__ skip,
    const float *__restrict__ w1p, const float *__restrict__ b1, const float *__restrict__ w2p,
    const float *__restrict__ b2, int L, int d, int accumulate, int ntiles, float *__restrict__ aout AP_ABLATE_PARAM) {
  AP_ABLATE_DECL
  using G = RBGeom<C, TTK>;
  constexpr int TT = TTK;   // time tile of this kernel (shadows ap::TT)
  constexpr int NT = G::NT;
  __shared__ float lds[G::LDS_FLOATS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mw = wave / G::NWN, nw = wave % G::NWN;
  const int j = lane & 31, hh = lane >> 5;
  int b_, tile_;
  ap_tile_of_block(blockIdx.x, gridDim.x, ntiles, d, TT, b_, tile_);      // XCD-local walk (speed only)
  const int b = __builtin_amdgcn_readfirstlane(b_);
  const int t0 = __builtin_amdgcn_readfirstlane(tile_ * TT);
  const float *hin_b;
  {   // make the per-utterance base provably wave-uniform (buffer descriptor must live in SGPRs)
    const uint64_t hb = (uint64_t)(hin + (size_t)b * C * L);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)hb);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(hb >> 32));
    hin_b = (const float *)(((uint64_t)hi << 32) | lo);
  }

  f32x16 acc[4][2];
  // accumulators start from the dilated conv's bias; row tiles interleave tanh (even rt) / sigmoid (odd rt) halves
#pragma unroll
  for (int rt = 0; rt < 4; rt++) {
    const int obase = (rt & 1) * C + 64 * mw + 32 * (rt >> 1);
#pragma unroll
    for (int q = 0; q < 4; q++) {                                // rows rowoff(4q .. 4q+3, hh) are consecutive
      const float4 bv = *reinterpret_cast<const float4 *>(b1 + obase + 8 * q + 4 * hh);
#pragma unroll
      for (int ct = 0; ct < 2; ct++) {
        acc[rt][ct][4 * q + 0] = bv.x;
        acc[rt][ct][4 * q + 1] = bv.y;
        acc[rt][ct][4 * q + 2] = bv.z;
        acc[rt][ct][4 * q + 3] = bv.w;
      }
    }
  }

  // ---- staging of X = [tap][c_local][t] chunks through registers: buffer loads with 32-bit offsets issued at
  // the head of a chunk, FiLM add + zero-pad select + ds_write at its tail (one barrier per chunk).
  // Element i of a thread sits at LDS index i*NT + tid = (row i*RPI + rsel, col tid % TT).
  constexpr int RPI = G::RPI, NPT = G::NPT;
  const int rsel = tid / TT;
  unsigned voff[3];
  bool tok[3];
#pragma unroll
  for (int tap = 0; tap < 3; tap++) {
    const int tp = t0 + (tid & (TT - 1)) + (tap - 1) * d;
    tok[tap] = (tp >= 0) && (tp < L);
    voff[tap] = ((unsigned)min(max(tp, 0), L - 1) + (unsigned)rsel * (unsigned)L) * 4u;
  }
  const __amdgpu_buffer_rsrc_t hrs =
      __builtin_amdgcn_make_buffer_rsrc((void *)hin_b, 0, (int)((unsigned)C * (unsigned)L * 4u), 0x00020000);
  float xr[G::EPT];
  float ptv[NPT];
  auto issue_loads = [&](int ch) {
#pragma unroll
    for (int q = 0; q < NPT; q++) ptv[q] = pt[ch * KC + q * RPI + rsel];
#pragma unroll
    for (int i = 0; i < G::EPT; i++) {
      const int rowc = i * RPI;                                // compile-time part of the row
      const int tap = rowc / KC, clc = rowc % KC;
      const int soff = (ch * KC + clc) * L * 4;                // wave-uniform
      xr[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(hrs, voff[tap], soff, 0));
    }
  };
  auto store_chunk = [&](float *dst) {
#pragma unroll
    for (int i = 0; i < G::EPT; i++) {
      const int rowc = i * RPI;
      const int tap = rowc / KC, clc = rowc % KC;
      const float u = xr[i] + ptv[clc / RPI];                  // u = h + part_t (WaveNet.py:84)
      dst[i * NT + tid] = tok[tap] ? u : 0.f;                  // zero padding of the conv input (WaveNet.py:26-27)
    }
  };

  issue_loads(0);
  store_chunk(lds);
  __syncthreads();

  // A operands (weights) stream straight from L2 into registers, one group (4 k-steps x 4 row tiles = 16 VGPRs)
  // ahead of its use, ping-ponging between two named register sets so no copy or early wait is needed.
  auto load_a = [&](f32x4(&a)[4], const f32x4 *base, int Gi) {
#pragma unroll
    for (int rt = 0; rt < 4; rt++) a[rt] = base[(size_t)((ablate & 4) ? 0 : Gi) * 256 + rt * 64];
  };
  auto mma4 = [&](const f32x4(&a)[4], const float *xb) {      // 4 k-steps: 8 LDS reads, 32 MFMAs
    float bv[4][2];
#pragma unroll
    for (int e = 0; e < 4; e++)
#pragma unroll
      for (int ct = 0; ct < 2; ct++) bv[e][ct] = xb[e * 2 * TT + 32 * ct];
#pragma unroll
    for (int e = 0; e < 4; e++)
#pragma unroll
      for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int ct = 0; ct < 2; ct++)
          acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[rt][e], bv[e][ct], acc[rt][ct], 0, 0, 0);
  };

  const int colbase = 64 * nw + j;
  const f32x4 *ap = reinterpret_cast<const f32x4 *>(w1p) + (size_t)mw * G::NG1 * 4 * 64 + lane;
  f32x4 a0[4], a1[4];
  load_a(a0, ap, 0);
  {
    static_assert(G::GPC % 2 == 0 && G::NG1 % 2 == 0, "pair-unrolled loop");
    int ch = 0, g = 0;
#pragma unroll 1
    for (int Gi = 0; Gi < G::NG1; Gi += 2) {
      // vmcnt retires in issue order: the next weight group is requested BEFORE the (HBM-latency) X loads of the next
      // chunk, so its wait does not include them
      load_a(a1, ap, Gi + 1);
      if (g == 0 && ch + 1 < G::NCHUNK && !(ablate & 8)) issue_loads(ch + 1);
      __builtin_amdgcn_sched_barrier(0);
      const float *xb = lds + (ch & 1) * G::XBUF + (g * 8 + hh) * TT + colbase;
      mma4(a0, xb);
      __builtin_amdgcn_sched_barrier(0);
      load_a(a0, ap, (Gi + 2 < G::NG1) ? Gi + 2 : Gi);          // last pair re-reads its own group (unused)
      __builtin_amdgcn_sched_barrier(0);
      mma4(a1, xb + 8 * TT);
      __builtin_amdgcn_sched_barrier(0);
      g += 2;
      if (g == G::GPC) {
        if (ch + 1 < G::NCHUNK) store_chunk(lds + ((ch + 1) & 1) * G::XBUF);
        __syncthreads();
        g = 0;
        ch++;
      }
    }
  }

  // gated non-linearity (WaveNet.py:90); g -> LDS [C][TT] (aliases the X buffers: all reads retired by the barrier)
#pragma unroll
  for (int p = 0; p < 2; p++)
#pragma unroll
    for (int ct = 0; ct < 2; ct++) {
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int c = 64 * mw + 32 * p + rowoff(r, hh);
        if constexpr (SAVE) {
          const int t = t0 + 32 * ct + colbase;
          if (t < L) {
            float *ab = aout + ((size_t)b * 2 * C + c) * L + t;
            ab[0] = acc[2 * p][ct][r];
            ab[(size_t)C * L] = acc[2 * p + 1][ct][r];
          }
        }
        lds[c * TT + 32 * ct + colbase] =
            (ablate & 2) ? acc[2 * p][ct][r] : gate(acc[2 * p][ct][r], acc[2 * p + 1][ct][r]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }

  // GEMM2: row tiles 0,1 = res_conv rows of this wave's 64 channels, row tiles 2,3 = skip_conv rows of the same
  // channels.  Accumulators start from b_res + part_t (u = h + part_t re-enters the residual) / b_skip.  The pointers
  // are laundered through an empty asm so these loads cannot be hoisted above the main loop.
  {
    const float *b2l = b2, *ptl = pt;
    asm volatile("" : "+s"(b2l), "+s"(ptl));
#pragma unroll
    for (int rt = 0; rt < 4; rt++) {
      const int cb = 64 * mw + 32 * (rt & 1);
#pragma unroll
      for (int q = 0; q < 4; q++) {                              // rows rowoff(4q .. 4q+3, hh) are consecutive: one 16-B load
        const int c = cb + 8 * q + 4 * hh;
        float4 bv = *reinterpret_cast<const float4 *>(b2l + (rt < 2 ? 0 : C) + c);
        if (rt < 2) {
          const float4 pv = *reinterpret_cast<const float4 *>(ptl + c);
          bv.x += pv.x; bv.y += pv.y; bv.z += pv.z; bv.w += pv.w;
        }
#pragma unroll
        for (int ct = 0; ct < 2; ct++) {
          acc[rt][ct][4 * q + 0] = bv.x;
          acc[rt][ct][4 * q + 1] = bv.y;
          acc[rt][ct][4 * q + 2] = bv.z;
          acc[rt][ct][4 * q + 3] = bv.w;
        }
      }
    }
  }
  const f32x4 *ap2 = reinterpret_cast<const f32x4 *>(w2p) + (size_t)mw * G::NG2 * 4 * 64 + lane;
  load_a(a0, ap2, 0);                                            // ahead of the residual-input loads below (in-order vmcnt)
  load_a(a1, ap2, 1);
  __syncthreads();

  // The residual input h[c][t] of this wave's 64 x 64 patch is fetched now (64 VGPRs) and consumed after GEMM2,
  // so the epilogue never waits on memory; the skip half needs no read at all (float atomics at the memory side).
  float hres[2][2][16];
  unsigned evoff[2][2];
#pragma unroll
  for (int rt = 0; rt < 2; rt++)
#pragma unroll
    for (int ct = 0; ct < 2; ct++) {
      const int t = min(t0 + 32 * ct + colbase, L - 1);
      evoff[rt][ct] = ((unsigned)(64 * mw + 32 * rt + 4 * hh) * (unsigned)L + (unsigned)t) * 4u;
    }
  if (!(ablate & 1)) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
      for (int ct = 0; ct < 2; ct++)
#pragma unroll
        for (int r = 0; r < 16; r++)
          hres[rt][ct][r] = __builtin_bit_cast(
              float, __builtin_amdgcn_raw_buffer_load_b32(hrs, evoff[rt][ct], rowoff(r, 0) * L * 4, 2));   // nt: hits or passes without allocating
  }

  {
    static_assert(G::NG2 % 2 == 0, "pair-unrolled loop");
#pragma unroll 1
    for (int Gi = 0; Gi < G::NG2; Gi += 2) {
      const float *gb = lds + (Gi * 8 + hh) * TT + colbase;
      mma4(a0, gb);
      __builtin_amdgcn_sched_barrier(0);
      load_a(a0, ap2, (Gi + 2 < G::NG2) ? Gi + 2 : Gi);
      __builtin_amdgcn_sched_barrier(0);
      mma4(a1, gb + 8 * TT);
      __builtin_amdgcn_sched_barrier(0);
      load_a(a1, ap2, (Gi + 3 < G::NG2) ? Gi + 3 : Gi + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // epilogue (WaveNet.py:97, :133)
  if (ablate & 1) return;
  const float RS = 0.707106781186547524f;   // float(math.sqrt(0.5))
  float *ho = hout + (size_t)b * C * L;
  float *sk = skip + (size_t)b * C * L;     // S == C
#pragma unroll
  for (int rt = 0; rt < 4; rt++) {
#pragma unroll
    for (int ct = 0; ct < 2; ct++) {
      const int t = t0 + 32 * ct + colbase;
      const unsigned rbase = (unsigned)(64 * mw + 32 * (rt & 1) + 4 * hh) * (unsigned)L + (unsigned)t;
      if (t < L) {
        if (rt < 2) {
#pragma unroll
          for (int r = 0; r < 16; r++)
            // nt (also the skip store below): once-written streams must not displace the h rows in the XCD's L2, which
            // neighbouring tiles' taps and the residual read again
            __builtin_nontemporal_store((hres[rt][ct][r] + acc[rt][ct][r]) * RS, &ho[rbase + (unsigned)rowoff(r, 0) * (unsigned)L]);
        } else if (accumulate) {
#pragma unroll
          for (int r = 0; r < 16; r++)
            unsafeAtomicAdd(&sk[rbase + (unsigned)rowoff(r, 0) * (unsigned)L], acc[rt][ct][r]);
        } else {
#pragma unroll
          for (int r = 0; r < 16; r++) __builtin_nontemporal_store(acc[rt][ct][r], &sk[rbase + (unsigned)rowoff(r, 0) * (unsigned)L]);
        }
      }
    }
  }
}

#ifdef AP_TOOLS
BlockTune g_block_tune;        // the block-dispatch switches (ap_block_plan.h), written by the ap_debug_* hooks
static int g_ablate = 0;       // timing-only ablation mask (ap_debug_ablate)
// tools/csrc/ap_resblock_bf16.hip: kernels that are never planned, tried first where a switch asks; 1: the plan serves the launch
int try_resblock_bf16_tools(ap_ctx *ctx, int layer, const float *hin, const float *pt, float *hout, float *skip, int accumulate, int B, int L, hipStream_t st);
#endif

// the direct-form fp32 block: exactly the instantiations the plan can name (C = 64 with SAVE: 64-sample tiles only; C = 128: no SAVE)
static int launch_block_f32(ap_ctx *ctx, const BlockPlan &p, int layer, const float *hin, const float *pt, float *hout, float *skip, int accumulate,
                            int L, hipStream_t st, float *aout) {
  const int C = ctx->C, S = ctx->S;
  const float *w1p = ctx->w1p + (size_t)layer * 2 * C * C * 3, *w2p = ctx->w2p + (size_t)layer * (C + S) * C;
  const float *b1 = ctx->b1 + (size_t)layer * 2 * C, *b2 = ctx->b2 + (size_t)layer * (C + S);
#define AP_RB(CC, TK, SV)                                                                                                       \
  if (C == CC && p.tile == TK && p.save == SV)                                                                                  \
    resblock_f32_kernel<CC, TK, SV><<<p.grid, p.wg, 0, st>>>(hin, pt, hout, skip, w1p, b1, w2p, b2, L, p.d, accumulate, p.ntiles, \
                                                             SV ? aout : nullptr AP_ABLATE_ARG(g_ablate))
  AP_RB(256, 64, true); AP_RB(256, 128, true); AP_RB(64, 64, true);
  AP_RB(64, 64, false); AP_RB(64, 128, false); AP_RB(128, 64, false); AP_RB(128, 128, false); AP_RB(256, 64, false); AP_RB(256, 128, false);
#undef AP_RB
  AP_HIP(hipGetLastError());
  return 0;
}

int launch_resblock(ap_ctx *ctx, int layer, const float *hin, const float *pt, float *hout, float *skip,
                    int accumulate, int B, int L, hipStream_t st, float *aout, void *gout, void *fout) {
  int refused;
  const BlockPlan &p = planned_block(ctx, layer, B, L, hout, skip, aout, gout, fout, false, &refused);
  if (refused) return refused;
  ProfileSpan span;
  if (int e = span.begin(ctx, 0, st)) return e;
  int rc = 1;
#ifdef AP_TOOLS
  if (p.family == BLOCK_BF16_P && !gout) rc = try_resblock_bf16_tools(ctx, layer, hin, pt, hout, skip, accumulate, B, L, st);
#endif
  if (rc == 1) switch (p.family) {
    case BLOCK_F32_DIRECT: rc = launch_block_f32(ctx, p, layer, hin, pt, hout, skip, accumulate, L, st, aout); break;
    case BLOCK_F32_F23: rc = launch_block_f32w(ctx, p, layer, hin, pt, hout, skip, accumulate, L, st, aout); break;
    case BLOCK_SPLIT_DIRECT: rc = launch_block_split(ctx, p, layer, hin, pt, hout, skip, accumulate, L, st); break;
    case BLOCK_SPLIT_F23: rc = launch_block_split23(ctx, p, layer, hin, pt, hout, skip, accumulate, L, st); break;
    case BLOCK_BF16_P: rc = launch_block_bf16p(ctx, p, layer, hin, pt, hout, skip, accumulate, L, st, gout, fout); break;
    default: rc = launch_block_bf16s(ctx, p, layer, hin, pt, hout, gout, L, st); break;   // BLOCK_BF16_S (the u families: launch_resblock_bf16u)
  }
  if (int e = span.end()) return e;
  return rc;
}

// ---------------------------------------------------------------------------------------------
// counter-based noise: Philox4x32-10 + Box-Muller, keyed on (seed; quad, draw, global utterance)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox_normal4(uint64_t seed, uint32_t draw, uint64_t utt, uint32_t quad,
                                               float (&z)[4]) {
  uint32_t r[4];
  philox4x32_10(quad, draw, (uint32_t)utt, (uint32_t)(utt >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
  const float TWO_PI = 6.283185307179586f;
#pragma unroll
  for (int p = 0; p < 2; p++) {
    float u1 = ((float)(r[2 * p] >> 9) + 0.5f) * 1.1920928955078125e-07f;      // (0,1), 2^-23
    float u2 = (float)(r[2 * p + 1] >> 8) * 5.9604644775390625e-08f;           // [0,1), 2^-24
    float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(TWO_PI * u2, &sn, &cs);
    z[2 * p] = rad * cs;
    z[2 * p + 1] = rad * sn;
  }
}

__device__ __forceinline__ float philox_normal1(uint64_t seed, uint32_t draw, uint64_t utt, int t) {
  float z[4];
  philox_normal4(seed, draw, utt, (uint32_t)t >> 2, z);
  return z[t & 3];
}

// out = ca*x + cs*z    (q-sample, diffwave_ddpm.py:66-67)
__global__ void affine_noise_kernel(const float *__restrict__ x, float *__restrict__ out, float ca, float cs,
                                    const float *__restrict__ z, uint64_t seed, uint32_t draw, uint64_t utt_offset,
                                    int L) {
  const int b = blockIdx.y;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;   // quad of samples
  const int t = q * 4;
  if (t >= L) return;
  float zz[4];
  if (z == nullptr) {
    if (cs != 0.f) philox_normal4(seed, draw, utt_offset + b, (uint32_t)q, zz);
    else zz[0] = zz[1] = zz[2] = zz[3] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (t + i < L) {
      const size_t off = (size_t)b * L + t + i;
      float zv = z ? z[off] : zz[i];
      float xv = x ? x[off] : 0.f;
      out[off] = ca * xv + cs * zv;
    }
  }
}

int launch_affine_noise(const float *x, float *out, float ca, float cs, const float *z, uint64_t seed,
                        uint32_t draw, uint64_t utt_offset, int B, int L, hipStream_t st) {
  int quads = (L + 3) / 4;
  dim3 grid((quads + 255) / 256, B);
  affine_noise_kernel<<<grid, 256, 0, st>>>(x, out, ca, cs, z, seed, draw, utt_offset, L);
  AP_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------
// final_conv + clip update:  eps = W_f2 relu(W_f1 (skip * sqrt(1/N)) + b_f1) + b_f2;  out = ca x + cb eps + cs z
// (WaveNet.py:135,160-162,170; diffwave_ddpm.py:159-160,99-102)
// ---------------------------------------------------------------------------------------------
// FT = columns per workgroup: 64 at S = 256 so that two workgroups share a CU (64 KB of LDS each) and one's staging
// runs under the other's MFMAs.
template <int S, int FT>
__global__ __launch_bounds__(S / 64 * 64, FT == 64 ? 2 : 1) void final_f32_kernel(
    const float *__restrict__ skip, const float *__restrict__ x, float *__restrict__ eps_out, float *__restrict__ out,
    const float *__restrict__ wf1p, const float *__restrict__ bf1, const float *__restrict__ wf2,
    const float *__restrict__ bf2, float scale, float ca, float cb, float cs, const float *__restrict__ z,
    uint64_t seed, uint32_t draw, uint64_t utt_offset, int L, int ntiles) {
  constexpr int NW = S / 64, NT = NW * 64, NG = S / 8;
  constexpr int TT = FT, NCT = FT / 32;                        // shadows ap::TT
  __shared__ float lds[S * TT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, hh = lane >> 5;
  const int b = blockIdx.x / ntiles;
  const int t0 = (blockIdx.x % ntiles) * TT;
  const float *sk = skip + (size_t)b * S * L;

  // stage skip * sqrt(1/N)  ->  lds[S][TT]
  for (int e = tid; e < S * TT; e += NT) {
    const int row = e / TT, col = e % TT;
    const int t = t0 + col;
    lds[e] = (t < L) ? sk[(size_t)row * L + t] * scale : 0.f;
  }
  f32x16 acc[2][NCT];
#pragma unroll
  for (int rt = 0; rt < 2; rt++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      float bv = bf1[64 * wave + 32 * rt + rowoff(r, hh)];
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) acc[rt][ct][r] = bv;
    }
  __syncthreads();

  const f32x4 *ap = reinterpret_cast<const f32x4 *>(wf1p) + (size_t)wave * NG * 2 * 64 + lane;
  f32x4 a_cur[2], a_nxt[2];
  a_cur[0] = ap[0];
  a_cur[1] = ap[64];
#pragma unroll 2
  for (int Gi = 0; Gi < NG; Gi++) {
    if (Gi + 1 < NG) {
      a_nxt[0] = ap[(size_t)(Gi + 1) * 128];
      a_nxt[1] = ap[(size_t)(Gi + 1) * 128 + 64];
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int s = Gi * 4 + e;
      float bv[NCT];
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) bv[ct] = lds[(2 * s + hh) * TT + 32 * ct + j];
#pragma unroll
      for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int ct = 0; ct < NCT; ct++)
          acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[rt][e], bv[ct], acc[rt][ct], 0, 0, 0);
    }
    a_cur[0] = a_nxt[0];
    a_cur[1] = a_nxt[1];
  }
  // relu, dot with W_f2 over this wave's 64 rows
  float part[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) part[ct] = 0.f;
#pragma unroll
  for (int rt = 0; rt < 2; rt++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float w = wf2[64 * wave + 32 * rt + rowoff(r, hh)];
#pragma unroll
      for (int ct = 0; ct < NCT; ct++) part[ct] = __builtin_fmaf(fmaxf(acc[rt][ct][r], 0.f), w, part[ct]);
    }
#pragma unroll
  for (int ct = 0; ct < NCT; ct++) part[ct] += __shfl_xor(part[ct], 32);
  __syncthreads();   // all MFMA reads of lds retired
  if (hh == 0) {
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) lds[wave * TT + 32 * ct + j] = part[ct];
  }
  __syncthreads();
  for (int col = tid; col < TT; col += NT) {
    const int t = t0 + col;
    if (t < L) {
      float e = bf2[0];
#pragma unroll
      for (int w = 0; w < NW; w++) e += lds[w * TT + col];
      const size_t off = (size_t)b * L + t;
      if (eps_out) eps_out[off] = e;
      if (out) {
        float v = ca * x[off] + cb * e;
        if (cs != 0.f) {
          float zv = z ? z[off] : philox_normal1(seed, draw, utt_offset + b, t);
          v += cs * zv;
        }
        out[off] = v;
      }
    }
  }
}

// The same final_conv + update with bf16 MFMA operands (AP_PREC_BF16; fp32 accumulate, fp32 skip in HBM): at S = 256 the
// fp32 kernel above is MFMA-bound (1.07 TFLOP per 512-clip launch on the fp32 pipe = 13.8 ms, 3.7 % of a bf16 step); on the
// bf16 pipe the launch is bound by reading skip once.  4 waves x 64 rows, 64-column tiles, two workgroups per CU; skip is
// staged as a bf16 [column][channel] image (528-B rows: conflict-free ds_read_b128 B fragments).
typedef __bf16 fb16x8 __attribute__((ext_vector_type(8)));
__global__ __launch_bounds__(256, 2) void final_bf16_kernel(
    const float *__restrict__ skip, const float *__restrict__ x, float *__restrict__ eps_out, float *__restrict__ out,
    const fb16x8 *__restrict__ wfp, const float *__restrict__ bf1, const float *__restrict__ wf2,
    const float *__restrict__ bf2, float scale, float ca, float cb, float cs, const float *__restrict__ z, uint64_t seed,
    uint32_t draw, uint64_t utt_offset, int L, int ntiles) {
  constexpr int S = 256, FT = 64, NW = 4, RB = S * 2 + 16, NKS = S / 16;
  __shared__ __attribute__((aligned(16))) unsigned char img[FT * RB];
  __shared__ float red[NW * FT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, hh = lane >> 5;
  const int b = blockIdx.x / ntiles;
  const int t0 = (blockIdx.x % ntiles) * FT;
  const float *sk = skip + (size_t)b * S * L;
  // stage skip * sqrt(1/N) -> bf16 image; item = (column quad cq of 16, channel octet oct of 32): 4 samples x 8 channels
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const int item = tid + 256 * r, cq = item & 15, oct = item >> 4;
    const int t = t0 + 4 * cq;
    float v[8][4];
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const float *row = sk + (size_t)(oct * 8 + e) * L;
      if ((L & 3) == 0) {
        const float4 q = t < L ? *reinterpret_cast<const float4 *>(row + t) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[e][0] = q.x; v[e][1] = q.y; v[e][2] = q.z; v[e][3] = q.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) v[e][i] = t + i < L ? row[t + i] : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      fb16x8 pk;
#pragma unroll
      for (int e = 0; e < 8; e++) pk[e] = (__bf16)(v[e][i] * scale);
      *reinterpret_cast<fb16x8 *>(img + (4 * cq + i) * RB + oct * 16) = pk;
    }
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int rt = 0; rt < 2; rt++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float bv = bf1[64 * wave + 32 * rt + rowoff(r, hh)];
      acc[rt][0][r] = bv;
      acc[rt][1][r] = bv;
    }
  __syncthreads();
  // image [wave][rowtile 2][kstep 16][lane][8 bf16]; fragments two k-steps ahead
  const fb16x8 *ap = wfp + (size_t)(wave * 2) * NKS * 64 + lane;
  fb16x8 a0[2], a1[2], a2[2];
  a0[0] = ap[0]; a0[1] = ap[NKS * 64];
  a1[0] = ap[64]; a1[1] = ap[NKS * 64 + 64];
  const unsigned char *bp = img + j * RB + 16 * hh;
  auto kstep = [&](const fb16x8(&a)[2], int ks) {
    fb16x8 bv[2];
#pragma unroll
    for (int ct = 0; ct < 2; ct++) bv[ct] = *reinterpret_cast<const fb16x8 *>(bp + (32 * ct) * RB + ks * 32);
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
      for (int ct = 0; ct < 2; ct++) acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rt], bv[ct], acc[rt][ct], 0, 0, 0);
  };
  auto fetch = [&](fb16x8(&a)[2], int ks) {
    const int k2 = ks < NKS ? ks : NKS - 1;
    a[0] = ap[k2 * 64];
    a[1] = ap[NKS * 64 + k2 * 64];
  };
#pragma unroll 1
  for (int ks = 0; ks < NKS; ks += 3) {                         // 16 k-steps: 5 rounds of 3 + 1
    fetch(a2, ks + 2);
    kstep(a0, ks);
    if (ks + 1 < NKS) {
      fetch(a0, ks + 3);
      kstep(a1, ks + 1);
    }
    if (ks + 2 < NKS) {
      fetch(a1, ks + 4);
      kstep(a2, ks + 2);
    }
  }
  // relu, dot with W_f2 over this wave's 64 rows
  float part[2] = {0.f, 0.f};
#pragma unroll
  for (int rt = 0; rt < 2; rt++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const float w = wf2[64 * wave + 32 * rt + rowoff(r, hh)];
#pragma unroll
      for (int ct = 0; ct < 2; ct++) part[ct] = __builtin_fmaf(fmaxf(acc[rt][ct][r], 0.f), w, part[ct]);
    }
#pragma unroll
  for (int ct = 0; ct < 2; ct++) part[ct] += __shfl_xor(part[ct], 32);
  if (hh == 0) {
#pragma unroll
    for (int ct = 0; ct < 2; ct++) red[wave * FT + 32 * ct + j] = part[ct];
  }
  __syncthreads();
  if (tid < FT) {
    const int t = t0 + tid;
    if (t < L) {
      float e = bf2[0];
#pragma unroll
      for (int w = 0; w < NW; w++) e += red[w * FT + tid];
      const size_t off = (size_t)b * L + t;
      if (eps_out) eps_out[off] = e;
      if (out) {
        float v = ca * x[off] + cb * e;
        if (cs != 0.f) {
          const float zv = z ? z[off] : philox_normal1(seed, draw, utt_offset + b, t);
          v += cs * zv;
        }
        out[off] = v;
      }
    }
  }
}

int launch_final_affine(ap_ctx *ctx, const float *skip, const float *x, float *eps_out, float *out, float ca,
                        float cb, float cs, const float *z, uint64_t seed, uint32_t draw, uint64_t utt_offset,
                        int B, int L, hipStream_t st) {
  BlockPlan p;                                                   // bf16 modes: the 1x1 convs of final_conv on the bf16 pipe as well
  if (int e = plan_refused(final_plan(block_ask(ctx, 0, B, L), &p), p)) return e;
  const float scale = (float)sqrt(1.0 / (double)ctx->NL);      // math.sqrt(1.0/N) (WaveNet.py:135)
#define AP_FINAL(SS, FTV)                                                                                                \
  final_f32_kernel<SS, FTV><<<p.grid, p.wg, 0, st>>>(skip, x, eps_out, out, ctx->wf1p, ctx->bf1, ctx->wf2, ctx->bf2, scale, \
                                                     ca, cb, cs, z, seed, draw, utt_offset, L, p.ntiles)
  if (p.family == BLOCK_FINAL_BF16)
    final_bf16_kernel<<<p.grid, p.wg, 0, st>>>(skip, x, eps_out, out, (const fb16x8 *)ctx->wf1p_bf, ctx->bf1, ctx->wf2, ctx->bf2, scale, ca, cb, cs, z,
                                               seed, draw, utt_offset, L, p.ntiles);
  else if (ctx->S == 64) AP_FINAL(64, BLOCK_TT);
  else if (ctx->S == 128) AP_FINAL(128, BLOCK_TT);
  else AP_FINAL(256, BLOCK_FT);
#undef AP_FINAL
  AP_HIP(hipGetLastError());
  return 0;
}

// ---- NES queries of the black-box attack (robustness_eval/_NES.py:14-55) with counter-based noise ----------------
// copy s of audio a: lead (s == 0 when `lead`) is the unperturbed audio, then S/2 copies x + sigma z_p and S/2 copies
// x - sigma z_p (antithetic pairs, :19-23); z_p = Philox(seed, draw, a * S/2 + p) is regenerated by the gradient
// kernel, so the [A][S][L] noise tensor of the reference never exists.
__global__ void nes_perturb_kernel(const float *__restrict__ x, float *__restrict__ out, float sigma, uint64_t seed,
                                   uint32_t draw, int S, int lead, int L) {
  const int a = blockIdx.z, s = blockIdx.y;                     // s over S + lead copies
  const int q = blockIdx.x * blockDim.x + threadIdx.x, t = 4 * q;
  if (t >= L) return;
  const int half = S / 2, sp = s - lead;
  float zz[4] = {0.f, 0.f, 0.f, 0.f};
  float sgn = 0.f;
  if (sp >= 0) {
    const int p = sp < half ? sp : sp - half;
    sgn = sp < half ? sigma : -sigma;
    philox_normal4(seed, draw, (uint64_t)a * half + p, (uint32_t)q, zz);
  }
  const float *xa = x + (size_t)a * L;
  float *o = out + ((size_t)a * (S + lead) + s) * L;
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (t + i < L) o[t + i] = __builtin_fmaf(sgn, zz[i], xa[t + i]);
}

// grad[a][t] (+)= (1/S) sum_p (loss[a][p] - loss[a][p + S/2]) z_p[t]    (:44-48: mean over copies of loss * noise)
__global__ void nes_grad_kernel(const float *__restrict__ loss, float *__restrict__ grad, uint64_t seed, uint32_t draw,
                                int S, int L, int accumulate) {
  const int a = blockIdx.y;
  const int q = blockIdx.x * blockDim.x + threadIdx.x, t = 4 * q;
  if (t >= L) return;
  const int half = S / 2;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < half; p++) {
    float zz[4];
    philox_normal4(seed, draw, (uint64_t)a * half + p, (uint32_t)q, zz);
    const float w = loss[(size_t)a * S + p] - loss[(size_t)a * S + half + p];
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = __builtin_fmaf(w, zz[i], acc[i]);
  }
  float *g = grad + (size_t)a * L;
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (t + i < L) g[t + i] = (accumulate ? g[t + i] : 0.f) + acc[i] / (float)S;
}

__global__ void philox_fill_kernel(float *__restrict__ out, uint64_t seed, uint32_t draw, uint64_t utt_offset,
                                   int L) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < L) out[(size_t)b * L + t] = philox_normal1(seed, draw, utt_offset + b, t);
}

}  // namespace ap

#ifdef AP_TOOLS
extern "C" int ap_debug_tile(int tile) {
  if (tile != 64 && tile != 128) return -22;
  ap::g_block_tune.tile = tile;
  return 0;
}

extern "C" int ap_debug_force_f32(int on) {
  ap::g_block_tune.force_f32 = on;
  return 0;
}

extern "C" int ap_debug_no_bf16s(int on) {                       // 1: small bf16 launches stay on the persistent kernel
  ap::g_block_tune.no_bf16s = on;
  return 0;
}

namespace ap { extern int g_ablate_bf16; extern int g_dbg_bf16; extern unsigned long long *g_trace_bf16; }
extern "C" int ap_debug_bf16_dbg(int bits) {
  ap::g_dbg_bf16 = bits;
  return 0;
}

// timing-only: device buffer (nblk x 2 x 16 u64) the bf16 residual block writes phase timestamps into; null = off
extern "C" int ap_debug_trace(void *buf) {
  ap::g_trace_bf16 = (unsigned long long *)buf;
  return 0;
}

extern "C" int ap_debug_ablate(int mask) {
  ap::g_ablate = mask;
  ap::g_ablate_bf16 = mask;
  return 0;
}
#endif  // AP_TOOLS

extern "C" int ap_nes_perturb(const float *x, float *out, float sigma, uint64_t seed, uint32_t draw, int A, int S,
                              int lead, int L, void *stream) {
  if (!x || !out || A < 1 || S < 2 || (S & 1) || L < 1 || lead < 0 || lead > 1) { ap::set_error("ap_nes_perturb: bad argument"); return -22; }
  dim3 grid((unsigned)(((L + 3) / 4 + 255) / 256), (unsigned)(S + lead), (unsigned)A);
  ap::nes_perturb_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(x, out, sigma, seed, draw, S, lead, L);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_nes_grad(const float *loss, float *grad, uint64_t seed, uint32_t draw, int A, int S, int L,
                           int accumulate, void *stream) {
  if (!loss || !grad || A < 1 || S < 2 || (S & 1) || L < 1) { ap::set_error("ap_nes_grad: bad argument"); return -22; }
  dim3 grid((unsigned)(((L + 3) / 4 + 255) / 256), (unsigned)A);
  ap::nes_grad_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(loss, grad, seed, draw, S, L, accumulate);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_philox_normal(float *out, uint64_t seed, uint32_t draw, uint64_t utt_offset, int B, int L,
                                void *stream) {
  dim3 grid((L + 255) / 256, B);
  ap::philox_fill_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(out, seed, draw, utt_offset, L);
  AP_HIP(hipGetLastError());
  return 0;
}
