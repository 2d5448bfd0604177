// Parameter gradients of the DiffWave eps-network (the reference trains it with diffusion_models/DiffWave_Unconditional/
// util.py:161-185 `training_loss`, loss.backward() and Adam in train.py).  The input-gradient sweep (ap_resblock_bwd.hip,
// ap_backward.hip) already forms every cotangent; what is here contracts a cotangent with an activation over (clip, time):
//   ap_wgrad_corr       G[m][n][k] (+)= scale sum_{b,t} P[b][m][t] Q~[b][n][t + (k - taps/2) dil]   on the exact-fp32 matrix instruction
//   ap_rowsum           out[m] (+)= scale sum_{b,t} A[b][m][t] w(b, m, t)                            (biases, FiLM, init conv, final_conv.2)
//   ap_embed_bwd        backward of ap_embed: every fc_t, then swish(fc_t2(swish(fc_t1(.))))
//   ap_weight_norm_bwd  dW of a folded W = g v / ||v|| back to (dg, dv)
// No atomics anywhere: every sum has a fixed order, two runs give the same bits.
#include "ap_common.h"

namespace ap {

// ---------------------------------------------------------------------------------------------
// ap_wgrad_corr.  Both operands are contiguous along time, the contraction index, so a chunk of WG_KC samples of 128 P rows and of
// 64 Q rows per tap is staged in LDS as [row][time] with 16-byte global loads and the MFMA fragments (lane (j, hh): row j, k = hh)
// are read with an ODD row stride: the 32 lanes of a ds_read_b32 group hit 32 different banks.  A workgroup stages its P tile once
// per chunk and accumulates every tap from that tap's own window of Q: window k starts at the 16-byte-aligned sample
// t0 + floor4((k - taps/2) dil) and is WG_KC + 4 samples wide, the fragment read adds the remainder 0..3.
// Wave (wm, wn) of the 2 x 2 owns rows [64 wm, 64 wm + 64) x columns [32 wn, 32 wn + 32): 2 x TAPS accumulator tiles.
// K = B L is cut into chunks that never straddle a clip; slice z of the grid takes a contiguous run of chunks and writes its raw
// partial sums to the workspace, slice_sum_kernel adds the slices in slice order.
// ---------------------------------------------------------------------------------------------
constexpr int WG_KC = 32;                 // samples per staged chunk
constexpr int WG_BM = 128, WG_BN = 64;    // tile of G per workgroup
constexpr int WG_PS = WG_KC + 1;          // floats per staged P row (odd)
constexpr int WG_QW = WG_KC + 4;          // samples per staged Q window
constexpr int WG_QS = WG_QW + 1;          // floats per staged Q row (odd)
constexpr int WG_NT = 256;
constexpr int WG_PV = WG_BM * (WG_KC / 4) / WG_NT;          // 16-byte loads of P per thread and chunk (4)

struct WgradArgs {
  const float *P, *Q, *film;
  float *part;
  int B, M, N, L, dil, slices, cpc, nchunk;   // cpc: chunks per clip
};

enum { WG_PLAIN = 0, WG_FILM = 1, WG_GATE = 2 };

template <int TAPS, bool VEC, int MODE>
__global__ __launch_bounds__(WG_NT) void wgrad_corr_kernel(WgradArgs a) {
  constexpr int NQV = TAPS * WG_BN * (WG_QW / 4);            // 16-byte loads of Q per chunk
  constexpr int QV = (NQV + WG_NT - 1) / WG_NT;              // ... per thread
  constexpr bool GATE = MODE == WG_GATE;
  __shared__ float Ps[WG_BM * WG_PS];
  __shared__ float Qs[TAPS * WG_BN * WG_QS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, hh = lane >> 5, wm = wave & 1, wn = wave >> 1;
  const int n0 = blockIdx.x * WG_BN, m0 = blockIdx.y * WG_BM, slice = blockIdx.z;
  const int L = a.L, M = a.M, N = a.N;
  const int QR = GATE ? 2 * N : N;                           // rows per clip of the Q tensor

  // per tap: offset, aligned window start, remainder, and whether any sample of a clip can meet it
  int al[TAPS], sh[TAPS];
  bool on[TAPS];
#pragma unroll
  for (int k = 0; k < TAPS; k++) {
    const int off = (k - TAPS / 2) * a.dil;
    al[k] = off & ~3;
    sh[k] = off - al[k];
    on[k] = off > -L && off < L;
  }

  f32x4 pr[WG_PV], qr[QV], qr2[GATE ? QV : 1];

  auto load = [&](int c) {
    const int b = c / a.cpc, t0 = (c % a.cpc) * WG_KC;
#pragma unroll
    for (int i = 0; i < WG_PV; i++) {
      const int idx = tid + i * WG_NT, r = idx >> 3, q = idx & 7;
      const int m = m0 + r, t = t0 + 4 * q;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (m < M) {
        const float *p = a.P + ((size_t)b * M + m) * L;
        if (VEC) {
          if (t < L) v = *reinterpret_cast<const f32x4 *>(p + t);
        } else {
#pragma unroll
          for (int e = 0; e < 4; e++)
            if (t + e < L) v[e] = p[t + e];
        }
      }
      pr[i] = v;
    }
#pragma unroll
    for (int i = 0; i < QV; i++) {
      const int idx = tid + i * WG_NT;
      f32x4 v = {0.f, 0.f, 0.f, 0.f}, v2 = {0.f, 0.f, 0.f, 0.f};
      if (idx < NQV) {
        const int k = idx / (WG_BN * (WG_QW / 4)), rem = idx % (WG_BN * (WG_QW / 4));
        const int r = rem / (WG_QW / 4), q = rem % (WG_QW / 4);
        const int n = n0 + r, t = t0 + al[k] + 4 * q;
        if (n < N && on[k]) {
          const float *p = a.Q + ((size_t)b * QR + n) * L;
          if (VEC) {
            if (t >= 0 && t < L) {
              v = *reinterpret_cast<const f32x4 *>(p + t);
              if (GATE) v2 = *reinterpret_cast<const f32x4 *>(p + (size_t)N * L + t);
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
              if (t + e >= 0 && t + e < L) {
                v[e] = p[t + e];
                if (GATE) v2[e] = p[(size_t)N * L + t + e];
              }
          }
        }
      }
      qr[i] = v;
      if (GATE) qr2[i] = v2;
    }
  };

  auto store = [&](int c) {
    const int t0 = (c % a.cpc) * WG_KC;
#pragma unroll
    for (int i = 0; i < WG_PV; i++) {
      const int idx = tid + i * WG_NT, r = idx >> 3, q = idx & 7;
#pragma unroll
      for (int e = 0; e < 4; e++) Ps[r * WG_PS + 4 * q + e] = pr[i][e];
    }
#pragma unroll
    for (int i = 0; i < QV; i++) {
      const int idx = tid + i * WG_NT;
      if (idx < NQV) {
        const int k = idx / (WG_BN * (WG_QW / 4)), rem = idx % (WG_BN * (WG_QW / 4));
        const int r = rem / (WG_QW / 4), q = rem % (WG_QW / 4);
        const int n = n0 + r, t = t0 + al[k] + 4 * q;
        const bool row = n < N && on[k];
        const float f = (MODE == WG_FILM && row) ? a.film[n] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const bool in = row && t + e >= 0 && t + e < L;       // the conv's zero padding applies to Q~: padded samples stay 0
          float v = qr[i][e];
          if (MODE == WG_FILM) v += f;
          if (GATE) v = gate(v, qr2[i][e]);
          Qs[(k * WG_BN + r) * WG_QS + 4 * q + e] = in ? v : 0.f;
        }
      }
    }
  };

  f32x16 acc[2][TAPS];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int k = 0; k < TAPS; k++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][k][r] = 0.f;

  const int c0 = (int)((long long)slice * a.nchunk / a.slices), c1 = (int)((long long)(slice + 1) * a.nchunk / a.slices);
  if (c0 < c1) {
    load(c0);
    store(c0);
  }
  __syncthreads();
  for (int c = c0; c < c1; c++) {
    if (c + 1 < c1) load(c + 1);
    const float *pa = Ps + (wm * 64 + j) * WG_PS + hh;
#pragma unroll
    for (int k = 0; k < TAPS; k++) {
      if (!on[k]) continue;                                     // (uniform) a tap no sample meets: its slab of G stays exactly 0
      const float *qb = Qs + (k * WG_BN + wn * 32 + j) * WG_QS + sh[k] + hh;
#pragma unroll
      for (int s = 0; s < WG_KC / 2; s++) {
        const float bv = qb[2 * s];
        acc[0][k] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * s], bv, acc[0][k], 0, 0, 0);
        acc[1][k] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[32 * WG_PS + 2 * s], bv, acc[1][k], 0, 0, 0);
      }
    }
    __syncthreads();
    if (c + 1 < c1) store(c + 1);
    __syncthreads();
  }

  // lane (j, hh) holds column n0 + 32 wn + j, rows m0 + 64 wm + 32 i + rowoff(r, hh)
  const int n = n0 + wn * 32 + j;
  if (n < N) {
    float *out = a.part + (size_t)slice * M * N * TAPS;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int m = m0 + wm * 64 + i * 32 + rowoff(r, hh);
        if (m < M) {
#pragma unroll
          for (int k = 0; k < TAPS; k++) out[((size_t)m * N + n) * TAPS + k] = acc[i][k][r];
        }
      }
  }
}

static int wgrad_slices(int B, int M, int N, int L) {
  const long long tiles = (long long)((M + WG_BM - 1) / WG_BM) * ((N + WG_BN - 1) / WG_BN);
  const long long nchunk = (long long)B * ((L + WG_KC - 1) / WG_KC);
  // two workgroups for each of the 256 CUs (one stages while the other multiplies).  A constant, not the device's CU count: the
  // slicing sets the summation order, and a gradient's bits must not depend on the card or its partition mode
  const long long want = (512 + tiles - 1) / tiles;
  return (int)(want < 1 ? 1 : want > nchunk ? nchunk : want);
}

// ---------------------------------------------------------------------------------------------
// ap_rowsum: one workgroup per row m; thread i takes elements i, i + 256, ... of the row's (clip, time) run, then a tree over the
// 256 partial sums: one fixed order.  The sums are fp64 (the products fp32), rounded once on the way out.
// ---------------------------------------------------------------------------------------------
template <typename OUT>
__global__ __launch_bounds__(256) void rowsum_kernel(const float *__restrict__ A, const float *__restrict__ W, const float *__restrict__ R,
                                                     OUT *__restrict__ out, int B, int M, int L, int w_bcast, float scale, int accumulate) {
  __shared__ double red[256];
  const int m = blockIdx.x;
  double s = 0.0;                                               // fp64 sums: these rows cancel heavily, and what is summed per clip must
  for (int b = 0; b < B; b++) {                                 // add up to what is summed per batch
    const size_t row = ((size_t)b * M + m) * L, wrow = w_bcast ? (size_t)b * L : row;
    for (int t = threadIdx.x; t < L; t += 256) {
      float v = A[row + t];
      if (W) v *= W[wrow + t];
      if (R) v = R[row + t] > 0.f ? v : 0.f;
      s += (double)v;
    }
  }
  s = block_tree<256>(s, red, SumOp{});
  if (threadIdx.x == 0) {
    const OUT v = (OUT)((double)scale * s);
    out[m] = accumulate ? out[m] + v : v;
  }
}

// ---------------------------------------------------------------------------------------------
// ap_weight_norm_bwd: W[o] = g[o] v[o] / ||v[o]||   (WaveNet.py:23-34, nn.utils.weight_norm dim = 0); one workgroup per row o.
//   dg = (dW . v) / ||v||;   dv = (g / ||v||) (dW - v (dW . v) / ||v||^2).
// A row of one element (the init conv) has dv = 0 analytically (W depends on sign(v) only): written as exact 0, never 0/0-ish.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void weight_norm_bwd_kernel(const float *__restrict__ dW, const float *__restrict__ v,
                                                              const float *__restrict__ g, float *__restrict__ dg,
                                                              float *__restrict__ dv, int cols) {
  __shared__ double red[512];
  const size_t row = (size_t)blockIdx.x * cols;
  double nn = 0.0, dot = 0.0;
  for (int i = threadIdx.x; i < cols; i += 256) {
    const double x = v[row + i];
    nn += x * x;
    dot += (double)dW[row + i] * x;
  }
  block_tree2<256>(nn, dot, red, SumOp{});
  const double inv = nn > 0.0 ? 1.0 / sqrt(nn) : 0.0;           // (an all-zero v row has no direction: gradients 0, not NaN)
  if (threadIdx.x == 0) dg[blockIdx.x] = (float)(dot * inv);
  const double gs = (double)g[blockIdx.x] * inv, proj = dot * inv * inv;
  for (int i = threadIdx.x; i < cols; i += 256)
    dv[row + i] = cols == 1 ? 0.f : (float)(gs * ((double)dW[row + i] - (double)v[row + i] * proj));
}

// ---------------------------------------------------------------------------------------------
// ap_embed_bwd (util.py:68-93; WaveNet.py:82-83, 124-126).  Tiny matrices, plain kernels.
// ---------------------------------------------------------------------------------------------
// Everything between dpart and the four weight gradients is a chain of heavily cancelling sums (832 rows into demb, 512 into da1),
// so it runs in fp64 from an fp64 dpart: what two sub-batches add up to is then what one batch gives, to fp32 rounding of the result.
__device__ __forceinline__ double sigmoid_d(double x) { return 1.0 / (1.0 + exp(-x)); }
__device__ __forceinline__ double swish_d(double x) { return x * sigmoid_d(x); }
__device__ __forceinline__ double swish_grad_d(double x) {
  const double s = sigmoid_d(x);
  return s * (1.0 + x * (1.0 - s));
}

// out[r][c] (+)= a[r] * (b ? b[c] : 1)
template <typename TA>
__global__ void outer_acc_kernel(const TA *__restrict__ av, const float *__restrict__ bv, float *__restrict__ out, int cols, size_t total,
                                 int accumulate) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const float v = (float)(av[idx / cols] * (bv ? (TA)bv[idx % cols] : (TA)1));
  out[idx] = accumulate ? out[idx] + v : v;
}

// demb[e] = sum_rows fct_w[row][e] dpart[row]: 64 columns per workgroup, wave w takes rows w, w + 4, ..., the four sums added in wave order
__global__ __launch_bounds__(256) void embed_demb_kernel(const float *__restrict__ w, const double *__restrict__ dpart, double *__restrict__ demb,
                                                         int rows, int E) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane, ec = min(e, E - 1);
  double s = 0.0;
#pragma unroll 4
  for (int r = wave; r < rows; r += 4) s += (double)w[(size_t)r * E + ec] * dpart[r];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && e < E) demb[e] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// One workgroup: recompute e0, z1, z2 of the forward MLP, then dz2 = demb swish'(z2), da1 = W2^T dz2, dz1 = da1 swish'(z1).
// scratch (behind demb): e0 [Ein], a1 [Emid], dz1 [Emid], dz2 [Eout] as fp32 (the outer products are taken from it by outer_acc_kernel).
__global__ __launch_bounds__(512) void embed_mlp_bwd_kernel(const float *__restrict__ freq, const float *__restrict__ w1,
                                                            const float *__restrict__ b1, const float *__restrict__ w2,
                                                            const float *__restrict__ b2, const double *__restrict__ demb, float step, int Ein,
                                                            int Emid, int Eout, float *__restrict__ scratch) {
  extern __shared__ double smd[];
  double *e0 = smd, *z1 = e0 + Ein, *a1 = z1 + Emid, *dz2 = a1 + Emid;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int half = Ein / 2;
  for (int i = threadIdx.x; i < half; i += blockDim.x) {
    const float x = step * freq[i];                             // fp32, as ap_embed forms the embedding
    e0[i] = sinf(x);
    e0[half + i] = cosf(x);
  }
  __syncthreads();
  for (int o = wave; o < Emid; o += nw) {                       // wave per row
    double s = 0.0;
    for (int i = lane; i < Ein; i += 64) s += (double)w1[(size_t)o * Ein + i] * e0[i];
    s = wave_sum(s);
    if (lane == 0) {
      z1[o] = s + (double)b1[o];
      a1[o] = swish_d(s + (double)b1[o]);
    }
  }
  __syncthreads();
  for (int o = wave; o < Eout; o += nw) {
    double s = 0.0;
    for (int i = lane; i < Emid; i += 64) s += (double)w2[(size_t)o * Emid + i] * a1[i];
    s = wave_sum(s);
    if (lane == 0) dz2[o] = demb[o] * swish_grad_d(s + (double)b2[o]);
  }
  __syncthreads();
  float *s_e0 = scratch, *s_a1 = s_e0 + Ein, *s_dz1 = s_a1 + Emid, *s_dz2 = s_dz1 + Emid;
  for (int i = threadIdx.x; i < Emid; i += blockDim.x) {         // da1[i] = sum_o W2[o][i] dz2[o], coalesced over i
    double s = 0.0;
    for (int o = 0; o < Eout; o++) s += (double)w2[(size_t)o * Emid + i] * dz2[o];
    s_dz1[i] = (float)(s * swish_grad_d(z1[i]));
    s_a1[i] = (float)a1[i];
  }
  for (int i = threadIdx.x; i < Ein; i += blockDim.x) s_e0[i] = (float)e0[i];
  for (int i = threadIdx.x; i < Eout; i += blockDim.x) s_dz2[i] = (float)dz2[i];
}

}  // namespace ap

using namespace ap;

extern "C" size_t ap_wgrad_workspace_bytes(int B, int M, int N, int L, int taps) {
  if (B < 1 || M < 1 || N < 1 || L < 1 || (taps != 1 && taps != 3)) return 0;
  return (size_t)wgrad_slices(B, M, N, L) * M * N * taps * sizeof(float);
}

template <int TAPS, bool VEC>
static void wgrad_launch_mode(const WgradArgs &a, int mode, dim3 grid, hipStream_t st) {
  if (mode == WG_PLAIN) wgrad_corr_kernel<TAPS, VEC, WG_PLAIN><<<grid, WG_NT, 0, st>>>(a);
  else if (mode == WG_FILM) wgrad_corr_kernel<TAPS, VEC, WG_FILM><<<grid, WG_NT, 0, st>>>(a);
  else wgrad_corr_kernel<TAPS, VEC, WG_GATE><<<grid, WG_NT, 0, st>>>(a);
}

extern "C" int ap_wgrad_corr(const float *P, const float *Q, const float *film, float *G, void *workspace, size_t ws_bytes, int B,
                             int M, int N, int L, int taps, int dil, int mode, float p_scale, int accumulate, void *stream) {
  if (!P || !Q || !G || !workspace || B < 1 || L < 1 || M < 32 || N < 32 || M % 32 || N % 32 || (taps != 1 && taps != 3) || dil < 1 ||
      mode < WG_PLAIN || mode > WG_GATE || (mode == WG_FILM && !film)) {
    set_error("ap_wgrad_corr: bad argument (M=%d N=%d multiples of 32, taps=%d in {1,3}, dil=%d >= 1, mode=%d, B=%d L=%d)", M, N, taps, dil,
              mode, B, L);
    return -22;
  }
  if ((long long)dil * 2 + L + 64 > 0x7fffffffLL) { set_error("ap_wgrad_corr: dil=%d out of range", dil); return -22; }
  const size_t need = ap_wgrad_workspace_bytes(B, M, N, L, taps);
  if (ws_bytes < need) { set_error("ap_wgrad_corr: workspace of %zu bytes, need %zu (ap_wgrad_workspace_bytes)", ws_bytes, need); return -22; }
  WgradArgs a;
  a.P = P, a.Q = Q, a.film = film, a.part = (float *)workspace;
  a.B = B, a.M = M, a.N = N, a.L = L, a.dil = taps == 1 ? 1 : dil;
  a.slices = wgrad_slices(B, M, N, L);
  a.cpc = (L + WG_KC - 1) / WG_KC;
  a.nchunk = B * a.cpc;
  const dim3 grid((N + WG_BN - 1) / WG_BN, (M + WG_BM - 1) / WG_BM, a.slices);
  const hipStream_t st = (hipStream_t)stream;
  // 16-byte loads need every row to start on a 16-byte boundary
  const bool vec = L % 4 == 0 && ((uintptr_t)P & 15) == 0 && ((uintptr_t)Q & 15) == 0;
  if (taps == 3) {
    if (vec) wgrad_launch_mode<3, true>(a, mode, grid, st);
    else wgrad_launch_mode<3, false>(a, mode, grid, st);
  } else {
    if (vec) wgrad_launch_mode<1, true>(a, mode, grid, st);
    else wgrad_launch_mode<1, false>(a, mode, grid, st);
  }
  const size_t total = (size_t)M * N * taps;
  slice_sum_kernel<float><<<(unsigned)((total + 255) / 256), 256, 0, st>>>(a.part, G, total, a.slices, 1, p_scale, accumulate);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_rowsum(const float *A, const float *W, const float *R, float *out, int B, int M, int L, int w_broadcast, float scale,
                         int accumulate, void *stream) {
  if (!A || !out || B < 1 || M < 1 || L < 1) { set_error("ap_rowsum: bad argument"); return -22; }
  rowsum_kernel<float><<<M, 256, 0, (hipStream_t)stream>>>(A, W, R, out, B, M, L, W && w_broadcast ? 1 : 0, scale, accumulate);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_rowsum_f64(const float *A, double *out, int B, int M, int L, int accumulate, void *stream) {
  if (!A || !out || B < 1 || M < 1 || L < 1) { set_error("ap_rowsum_f64: bad argument"); return -22; }
  rowsum_kernel<double><<<M, 256, 0, (hipStream_t)stream>>>(A, nullptr, nullptr, out, B, M, L, 0, 1.0f, accumulate);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_weight_norm_bwd(const float *dW, const float *v, const float *g, float *dg, float *dv, int rows, int cols, void *stream) {
  if (!dW || !v || !g || !dg || !dv || rows < 1 || cols < 1) { set_error("ap_weight_norm_bwd: bad argument"); return -22; }
  weight_norm_bwd_kernel<<<rows, 256, 0, (hipStream_t)stream>>>(dW, v, g, dg, dv, cols);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" size_t ap_embed_bwd_scratch_elems(const ap_ctx *ctx) {
  if (!ctx) return 0;
  const ap_config &c = ctx->cfg;
  return 2 * (size_t)c.embed_dim_out + (size_t)c.embed_dim_in + 2 * (size_t)c.embed_dim_mid + (size_t)c.embed_dim_out;   // demb as fp64, then fp32
}

extern "C" int ap_embed_bwd(ap_ctx *ctx, float step, const double *dpart, const float *emb, float *d_fct_w, float *d_fct_b, float *d_fc1_w,
                            float *d_fc1_b, float *d_fc2_w, float *d_fc2_b, float *scratch, int accumulate, void *stream) {
  if (!ctx || !ctx->loaded || !dpart || !emb || !d_fct_w || !d_fct_b || !d_fc1_w || !d_fc1_b || !d_fc2_w || !d_fc2_b || !scratch) {
    set_error("ap_embed_bwd: not loaded / null");
    return -22;
  }
  const ap_config &c = ctx->cfg;
  const int Ein = c.embed_dim_in, Emid = c.embed_dim_mid, Eout = c.embed_dim_out, rows = ctx->NL * ctx->C;
  const hipStream_t st = (hipStream_t)stream;
  // every refusal comes before the first launch: the results accumulate into the caller's buffers
  if ((uintptr_t)scratch & 7) { set_error("ap_embed_bwd: scratch must be 8-byte aligned"); return -22; }
  const size_t sm = (size_t)(Ein + 2 * Emid + Eout) * sizeof(double);
  if (sm > 64 * 1024) { set_error("ap_embed_bwd: embedding dims %d / %d / %d exceed the MLP kernel's LDS image", Ein, Emid, Eout); return -22; }
  double *demb = (double *)scratch;
  float *fs = scratch + 2 * (size_t)Eout;
  float *s_e0 = fs, *s_a1 = s_e0 + Ein, *s_dz1 = s_a1 + Emid, *s_dz2 = s_dz1 + Emid;
  auto outer = [&](auto *av, const float *bv, float *out, int r, int cl) {
    const size_t total = (size_t)r * cl;
    outer_acc_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(av, bv, out, cl, total, accumulate);
  };
  outer(dpart, emb, d_fct_w, rows, Eout);                       // d fc_t_n.weight = dpart_n (x) emb    (WaveNet.py:82)
  outer(dpart, (const float *)nullptr, d_fct_b, rows, 1);
  embed_demb_kernel<<<(Eout + 63) / 64, 256, 0, st>>>(ctx->fct_w, dpart, demb, rows, Eout);
  embed_mlp_bwd_kernel<<<1, 512, sm, st>>>(ctx->emb_freq, ctx->fc1_w, ctx->fc1_b, ctx->fc2_w, ctx->fc2_b, demb, step, Ein, Emid, Eout, fs);
  outer(s_dz2, s_a1, d_fc2_w, Eout, Emid);                      // WaveNet.py:126
  outer(s_dz2, (const float *)nullptr, d_fc2_b, Eout, 1);
  outer(s_dz1, s_e0, d_fc1_w, Emid, Ein);                       // WaveNet.py:125
  outer(s_dz1, (const float *)nullptr, d_fc1_b, Emid, 1);
  AP_HIP(hipGetLastError());
  return 0;
}
