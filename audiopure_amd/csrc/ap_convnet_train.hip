// Train-mode step of the 2-D ConvNet classifiers (audio_models/ConvNets_SpeechCommands/train_speech_commands.py:122-153: model.train(),
// criterion(model(x), y), loss.backward(); models/{resnet,wideresnet,resnext,dpn,densenet}.py).  The eval plan folds BatchNorm into the
// convolutions; in train mode the statistics are the batch's, so the plan keeps BatchNorm as a step of its own and the step needs
//   ap_conv2d_wgrad      dW[co][n][i][j] (+)= sum_{b,oh,ow} dy[b][co][oh][ow] x[b][g Cin/g + n][oh s + i - pad][ow s + j - pad]
//   ap_conv2d_pack_bwd   the live weight -> the A-operand image ap_conv2d_fwd reads for the input gradient (taps flipped, in / out swapped)
//   ap_bn2d_train_fwd    batch statistics, y = gamma xhat + beta [ReLU], running statistics
//   ap_bn2d_train_bwd    d beta, d gamma, dx
// Conv forward and conv dx stay ap_conv2d_fwd, the biases ap_rowsum, everything element-wise the primitives of ap_convnet.hip.
// No floating-point atomics: every sum has a fixed order and a slice count that does not depend on the card; two runs give equal bits.
#include "ap_common.h"

namespace ap {
namespace {

// ---------------------------------------------------------------------------------------------
// ap_conv2d_wgrad: per group an implicit GEMM on v_mfma_f32_32x32x2_f32 with rows = Cout/g (the channels of dy), columns =
// (Cin/g) k k in the order of dW's own memory (column = n k k + i k + j) and the contraction index kk = b OH OW + oh OW + ow running
// over the whole batch: a chunk of CW_KC positions may start in one image and end in the next (H = W = 1, nn.Linear, contracts over
// B alone).  The structure and the LDS fragment layout are wgrad_corr_kernel's (ap_wgrad.hip): both operands staged as
// [row][position] with an ODD row stride, so the 32 lanes of a fragment read hit 32 banks; the next chunk is fetched into
// registers while this one multiplies; slice z takes a contiguous run of chunks and writes raw partial sums, slice_sum_kernel
// adds the slices in slice order.  Wave (wm, wn) of the 2 x 2 owns rows [64 wm, +64) x columns [32 wn, +32) of the 128 x 64 tile.
// A tile lies inside ONE group: rows past Cout/g and columns past (Cin/g) k k are zeros in LDS and are not stored.
// dy is staged with 16-byte loads where OH OW % 4 == 0 and the pointer allows (a quad then never leaves its image); x likewise for
// the pointwise case k = 1, stride 1 (pad 0), where its image IS [channel][position]; otherwise x is gathered element by element
// (the halo, the stride-2 phase and the zero padding decided per element) with the position fastest across lanes.
// ---------------------------------------------------------------------------------------------
constexpr int CW_KC = 32;                 // contraction positions per staged chunk
constexpr int CW_BM = 128, CW_BN = 64;    // tile of dW per workgroup
constexpr int CW_LS = CW_KC + 1;          // floats per staged row (odd)
constexpr int CW_NT = 256;
constexpr int CW_PI = CW_BM * CW_KC / CW_NT;   // scalar loads of dy per thread and chunk (16)
constexpr int CW_QI = CW_BN * CW_KC / CW_NT;   // scalar loads of x per thread and chunk (8)
constexpr int CW_TILES_WANTED = 512;      // workgroups asked for; a constant: the slicing sets the summation order

struct ConvWgradArgs {
  const float *dy, *x;
  float *part;
  int B, Cin, H, W, Cout, k, stride, pad, groups, OH, OW, x_cstride, x_coff;
  int Mg, Cg, Ng, mtiles, slices, nchunk, Ktot;
};

template <bool VECP, bool VECQ>
__global__ __launch_bounds__(CW_NT) void conv2d_wgrad_kernel(ConvWgradArgs a) {
  __shared__ float Ps[CW_BM * CW_LS];
  __shared__ float Qs[CW_BN * CW_LS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, hh = lane >> 5, wm = wave & 1, wn = wave >> 1;
  const int g = blockIdx.y / a.mtiles, m0 = (blockIdx.y % a.mtiles) * CW_BM, n0 = blockIdx.x * CW_BN, slice = blockIdx.z;
  const int OHW = a.OH * a.OW, HW = a.H * a.W, KK = a.k * a.k;
  const int Mg = a.Mg, Ng = a.Ng;
  const float *dyg = a.dy + (size_t)g * Mg * OHW;                                   // + (b Cout + m) OHW + p
  const float *xg = a.x + ((size_t)a.x_coff + (size_t)g * a.Cg) * HW;               // + (b x_cstride + n) HW + ih W + iw

  // the gathered path: a thread keeps one position of the chunk (tid & 31) and walks rows / columns (tid >> 5) + 8 i
  const int kl = tid & 31, r8 = tid >> 5;
  int qoff[VECQ ? 1 : CW_QI], qdi[VECQ ? 1 : CW_QI], qdj[VECQ ? 1 : CW_QI];         // per column: channel offset (-1: none), tap offsets
  if constexpr (!VECQ) {
#pragma unroll
    for (int i = 0; i < CW_QI; i++) {
      const int col = n0 + r8 + 8 * i;
      if (col < Ng) {
        const int n = col / KK, t = col - n * KK, ti = t / a.k;
        qoff[i] = n * HW;
        qdi[i] = ti - a.pad;
        qdj[i] = t - ti * a.k - a.pad;
      } else {
        qoff[i] = -1;
        qdi[i] = qdj[i] = 0;
      }
    }
  }

  float pr[CW_PI], qr[CW_QI];

  auto load = [&](int c) {
    const int kk0 = c * CW_KC;
    // the gathered path's position
    const int kk = kk0 + kl;
    const bool kin = kk < a.Ktot;
    const int b = kin ? kk / OHW : 0, p = kin ? kk - b * OHW : 0;
    if constexpr (VECP) {
#pragma unroll
      for (int i = 0; i < CW_PI / 4; i++) {
        const int idx = tid + i * CW_NT, r = idx >> 3, q = idx & 7;
        const int m = m0 + r, kq = kk0 + 4 * q;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (m < Mg && kq < a.Ktot) {                              // Ktot % 4 == 0 here: a quad is inside or outside as a whole
          const int bq = kq / OHW, pq = kq - bq * OHW;
          v = *reinterpret_cast<const f32x4 *>(dyg + ((size_t)bq * a.Cout + m) * OHW + pq);
        }
#pragma unroll
        for (int e = 0; e < 4; e++) pr[4 * i + e] = v[e];
      }
    } else {
#pragma unroll
      for (int i = 0; i < CW_PI; i++) {
        const int m = m0 + r8 + 8 * i;
        pr[i] = (kin && m < Mg) ? dyg[((size_t)b * a.Cout + m) * OHW + p] : 0.f;
      }
    }
    if constexpr (VECQ) {                                                   // k = 1, stride 1, pad 0: column = channel, OHW == HW
#pragma unroll
      for (int i = 0; i < CW_QI / 4; i++) {
        const int idx = tid + i * CW_NT, r = idx >> 3, q = idx & 7;
        const int n = n0 + r, kq = kk0 + 4 * q;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (n < Ng && kq < a.Ktot) {
          const int bq = kq / HW, pq = kq - bq * HW;
          v = *reinterpret_cast<const f32x4 *>(xg + ((size_t)bq * a.x_cstride + n) * HW + pq);
        }
#pragma unroll
        for (int e = 0; e < 4; e++) qr[4 * i + e] = v[e];
      }
    } else {
      const int oh = p / a.OW, ow = p - oh * a.OW;
      const int ih0 = oh * a.stride, iw0 = ow * a.stride;
      const float *xb = xg + (size_t)b * a.x_cstride * HW;
#pragma unroll
      for (int i = 0; i < CW_QI; i++) {
        const int ih = ih0 + qdi[i], iw = iw0 + qdj[i];
        const bool in = kin && qoff[i] >= 0 && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;   // terms outside the image are 0
        qr[i] = in ? xb[(size_t)qoff[i] + ih * a.W + iw] : 0.f;
      }
    }
  };

  auto store = [&]() {
    if constexpr (VECP) {
#pragma unroll
      for (int i = 0; i < CW_PI / 4; i++) {
        const int idx = tid + i * CW_NT, r = idx >> 3, q = idx & 7;
#pragma unroll
        for (int e = 0; e < 4; e++) Ps[r * CW_LS + 4 * q + e] = pr[4 * i + e];
      }
    } else {
#pragma unroll
      for (int i = 0; i < CW_PI; i++) Ps[(r8 + 8 * i) * CW_LS + kl] = pr[i];
    }
    if constexpr (VECQ) {
#pragma unroll
      for (int i = 0; i < CW_QI / 4; i++) {
        const int idx = tid + i * CW_NT, r = idx >> 3, q = idx & 7;
#pragma unroll
        for (int e = 0; e < 4; e++) Qs[r * CW_LS + 4 * q + e] = qr[4 * i + e];
      }
    } else {
#pragma unroll
      for (int i = 0; i < CW_QI; i++) Qs[(r8 + 8 * i) * CW_LS + kl] = qr[i];
    }
  };

  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[i][r] = 0.f;

  const int c0 = (int)((long long)slice * a.nchunk / a.slices), c1 = (int)((long long)(slice + 1) * a.nchunk / a.slices);
  if (c0 < c1) {
    load(c0);
    store();
  }
  __syncthreads();
  for (int c = c0; c < c1; c++) {
    if (c + 1 < c1) load(c + 1);
    const float *pa = Ps + (wm * 64 + j) * CW_LS + hh;
    const float *qb = Qs + (wn * 32 + j) * CW_LS + hh;
#pragma unroll
    for (int s = 0; s < CW_KC / 2; s++) {
      const float bv = qb[2 * s];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * s], bv, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[32 * CW_LS + 2 * s], bv, acc[1], 0, 0, 0);
    }
    __syncthreads();
    if (c + 1 < c1) store();
    __syncthreads();
  }

  // lane (j, hh) holds column n0 + 32 wn + j, rows m0 + 64 wm + 32 i + rowoff(r, hh)
  const int n = n0 + wn * 32 + j;
  if (n < Ng) {
    float *out = a.part + (size_t)slice * a.Cout * Ng + (size_t)g * Mg * Ng;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int m = m0 + wm * 64 + i * 32 + rowoff(r, hh);
        if (m < Mg) out[(size_t)m * Ng + n] = acc[i][r];
      }
  }
}

// 0, or -22 with the error text set: everything ap_conv2d_wgrad refuses, and the geometry it runs on
int conv_wgrad_plan(int B, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int groups, int x_cstride, int x_coff,
                    ConvWgradArgs *a) {
  if (B < 1 || Cin < 1 || H < 1 || W < 1 || Cout < 1 || groups < 1) {
    set_error("ap_conv2d_wgrad: bad shape (B=%d Cin=%d H=%d W=%d Cout=%d groups=%d)", B, Cin, H, W, Cout, groups);
    return -22;
  }
  if (kh != kw || (kh != 1 && kh != 3 && kh != 7)) { set_error("ap_conv2d_wgrad: kernel %d x %d (square 1, 3 or 7 only)", kh, kw); return -22; }
  if (stride != 1 && stride != 2) { set_error("ap_conv2d_wgrad: stride %d (1 or 2 only)", stride); return -22; }
  if (pad < 0 || pad > kh - 1) { set_error("ap_conv2d_wgrad: pad %d outside [0, k - 1 = %d]", pad, kh - 1); return -22; }
  if (Cin % groups || Cout % groups) { set_error("ap_conv2d_wgrad: groups %d must divide Cin %d and Cout %d", groups, Cin, Cout); return -22; }
  if (x_coff < 0 || x_cstride < 1 || (long long)x_coff + Cin > x_cstride) {
    set_error("ap_conv2d_wgrad: channels [%d, %d) outside a tensor of %d channels", x_coff, x_coff + Cin, x_cstride);
    return -22;
  }
  if (H + 2 * pad < kh || W + 2 * pad < kh) { set_error("ap_conv2d_wgrad: image %d x %d smaller than the kernel", H, W); return -22; }
  const int OH = (H + 2 * pad - kh) / stride + 1, OW = (W + 2 * pad - kh) / stride + 1;
  const long long Ktot = (long long)B * OH * OW, Ng = (long long)(Cin / groups) * kh * kh;
  if (Ktot + CW_KC > 0x7fffffffLL || Ng > 0x7fffffffLL || (long long)H * W * (Cin / groups) > 0x7fffffffLL) {
    set_error("ap_conv2d_wgrad: B OH OW = %lld or (Cin/g) k k = %lld out of range", Ktot, Ng);
    return -22;
  }
  a->B = B, a->Cin = Cin, a->H = H, a->W = W, a->Cout = Cout, a->k = kh, a->stride = stride, a->pad = pad, a->groups = groups;
  a->OH = OH, a->OW = OW, a->x_cstride = x_cstride, a->x_coff = x_coff;
  a->Mg = Cout / groups, a->Cg = Cin / groups, a->Ng = (int)Ng, a->Ktot = (int)Ktot;
  a->mtiles = (a->Mg + CW_BM - 1) / CW_BM;
  a->nchunk = (int)((Ktot + CW_KC - 1) / CW_KC);
  const long long tiles = (long long)groups * a->mtiles * ((a->Ng + CW_BN - 1) / CW_BN);
  if (tiles > 0x3fffffffLL) { set_error("ap_conv2d_wgrad: %lld tiles out of range", tiles); return -22; }
  const long long want = (CW_TILES_WANTED + tiles - 1) / tiles;
  a->slices = (int)(want < 1 ? 1 : want > a->nchunk ? a->nchunk : want);
  if ((long long)groups * a->mtiles > 65535 || a->slices > 65535) { set_error("ap_conv2d_wgrad: grid out of range"); return -22; }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// ap_conv2d_pack_bwd: wt[g Cin/g + n][m][i][j] = w[g Cout/g + m][n][k - 1 - i][k - 1 - j] -- the weight of the convolution from Cout
// back to Cin (same groups) whose forward is the conv's input gradient; ap_conv2d_pack then writes every image of it.
// ---------------------------------------------------------------------------------------------
__global__ void conv_flip_kernel(const float *__restrict__ w, float *__restrict__ wt, int Mg, int Cg, int KK, int groups) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)groups * Mg * Cg * KK) return;
  const int t = idx % KK;
  size_t rest = idx / KK;
  const int m = rest % Mg;
  rest /= Mg;
  const int n = rest % Cg, g = (int)(rest / Cg);
  wt[idx] = w[(((size_t)g * Mg + m) * Cg + n) * KK + (KK - 1 - t)];
}

// ---------------------------------------------------------------------------------------------
// BatchNorm2d with batch statistics (nn.BatchNorm2d in training mode): per channel the n = B HW values are cut into BN_SLICES
// contiguous runs, each summed in fp64 by one workgroup in a fixed order (block_wave_sum2), the slices added in slice order by the
// finalisers M5 shares (bn_stats_final_kernel, bn_bstats_final_kernel: ap_reduce.h).
// ---------------------------------------------------------------------------------------------
constexpr int BN_SLICES = 64;

struct BnArgs {
  const float *x, *y, *dy, *gamma, *beta, *stat_in;
  float *out, *stat, *rm, *rv, *dgamma, *dbeta;
  double *part, *mean2;
  int B, C, HW, x_cstride, x_coff, relu;
  long long n;
  float eps, momentum;
};

// part[slice][c] = (sum x, sum x^2).  grid (C, BN_SLICES).  Not m5t_stats_kernel: a slice here is a contiguous run of the n values, M5's
// is the clips slice, slice + 64, ... -- two orders, two sets of bits (the same holds for bn2d_bstats_kernel and m5t_bstats_kernel)
__global__ __launch_bounds__(256) void bn2d_stats_kernel(BnArgs a) {
  const int c = blockIdx.x, sl = blockIdx.y;
  const long long e0 = a.n * sl / BN_SLICES, e1 = a.n * (sl + 1) / BN_SLICES;
  double s1 = 0.0, s2 = 0.0;
  for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
    const long long b = e / a.HW;
    const int p = (int)(e - b * a.HW);
    const double v = (double)a.x[((size_t)b * a.x_cstride + a.x_coff + c) * a.HW + p];
    s1 += v;
    s2 += v * v;
  }
  block_wave_sum2(s1, s2);
  if (threadIdx.x == 0) {
    a.part[((size_t)sl * a.C + c) * 2] = s1;
    a.part[((size_t)sl * a.C + c) * 2 + 1] = s2;
  }
}

// y = gamma (x - mean) rstd + beta, optional ReLU: the affine first, so gamma of either sign (or 0) is served
__global__ __launch_bounds__(256) void bn2d_apply_kernel(BnArgs a, size_t total) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int p = (int)(idx % a.HW);
  const size_t rest = idx / a.HW;
  const int c = (int)(rest % a.C);
  const size_t b = rest / a.C;
  const float xh = (a.x[((size_t)b * a.x_cstride + a.x_coff + c) * a.HW + p] - a.stat[c]) * a.stat[a.C + c];
  float v = __builtin_fmaf(xh, a.gamma[c], a.beta[c]);
  if (a.relu) v = fmaxf(v, 0.f);
  a.out[idx] = v;
}

// part[slice][c] = (sum dy', sum dy' xhat), dy' = dy where the fused ReLU let y through.  grid (C, BN_SLICES)
__global__ __launch_bounds__(256) void bn2d_bstats_kernel(BnArgs a) {
  const int c = blockIdx.x, sl = blockIdx.y;
  const long long e0 = a.n * sl / BN_SLICES, e1 = a.n * (sl + 1) / BN_SLICES;
  const float mu = a.stat_in[c], rstd = a.stat_in[a.C + c];
  double s1 = 0.0, s2 = 0.0;
  for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
    const long long b = e / a.HW;
    const int p = (int)(e - b * a.HW);
    const size_t o = ((size_t)b * a.C + c) * a.HW + p;
    float g = a.dy[o];
    if (a.relu && !(a.y[o] > 0.f)) g = 0.f;
    const float xh = (a.x[((size_t)b * a.x_cstride + a.x_coff + c) * a.HW + p] - mu) * rstd;
    s1 += (double)g;
    s2 += (double)g * (double)xh;
  }
  block_wave_sum2(s1, s2);
  if (threadIdx.x == 0) {
    a.part[((size_t)sl * a.C + c) * 2] = s1;
    a.part[((size_t)sl * a.C + c) * 2 + 1] = s2;
  }
}

// dx = gamma rstd (dy' - mean(dy') - xhat mean(dy' xhat))
__global__ __launch_bounds__(256) void bn2d_dx_kernel(BnArgs a, size_t total) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int p = (int)(idx % a.HW);
  const size_t rest = idx / a.HW;
  const int c = (int)(rest % a.C);
  const size_t b = rest / a.C;
  const float rstd = a.stat_in[a.C + c];
  const float xh = (a.x[((size_t)b * a.x_cstride + a.x_coff + c) * a.HW + p] - a.stat_in[c]) * rstd;
  float g = a.dy[idx];
  if (a.relu && !(a.y[idx] > 0.f)) g = 0.f;
  const float m1 = (float)a.mean2[2 * c], m2 = (float)a.mean2[2 * c + 1];
  a.out[idx] = a.gamma[c] * rstd * (g - m1 - xh * m2);
}

int bn_check(const char *who, int B, int C, int HW, int x_cstride, int x_coff, size_t ws_bytes) {
  if (B < 1 || C < 1 || HW < 1 || x_coff < 0 || x_cstride < 1 || (long long)x_coff + C > x_cstride) {
    set_error("%s: bad shape (B=%d C=%d HW=%d, channels [%d, %d) of %d)", who, B, C, HW, x_coff, x_coff + C, x_cstride);
    return -22;
  }
  if ((long long)B * HW <= 1) {                                  // torch raises there too: the unbiased variance divides by n - 1
    set_error("%s: %lld values per channel, batch statistics need more than 1", who, (long long)B * HW);
    return -22;
  }
  if ((long long)B * C * HW > ((long long)1 << 40) || (((long long)B * C * HW + 255) / 256) > 0x7fffffffLL) {
    set_error("%s: tensor out of range", who);
    return -22;
  }
  const size_t need = ap_bn2d_train_workspace_bytes(C);
  if (ws_bytes < need) { set_error("%s: workspace of %zu bytes, need %zu (ap_bn2d_train_workspace_bytes)", who, ws_bytes, need); return -22; }
  return 0;
}

}  // namespace
}  // namespace ap

using namespace ap;

extern "C" size_t ap_conv2d_wgrad_workspace_bytes(int B, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int groups) {
  ConvWgradArgs a;
  if (conv_wgrad_plan(B, Cin, H, W, Cout, kh, kw, stride, pad, groups, Cin, 0, &a)) return 0;
  return (size_t)a.slices * Cout * a.Ng * sizeof(float);
}

extern "C" int ap_conv2d_wgrad(const float *dy, const float *x, float *dW, void *workspace, size_t ws_bytes, int B, int Cin, int H, int W,
                               int Cout, int kh, int kw, int stride, int pad, int groups, int x_cstride, int x_coff, int accumulate,
                               void *stream) {
  if (!dy || !x || !dW || !workspace) { set_error("ap_conv2d_wgrad: null pointer"); return -22; }
  ConvWgradArgs a;
  if (int rc = conv_wgrad_plan(B, Cin, H, W, Cout, kh, kw, stride, pad, groups, x_cstride, x_coff, &a)) return rc;
  const size_t total = (size_t)Cout * a.Ng, need = (size_t)a.slices * total * sizeof(float);
  if (ws_bytes < need) { set_error("ap_conv2d_wgrad: workspace of %zu bytes, need %zu (ap_conv2d_wgrad_workspace_bytes)", ws_bytes, need); return -22; }
  a.dy = dy, a.x = x, a.part = (float *)workspace;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((a.Ng + CW_BN - 1) / CW_BN, a.groups * a.mtiles, a.slices);
  // 16-byte loads: every row of the operand starts on a 16-byte boundary and a quad of positions stays inside one image
  const bool vecp = (a.OH * a.OW) % 4 == 0 && ((uintptr_t)dy & 15) == 0;
  const bool vecq = kh == 1 && stride == 1 && pad == 0 && (H * W) % 4 == 0 && ((uintptr_t)x & 15) == 0;
  if (vecp && vecq) conv2d_wgrad_kernel<true, true><<<grid, CW_NT, 0, st>>>(a);
  else if (vecp) conv2d_wgrad_kernel<true, false><<<grid, CW_NT, 0, st>>>(a);
  else if (vecq) conv2d_wgrad_kernel<false, true><<<grid, CW_NT, 0, st>>>(a);
  else conv2d_wgrad_kernel<false, false><<<grid, CW_NT, 0, st>>>(a);
  slice_sum_kernel<float><<<(unsigned)((total + 255) / 256), 256, 0, st>>>(a.part, dW, total, a.slices, 1, 1.0f, accumulate);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_conv2d_pack_bwd(const float *w, float *wT, float *scratch, int Cout, int Cin_g, int kh, int kw, int groups, void *stream) {
  if (!w || !wT || !scratch || Cout < 1 || Cin_g < 1 || groups < 1 || Cout % groups || kh < 1 || kh != kw) {
    set_error("ap_conv2d_pack_bwd: bad argument (Cout=%d Cin/g=%d k=%d x %d groups=%d)", Cout, Cin_g, kh, kw, groups);
    return -22;
  }
  const size_t n = (size_t)Cout * Cin_g * kh * kw;
  if ((n + 255) / 256 > 0x7fffffffULL) { set_error("ap_conv2d_pack_bwd: weight out of range"); return -22; }
  // everything ap_conv2d_pack refuses (null pointers, counts below 1, an output count its groups do not divide) is excluded above for
  // the swapped shape it is called with -- groups * Cin_g rows, Cout / groups >= 1 inputs per group -- so no refusal follows the launch
  conv_flip_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(w, scratch, Cout / groups, Cin_g, kh * kw, groups);
  AP_HIP(hipGetLastError());
  return ap_conv2d_pack(scratch, nullptr, wT, groups * Cin_g, Cout / groups, kh, kw, groups, stream);
}

extern "C" size_t ap_bn2d_train_workspace_bytes(int C) {
  if (C < 1) return 0;
  return ((size_t)BN_SLICES * C * 2 + (size_t)C * 2) * sizeof(double);
}

extern "C" int ap_bn2d_train_fwd(const float *x, const float *gamma, const float *beta, float *running_mean, float *running_var, float *y,
                                 float *stat, void *workspace, size_t ws_bytes, int B, int C, int HW, int x_cstride, int x_coff, float eps,
                                 float momentum, int relu, void *stream) {
  if (!x || !gamma || !beta || !running_mean || !running_var || !y || !stat || !workspace) { set_error("ap_bn2d_train_fwd: null pointer"); return -22; }
  if (int rc = bn_check("ap_bn2d_train_fwd", B, C, HW, x_cstride, x_coff, ws_bytes)) return rc;
  if ((uintptr_t)workspace & 7) { set_error("ap_bn2d_train_fwd: workspace not 8-byte aligned"); return -22; }
  if (!(momentum >= 0.f && momentum <= 1.f)) { set_error("ap_bn2d_train_fwd: momentum %g outside [0, 1]", (double)momentum); return -22; }
  if (!(eps >= 0.f)) { set_error("ap_bn2d_train_fwd: eps %g negative", (double)eps); return -22; }
  BnArgs a = {};
  a.x = x, a.gamma = gamma, a.beta = beta, a.out = y, a.stat = stat, a.rm = running_mean, a.rv = running_var;
  a.part = (double *)workspace;
  a.B = B, a.C = C, a.HW = HW, a.x_cstride = x_cstride, a.x_coff = x_coff, a.relu = relu ? 1 : 0;
  a.n = (long long)B * HW, a.eps = eps, a.momentum = momentum;
  const hipStream_t st = (hipStream_t)stream;
  const size_t total = (size_t)B * C * HW;
  bn2d_stats_kernel<<<dim3(C, BN_SLICES), 256, 0, st>>>(a);
  bn_stats_final_kernel<BN_SLICES><<<(C + 63) / 64, 64, 0, st>>>(a.part, a.rm, a.rv, stat, a.rm, a.rv, C, (double)a.n, eps, momentum);
  bn2d_apply_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(a, total);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_bn2d_train_bwd(const float *x, const float *y, const float *dy, const float *gamma, const float *stat, float *dx,
                                 float *dgamma, float *dbeta, void *workspace, size_t ws_bytes, int B, int C, int HW, int x_cstride,
                                 int x_coff, int relu, void *stream) {
  if (!x || !dy || !gamma || !stat || !workspace || (relu && !y)) { set_error("ap_bn2d_train_bwd: null pointer"); return -22; }
  if (int rc = bn_check("ap_bn2d_train_bwd", B, C, HW, x_cstride, x_coff, ws_bytes)) return rc;
  if ((uintptr_t)workspace & 7) { set_error("ap_bn2d_train_bwd: workspace not 8-byte aligned"); return -22; }
  BnArgs a = {};
  a.x = x, a.y = y, a.dy = dy, a.gamma = gamma, a.stat_in = stat, a.out = dx, a.dgamma = dgamma, a.dbeta = dbeta;
  a.part = (double *)workspace;
  a.mean2 = a.part + (size_t)BN_SLICES * C * 2;
  a.B = B, a.C = C, a.HW = HW, a.x_cstride = x_cstride, a.x_coff = x_coff, a.relu = relu ? 1 : 0;
  a.n = (long long)B * HW;
  const hipStream_t st = (hipStream_t)stream;
  const size_t total = (size_t)B * C * HW;
  bn2d_bstats_kernel<<<dim3(C, BN_SLICES), 256, 0, st>>>(a);
  bn_bstats_final_kernel<BN_SLICES><<<(C + 63) / 64, 64, 0, st>>>(a.part, a.mean2, dgamma, dbeta, C, (double)a.n);
  if (dx) bn2d_dx_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(a, total);
  AP_HIP(hipGetLastError());
  return 0;
}
