// M5 in train mode (audio_models/M5/M5Net.py:21-38 with nn.BatchNorm1d in training mode; audio_models/M5/train.py:86-103): forward with
// batch statistics, and the backward for every parameter and the waveform.
//
// The eval kernels (ap_frontend.hip) fold BatchNorm into the conv and keep a clip's four stages in one workgroup's LDS.  Batch statistics
// couple every clip of the batch at every stage -- a grid-wide reduction between conv and ReLU, four times forward and four times
// backward -- so this file is a sequence of small kernels over activations in the caller's workspace (HBM).  Nothing here has the
// 160 KB LDS ceiling of launch_m5 / launch_m5_bwd: L = 48 000 trains although launch_m5_bwd refuses it.
//
// The arithmetic is small (about 4 MMAC per clip forward; the largest contraction, dW_1, is 32 x 80 x (B 996) = 0.65 GMAC at B = 256), so
// the cut follows data movement and everything is plain fp32 FMA, no MFMA.
//
// Four places where a port of the eval kernels goes wrong, each marked (T1)..(T4) where the code meets it:
//  (T1) pre-pool positions at and beyond 4 Q_i: the floor pooling drops them, but they enter the mean and the variance, they receive a
//       non-zero dz through the two mean terms although their dy is 0, they contribute to dW_i and to the stage's input gradient.
//  (T2) negative gamma: the eval kernel takes the max before the per-channel affine, which is right only because the scale is folded
//       into the weights first.  Here the max and the argmax are taken on y, after the affine.
//  (T3) first maximum wins (nn.MaxPool1d's tie rule) and an element shut by the ReLU passes no gradient: one selection byte per pooled
//       element, 0..3 = the window position, 4 = shut -- the form of m5_stage_save.
//  (T4) tiny n (B = 1 at L = 6848 leaves stage 4 four values per channel): the running variance takes n / (n - 1), and the variance is
//       formed from fp64 sums so that sum z^2 - n mean^2 does not cancel away.
//
// Sums: no floating-point atomics.  Every sum over the batch is split into M5T_SLICES slices -- a constant, not the card's CU count --
// each summed in a fixed order, the slices added in fp64 in slice order and rounded once (as ap_rowsum does).  Two runs give equal bits.
#include "ap_common.h"

namespace ap {

constexpr int M5T_SLICES = 64;   // partial sums per reduced value
constexpr int M5T_CHUNK = 128;   // positions per (clip, chunk) work item of the split-K weight gradient

namespace {

struct M5TPlan {
  int ci[4], co[4], k[4], s[4], lin[4], P[4], Q[4];
  size_t wT[4], z[4], a[4], sel[4], stat[4], part, mean2, wpart, dz, da[2], feat, dlogit, total;   // byte offsets into the workspace
  size_t bw[4], bb[4], bg[4], bbe[4], brm[4], brv[4], bfw, bfb;                             // float offsets into the state blob
  size_t gw[4], gb[4], gg[4], gbe[4], gfw, gfb;                                             // float offsets into the gradient blob
  size_t rm[4], rv[4];                                                                      // float offsets into new_running
  size_t nw_max;
};

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

// 0, or -22 with the error text set -- before anything is launched
int m5t_plan(const ap_m5 *m, int B, int L, M5TPlan *pl) {
  const int nc = m->n_channel;
  const int ci[4] = {1, nc, nc, 2 * nc}, co[4] = {nc, nc, 2 * nc, 2 * nc}, k[4] = {m->k1, 3, 3, 3}, s[4] = {m->stride, 1, 1, 1};
  if (B < 1 || B > (1 << 20) || L < m->k1 || (size_t)B * (size_t)L > ((size_t)1 << 33)) {
    set_error("m5 train: B=%d L=%d (clip shorter than the first kernel %d, or batch out of range)", B, L, m->k1);
    return -22;
  }
  int lin = L;
  size_t sco = 0;
  for (int i = 0; i < 4; i++) {
    pl->ci[i] = ci[i]; pl->co[i] = co[i]; pl->k[i] = k[i]; pl->s[i] = s[i]; pl->lin[i] = lin;
    pl->P[i] = lin >= k[i] ? (lin - k[i]) / s[i] + 1 : 0;
    pl->Q[i] = pl->P[i] / 4;
    lin = pl->Q[i];
    sco += co[i];
  }
  if (pl->Q[0] < 3 || pl->Q[1] < 3 || pl->Q[2] < 3 || pl->Q[3] < 1) {
    set_error("m5 train: clip length %d too short for four conv/pool stages", L);
    return -22;
  }
  for (int i = 0; i < 4; i++)
    if ((size_t)B * pl->P[i] <= 1) {   // (T4) the unbiased running variance divides by n - 1
      set_error("m5 train: stage %d has %zu values per channel, batch statistics need more than 1", i + 1, (size_t)B * pl->P[i]);
      return -22;
    }
  size_t o = 0, g = 0, r = 0, nwm = 0;
  for (int i = 0; i < 4; i++) {
    const size_t nw = (size_t)co[i] * ci[i] * k[i];
    pl->bw[i] = o; pl->bb[i] = o + nw; pl->bg[i] = pl->bb[i] + co[i]; pl->bbe[i] = pl->bg[i] + co[i]; pl->brm[i] = pl->bbe[i] + co[i];
    pl->brv[i] = pl->brm[i] + co[i];
    o += nw + 5 * (size_t)co[i];
    pl->gw[i] = g; pl->gb[i] = g + nw; pl->gg[i] = pl->gb[i] + co[i]; pl->gbe[i] = pl->gg[i] + co[i];
    g += nw + 3 * (size_t)co[i];
    pl->rm[i] = r; pl->rv[i] = sco + r;
    r += co[i];
    if (nw > nwm) nwm = nw;
  }
  pl->bfw = o; pl->bfb = o + (size_t)m->n_output * 2 * nc;
  pl->gfw = g; pl->gfb = g + (size_t)m->n_output * 2 * nc;
  pl->nw_max = nwm;
  size_t off = 0, zmax = 0, amax = 0;
  for (int i = 0; i < 4; i++) {
    const size_t nz = (size_t)B * co[i] * pl->P[i], na = (size_t)B * co[i] * pl->Q[i];
    pl->wT[i] = off; off += up256((size_t)co[i] * ci[i] * k[i] * sizeof(float));
    pl->z[i] = off; off += up256(nz * sizeof(float));
    pl->a[i] = off; off += up256(na * sizeof(float));
    pl->sel[i] = off; off += up256(na);
    pl->stat[i] = off; off += up256((size_t)co[i] * 2 * sizeof(float));                 // [mean[co]; rstd[co]]
    if (nz > zmax) zmax = nz;
    if (na > amax) amax = na;
  }
  pl->part = off; off += up256((size_t)M5T_SLICES * 2 * nc * 2 * sizeof(double));
  pl->mean2 = off; off += up256((size_t)2 * nc * 2 * sizeof(double));                    // the backward's (mean dy, mean dy xhat) of one stage
  pl->wpart = off; off += up256((size_t)M5T_SLICES * nwm * sizeof(float));
  pl->dz = off; off += up256(zmax * sizeof(float));
  pl->da[0] = off; off += up256(amax * sizeof(float));
  pl->da[1] = off; off += up256(amax * sizeof(float));
  pl->feat = off; off += up256((size_t)B * 2 * nc * sizeof(float));
  pl->dlogit = off; off += up256((size_t)B * m->n_output * sizeof(float));
  pl->total = off;
  return 0;
}

inline unsigned grid_for(size_t total) {
  size_t b = (total + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > ((size_t)1 << 20) ? ((size_t)1 << 20) : b);
}

struct M5TPack {
  const float *w[4];
  float *wT[4];
  int co[4], cik[4];
};

// wT[r][o] = w[o][r], r = c k + t: threads with the output channel fastest read the conv's weights coalesced
__global__ __launch_bounds__(256) void m5t_pack_kernel(M5TPack a) {
  const int i = blockIdx.y, co = a.co[i], n = co * a.cik[i];
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += gridDim.x * 256) {
    const int o = idx / a.cik[i], r = idx % a.cik[i];
    a.wT[i][(size_t)r * co + o] = a.w[i][idx];
  }
}

// z[b][o][p] = bias[o] + sum_c sum_t w[o][c][t] in[b][c][p s + t] for EVERY valid position p < P (T1: also those the pooling drops).
// One thread: one output channel (fastest: a wave shares the input samples) and four neighbouring positions.
__global__ __launch_bounds__(256) void m5t_conv_kernel(const float *__restrict__ in, const float *__restrict__ wT,
                                                       const float *__restrict__ bias, float *__restrict__ z, int B, int ci, int co,
                                                       int k, int s, int Lin, int P) {
  const int G = (P + 3) / 4;
  const size_t total = (size_t)B * G * co;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int o = (int)(idx % co);
    const size_t r = idx / co;
    const int g = (int)(r % G), b = (int)(r / G);
    int off[4];
#pragma unroll
    for (int i = 0; i < 4; i++) off[i] = (4 * g + i < P ? 4 * g + i : P - 1) * s;   // a position past the end re-reads the last one, and is not stored
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float *inb = in + (size_t)b * ci * Lin;
    for (int c = 0; c < ci; c++) {
      const float *row = inb + (size_t)c * Lin;
      const float *wr = wT + (size_t)c * k * co + o;
      for (int t = 0; t < k; t++) {
        const float w = wr[(size_t)t * co];
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i] = __builtin_fmaf(w, row[off[i] + t], acc[i]);
      }
    }
    float *zr = z + ((size_t)b * co + o) * P + 4 * g;
    const float bo = bias[o];
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (4 * g + i < P) zr[i] = acc[i] + bo;
  }
}

// part[slice][o] = (sum z, sum z^2) over the clips b = slice, slice + 64, ... and all P positions (T1), in fp64.  grid (co, slices)
// Not bn2d_stats_kernel (ap_convnet_train.hip): its slice is a contiguous run of the n values, this one's is every 64th clip -- two
// orders, two sets of bits (the same holds for m5t_bstats_kernel and bn2d_bstats_kernel).  The finalisers are shared (ap_reduce.h).
__global__ __launch_bounds__(256) void m5t_stats_kernel(const float *__restrict__ z, double *__restrict__ part, int B, int co, int P) {
  const int o = blockIdx.x, sl = blockIdx.y;
  double s1 = 0.0, s2 = 0.0;
  for (int b = sl; b < B; b += M5T_SLICES) {
    const float *row = z + ((size_t)b * co + o) * P;
    for (int p = threadIdx.x; p < P; p += 256) {
      const double v = (double)row[p];
      s1 += v;
      s2 += v * v;
    }
  }
  block_wave_sum2(s1, s2);
  if (threadIdx.x == 0) {
    part[((size_t)sl * co + o) * 2] = s1;
    part[((size_t)sl * co + o) * 2 + 1] = s2;
  }
}

// (bn_stats_final_kernel then forms stat = [mean[co]; rstd[co]] and the new running statistics as torch does: the variance UNBIASED, T4)

// y = gamma (z - mean) rstd + beta; a = maxpool4(relu(y)) over the first 4 Q positions; sel = which of the four won, 4 = shut by the ReLU
__global__ __launch_bounds__(256) void m5t_apply_kernel(const float *__restrict__ z, const float *__restrict__ stat,
                                                        const float *__restrict__ gamma, const float *__restrict__ beta,
                                                        float *__restrict__ a, unsigned char *__restrict__ sel, int B, int co, int P,
                                                        int Q) {
  const size_t total = (size_t)B * co * Q;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int q = (int)(idx % Q);
    const size_t r = idx / Q;
    const int o = (int)(r % co);
    const float mu = stat[o], rstd = stat[co + o], g = gamma[o], be = beta[o];
    const float *zr = z + r * P + 4 * q;
    float y[4];
#pragma unroll
    for (int i = 0; i < 4; i++) y[i] = __builtin_fmaf((zr[i] - mu) * rstd, g, be);   // (T2) the affine first, gamma of either sign
    int am = 0;
#pragma unroll
    for (int i = 1; i < 4; i++)
      if (y[i] > y[am]) am = i;                                                      // (T3) first maximum wins, like nn.MaxPool1d
    const float v = y[am];
    a[idx] = fmaxf(v, 0.f);
    if (sel) sel[idx] = (unsigned char)(v > 0.f ? am : 4);                           // (T3) 4 matches no window position: no gradient
  }
}

// per clip: mean over time (M5Net.py:34), fc1, log_softmax (M5Net.py:37-38).  dlogp given: the backward of the three --
// dlogit = dlogp - softmax sum(dlogp) and feat left for the fc1 gradients, da4[c][q] = (fc1.weight^T dlogit)[c] / Q4
__global__ __launch_bounds__(128) void m5t_head_kernel(const float *__restrict__ a4, const float *__restrict__ fcw,
                                                       const float *__restrict__ fcb, float *__restrict__ logprobs,
                                                       const float *__restrict__ dlogp, float *__restrict__ feat_out,
                                                       float *__restrict__ dlogit_out, float *__restrict__ da4, int c2, int Q4,
                                                       int n_out) {
  __shared__ float feat[128], logit[64], dlogit[64];
  const int b = blockIdx.x;
  const float *ab = a4 + (size_t)b * c2 * Q4;
  for (int c = threadIdx.x; c < c2; c += blockDim.x) {
    float s = 0.f;
    for (int q = 0; q < Q4; q++) s += ab[c * Q4 + q];
    feat[c] = s / (float)Q4;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < n_out; o += blockDim.x) {
    float s = 0.f;
    for (int c = 0; c < c2; c++) s = __builtin_fmaf(fcw[o * c2 + c], feat[c], s);
    logit[o] = s + fcb[o];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float mx = logit[0];
    for (int o = 1; o < n_out; o++) mx = fmaxf(mx, logit[o]);
    float se = 0.f;
    for (int o = 0; o < n_out; o++) se += expf(logit[o] - mx);
    if (!dlogp) {
      const float lse = mx + logf(se);
      for (int o = 0; o < n_out; o++) logprobs[(size_t)b * n_out + o] = logit[o] - lse;
    } else {
      float sd = 0.f;
      for (int o = 0; o < n_out; o++) sd += dlogp[(size_t)b * n_out + o];
      for (int o = 0; o < n_out; o++) {
        dlogit[o] = dlogp[(size_t)b * n_out + o] - expf(logit[o] - mx) / se * sd;
        dlogit_out[(size_t)b * n_out + o] = dlogit[o];
      }
    }
  }
  if (!dlogp) return;
  __syncthreads();
  for (int c = threadIdx.x; c < c2; c += blockDim.x) {
    feat_out[(size_t)b * c2 + c] = feat[c];
    float s = 0.f;
    for (int o = 0; o < n_out; o++) s = __builtin_fmaf(fcw[o * c2 + c], dlogit[o], s);
    for (int q = 0; q < Q4; q++) da4[((size_t)b * c2 + c) * Q4 + q] = s / (float)Q4;
  }
}

// d fc1.weight[o][c] = sum_b dlogit[b][o] feat[b][c], d fc1.bias[o] = sum_b dlogit[b][o]: one thread each, clips in order, fp64
__global__ __launch_bounds__(256) void m5t_fc_grad_kernel(const float *__restrict__ dlogit, const float *__restrict__ feat,
                                                          float *__restrict__ dw, float *__restrict__ db, int B, int c2, int n_out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_out * c2 + n_out) return;
  double s = 0.0;
  if (e < n_out * c2) {
    const int o = e / c2, c = e % c2;
    for (int b = 0; b < B; b++) s += (double)dlogit[(size_t)b * n_out + o] * (double)feat[(size_t)b * c2 + c];
    dw[e] = (float)s;
  } else {
    const int o = e - n_out * c2;
    for (int b = 0; b < B; b++) s += (double)dlogit[(size_t)b * n_out + o];
    db[o] = (float)s;
  }
}

// dy is da routed through the selection bytes (T3): part[slice][o] = (sum dy, sum dy xhat) -- only selected positions carry a dy
__global__ __launch_bounds__(256) void m5t_bstats_kernel(const float *__restrict__ z, const unsigned char *__restrict__ sel,
                                                         const float *__restrict__ da, const float *__restrict__ stat,
                                                         double *__restrict__ part, int B, int co, int P, int Q) {
  const int o = blockIdx.x, sl = blockIdx.y;
  const float mu = stat[o], rstd = stat[co + o];
  double s1 = 0.0, s2 = 0.0;
  for (int b = sl; b < B; b += M5T_SLICES) {
    const size_t r = (size_t)b * co + o;
    for (int q = threadIdx.x; q < Q; q += 256) {
      const int w = sel[r * Q + q];
      if (w < 4) {
        const float g = da[r * Q + q], xh = (z[r * P + 4 * q + w] - mu) * rstd;
        s1 += (double)g;
        s2 += (double)g * (double)xh;
      }
    }
  }
  block_wave_sum2(s1, s2);
  if (threadIdx.x == 0) {
    part[((size_t)sl * co + o) * 2] = s1;
    part[((size_t)sl * co + o) * 2 + 1] = s2;
  }
}

// (bn_bstats_final_kernel: d bn.bias = sum dy, d bn.weight = sum dy xhat; mean2[o] = their means over all n positions)

// dz = gamma rstd (dy - mean(dy) - xhat mean(dy xhat)) at EVERY position p < P: (T1) those at and beyond 4 Q have dy = 0 and still a
// dz through the two mean terms.  part[slice][o] = (sum dz, 0): the conv bias gradient, zero in exact arithmetic, computed anyway.
__global__ __launch_bounds__(256) void m5t_dz_kernel(const float *__restrict__ z, const unsigned char *__restrict__ sel,
                                                     const float *__restrict__ da, const float *__restrict__ stat,
                                                     const double *__restrict__ mean2, const float *__restrict__ gamma, float *__restrict__ dz,
                                                     double *__restrict__ part, int B, int co, int P, int Q) {
  const int o = blockIdx.x, sl = blockIdx.y;
  const float mu = stat[o], rstd = stat[co + o], m1 = (float)mean2[2 * o], m2 = (float)mean2[2 * o + 1], gr = gamma[o] * rstd;
  double s1 = 0.0, s2 = 0.0;
  for (int b = sl; b < B; b += M5T_SLICES) {
    const size_t r = (size_t)b * co + o;
    for (int p = threadIdx.x; p < P; p += 256) {
      const int q = p >> 2;
      float dy = 0.f;
      if (q < Q && sel[r * Q + q] == (p & 3)) dy = da[r * Q + q];
      const float xh = (z[r * P + p] - mu) * rstd;
      const float v = gr * (dy - m1 - xh * m2);
      dz[r * P + p] = v;
      s1 += (double)v;
    }
  }
  block_wave_sum2(s1, s2);
  if (threadIdx.x == 0) {
    part[((size_t)sl * co + o) * 2] = s1;
    part[((size_t)sl * co + o) * 2 + 1] = 0.0;
  }
}

// split-K weight gradient: dW[o][c][t] = sum_{b,p} dz[b][o][p] in[b][c][p s + t] over EVERY p < P (T1).  One workgroup per (64 (c, t)
// pairs, M5T_OB output channels, slice): a lane owns one (c, t) and M5T_OB accumulators, so an input sample is loaded once for M5T_OB FMAs
// and the dz values, the same for every lane, come through the scalar path.  The work items (clip, chunk of 128 positions) go round the
// 64 slices, and a slice's items round the workgroup's 8 waves -- the loop is bound by load latency, so waves in flight are what it
// needs.  A chunk is summed in fp32, a wave's chunks in fp64, the waves in wave order through LDS: a fixed order.
// grid (ceil(ci k / 64), ceil(co / M5T_OB), slices)
constexpr int M5T_OB = 8, M5T_DW_WAVES = 8;
__global__ __launch_bounds__(64 * M5T_DW_WAVES) void m5t_dw_kernel(const float *__restrict__ dz, const float *__restrict__ in,
                                                                   float *__restrict__ wpart, int B, int ci, int co, int k, int s, int Lin,
                                                                   int P, int nW) {
  __shared__ double sm[M5T_DW_WAVES][M5T_OB][64];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int cik = ci * k, r0 = blockIdx.x * 64 + lane, o0 = blockIdx.y * M5T_OB, sl = blockIdx.z;
  const int r = r0 < cik ? r0 : cik - 1;                                      // a lane past the end re-reads the last pair, and stores nothing
  const int c = r / k, t = r % k;
  const int nchunk = (P + M5T_CHUNK - 1) / M5T_CHUNK;
  const long items = (long)B * nchunk;
  int orow[M5T_OB];
#pragma unroll
  for (int i = 0; i < M5T_OB; i++) orow[i] = o0 + i < co ? o0 + i : co - 1;   // likewise a channel past the end
  double tot[M5T_OB];
#pragma unroll
  for (int i = 0; i < M5T_OB; i++) tot[i] = 0.0;
  for (long w = sl + (long)wv * M5T_SLICES; w < items; w += (long)M5T_SLICES * M5T_DW_WAVES) {
    const int b = (int)(w / nchunk), p0 = (int)(w % nchunk) * M5T_CHUNK, p1 = p0 + M5T_CHUNK < P ? p0 + M5T_CHUNK : P;
    const float *dzb = dz + (size_t)b * co * P;
    const float *ar = in + ((size_t)b * ci + c) * Lin + t;
    float acc[M5T_OB];
#pragma unroll
    for (int i = 0; i < M5T_OB; i++) acc[i] = 0.f;
#pragma unroll 8
    for (int p = p0; p < p1; p++) {                              // (unrolled: eight positions' loads in flight)
      const float a = ar[(size_t)p * s];
#pragma unroll
      for (int i = 0; i < M5T_OB; i++) acc[i] = __builtin_fmaf(dzb[(size_t)orow[i] * P + p], a, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < M5T_OB; i++) tot[i] += (double)acc[i];
  }
#pragma unroll
  for (int i = 0; i < M5T_OB; i++) sm[wv][i][lane] = tot[i];
  __syncthreads();
  if (wv == 0 && r0 < cik) {
#pragma unroll
    for (int i = 0; i < M5T_OB; i++) {
      double v = sm[0][i][lane];
      for (int j = 1; j < M5T_DW_WAVES; j++) v += sm[j][i][lane];
      if (o0 + i < co) wpart[(size_t)sl * nW + (size_t)(o0 + i) * cik + r0] = (float)v;
    }
  }
}

// the stage's input gradient, gathered: din[b][c][j] = sum_o sum_{p: 0 <= j - p s < k} w[o][c][j - p s] dz[b][o][p], p up to P - 1 (T1:
// m5_stage_bwd stops at 4 Q - 1 because in eval mode the dropped positions carry nothing; here they do)
__global__ __launch_bounds__(256) void m5t_din_kernel(const float *__restrict__ dz, const float *__restrict__ w, float *__restrict__ din,
                                                      int B, int ci, int co, int k, int s, int Lin, int P) {
  const size_t total = (size_t)B * ci * Lin;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int j = (int)(idx % Lin);
    const size_t r = idx / Lin;
    const int c = (int)(r % ci), b = (int)(r / ci);
    const int plo = j - k + 1 <= 0 ? 0 : (j - k + 1 + s - 1) / s;
    int phi = j / s;
    if (phi > P - 1) phi = P - 1;
    float acc = 0.f;
    for (int p = plo; p <= phi; p++) {
      const int t = j - p * s;
      const float *wr = w + (size_t)c * k + t;
      const float *dzr = dz + (size_t)b * co * P + p;
      for (int o = 0; o < co; o++) acc = __builtin_fmaf(wr[(size_t)o * ci * k], dzr[(size_t)o * P], acc);
    }
    din[idx] = acc;
  }
}

}  // namespace

size_t m5_train_workspace_bytes(const ap_m5 *m, int B, int L) {
  M5TPlan pl;
  if (m5t_plan(m, B, L, &pl)) return 0;
  return pl.total;
}

int launch_m5_train_fwd(ap_m5 *m, const float *blob, const float *x, float *logprobs, float *new_running, float momentum, void *ws,
                        size_t ws_bytes, int keep, int B, int L, hipStream_t st) {
  M5TPlan pl;
  if (int rc = m5t_plan(m, B, L, &pl)) return rc;
  if (ws_bytes < pl.total) { set_error("m5 train: workspace of %zu bytes, %zu needed", ws_bytes, pl.total); return -22; }
  if (!(momentum >= 0.f && momentum <= 1.f)) { set_error("m5 train: momentum %g outside [0, 1]", (double)momentum); return -22; }
  char *base = (char *)ws;
  M5TPack pk;
  for (int i = 0; i < 4; i++) {
    pk.w[i] = blob + pl.bw[i]; pk.wT[i] = (float *)(base + pl.wT[i]); pk.co[i] = pl.co[i]; pk.cik[i] = pl.ci[i] * pl.k[i];
  }
  m5t_pack_kernel<<<dim3(grid_for(pl.nw_max), 4), 256, 0, st>>>(pk);
  const float *in = x;
  for (int i = 0; i < 4; i++) {
    const int co = pl.co[i], P = pl.P[i], Q = pl.Q[i];
    // keep = 0 (no_grad): nothing is left for a backward -- every stage's z goes through stage 1's region, no selection bytes
    float *z = (float *)(base + pl.z[keep ? i : 0]);
    float *a = (float *)(base + pl.a[i]), *stat = (float *)(base + pl.stat[i]);
    double *part = (double *)(base + pl.part);
    m5t_conv_kernel<<<grid_for((size_t)B * ((P + 3) / 4) * co), 256, 0, st>>>(in, pk.wT[i], blob + pl.bb[i], z, B, pl.ci[i], co, pl.k[i],
                                                                           pl.s[i], pl.lin[i], P);
    m5t_stats_kernel<<<dim3(co, M5T_SLICES), 256, 0, st>>>(z, part, B, co, P);
    bn_stats_final_kernel<M5T_SLICES><<<(co + 63) / 64, 64, 0, st>>>(part, blob + pl.brm[i], blob + pl.brv[i], stat, new_running + pl.rm[i],
                                                                   new_running + pl.rv[i], co, (double)B * P, m->eps, momentum);
    m5t_apply_kernel<<<grid_for((size_t)B * co * Q), 256, 0, st>>>(z, stat, blob + pl.bg[i], blob + pl.bbe[i], a,
                                                                 keep ? (unsigned char *)(base + pl.sel[i]) : nullptr, B, co, P, Q);
    in = a;
  }
  m5t_head_kernel<<<B, 128, 0, st>>>(in, blob + pl.bfw, blob + pl.bfb, logprobs, nullptr, nullptr, nullptr, nullptr, pl.co[3], pl.Q[3],
                                    m->n_output);
  AP_HIP(hipGetLastError());
  return 0;
}

int launch_m5_train_bwd(ap_m5 *m, const float *blob, const float *x, const float *dlogp, float *grads, float *dx, void *ws, size_t ws_bytes,
                        int B, int L, hipStream_t st) {
  M5TPlan pl;
  if (int rc = m5t_plan(m, B, L, &pl)) return rc;
  if (ws_bytes < pl.total) { set_error("m5 train: workspace of %zu bytes, %zu needed", ws_bytes, pl.total); return -22; }
  char *base = (char *)ws;
  float *da[2] = {(float *)(base + pl.da[0]), (float *)(base + pl.da[1])};
  float *feat = (float *)(base + pl.feat), *dlogit = (float *)(base + pl.dlogit), *dzb = (float *)(base + pl.dz);
  float *wpart = (float *)(base + pl.wpart);
  double *part = (double *)(base + pl.part), *mean2 = (double *)(base + pl.mean2);
  const int c2 = pl.co[3], n_out = m->n_output;
  m5t_head_kernel<<<B, 128, 0, st>>>((const float *)(base + pl.a[3]), blob + pl.bfw, blob + pl.bfb, nullptr, dlogp, feat, dlogit, da[0], c2,
                                    pl.Q[3], n_out);
  m5t_fc_grad_kernel<<<(n_out * c2 + n_out + 255) / 256, 256, 0, st>>>(dlogit, feat, grads + pl.gfw, grads + pl.gfb, B, c2, n_out);
  int cur = 0;
  for (int i = 3; i >= 0; i--) {
    const int ci = pl.ci[i], co = pl.co[i], k = pl.k[i], s = pl.s[i], P = pl.P[i], Q = pl.Q[i], lin = pl.lin[i];
    const int nW = co * ci * k;
    const float *z = (const float *)(base + pl.z[i]);
    const unsigned char *sel = (const unsigned char *)(base + pl.sel[i]);
    const float *stat = (const float *)(base + pl.stat[i]);
    const float *in = i ? (const float *)(base + pl.a[i - 1]) : x;
    m5t_bstats_kernel<<<dim3(co, M5T_SLICES), 256, 0, st>>>(z, sel, da[cur], stat, part, B, co, P, Q);
    bn_bstats_final_kernel<M5T_SLICES><<<(co + 63) / 64, 64, 0, st>>>(part, mean2, grads + pl.gg[i], grads + pl.gbe[i], co, (double)B * P);
    m5t_dz_kernel<<<dim3(co, M5T_SLICES), 256, 0, st>>>(z, sel, da[cur], stat, mean2, blob + pl.bg[i], dzb, part, B, co, P, Q);
    slice_sum_kernel<double, M5T_SLICES><<<(co + 255) / 256, 256, 0, st>>>(part, grads + pl.gb[i], (size_t)co, /* slices: the template's */ 0, 2, 1.0f, 0);
    m5t_dw_kernel<<<dim3((ci * k + 63) / 64, (co + M5T_OB - 1) / M5T_OB, M5T_SLICES), 64 * M5T_DW_WAVES, 0, st>>>(dzb, in, wpart, B, ci, co, k, s, lin, P, nW);
    slice_sum_kernel<float, M5T_SLICES><<<(nW + 255) / 256, 256, 0, st>>>(wpart, grads + pl.gw[i], (size_t)nW, /* slices: the template's */ 0, 1, 1.0f, 0);
    if (i > 0) {
      m5t_din_kernel<<<grid_for((size_t)B * ci * lin), 256, 0, st>>>(dzb, blob + pl.bw[i], da[cur ^ 1], B, ci, co, k, s, lin, P);
      cur ^= 1;
    } else if (dx) {
      m5t_din_kernel<<<grid_for((size_t)B * ci * lin), 256, 0, st>>>(dzb, blob + pl.bw[i], dx, B, ci, co, k, s, lin, P);
    }
  }
  AP_HIP(hipGetLastError());
  return 0;
}

}  // namespace ap
