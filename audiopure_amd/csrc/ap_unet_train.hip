// Train-mode step of the Improved-Diffusion UNet (improved_diffusion/train_util.py:191-229: losses = diffusion.training_losses(...),
// loss.backward(); gaussian_diffusion.py:709-746 MSE on eps; unet.py:150-197 ResBlock with nn.Dropout(p) behind the FiLM-ed
// GroupNorm).  The convolutions' weight gradients are ap_conv2d_wgrad, their biases ap_rowsum, the input-gradient sweep is
// ap_unet_bwd.hip's; what the parameters add to it is here:
//   ap_groupnorm_train_bwd   GroupNorm32 + scale-shift + activation backward with EVERY cotangent (dx, d gamma, d beta, d scale-shift)
//   ap_dropout               nn.Dropout on a counter-based (Philox4x32-10) mask: nothing stored, the backward is the same call on dy
//   ap_silu_bwd              dx = dy silu'(x)
//   ap_qsample_rows          q_sample with one diffusion step per sample
// Plain fp32, no floating-point atomics: every sum has a fixed order, sums over the batch run in fp64 and round once.
#include "ap_common.h"

namespace ap {
namespace {

// One workgroup per (sample, group) slab.  Notation of groupnorm_bwd_kernel (ap_unet_bwd.hip): xh = (x - mean) rstd, y0 = gamma xh +
// beta, y1 = y0 (1 + sc) + sh, e = dy act'(y1).  Per channel c of the group, in channel order:
//   S1 = sum_hw e, S2 = sum_hw e xh   ->   dss[b][c] = gamma S2 + beta S1 (= sum e y0), dss[b][C + c] = S1, sums[b][c] = (S1, S2)
// and with k = gamma (1 + sc):  m1 = sum_c k S1 / n, m2 = sum_c k S2 / n,  dx = rstd (e k - m1 - xh m2).
__global__ __launch_bounds__(256) void groupnorm_train_bwd_kernel(const float *__restrict__ x, const float *__restrict__ gamma,
                                                                  const float *__restrict__ beta, const float *__restrict__ ss,
                                                                  const float *__restrict__ dy, float *__restrict__ dx,
                                                                  float *__restrict__ dss, float *__restrict__ sums, int C, int HW,
                                                                  int groups, float eps, int act) {
  // two trees at once (block_tree2), in fp64: the per-thread partials are fp32 sums of n / 256 terms
  __shared__ double red[512];
  const int b = blockIdx.x / groups, g = blockIdx.x % groups, cpg = C / groups;
  const size_t n = (size_t)cpg * HW;
  const size_t off = ((size_t)b * C + (size_t)g * cpg) * HW;
  const float *xp = x + off, *dyp = dy + off;
  float s = 0.f;
  for (size_t i = threadIdx.x; i < n; i += 256) s += xp[i];
  double t0 = (double)s, t1 = 0.0;
  block_tree2<256>(t0, t1, red, SumOp{});
  __syncthreads();
  const float mean = (float)(t0 / (double)n);
  float v = 0.f;
  for (size_t i = threadIdx.x; i < n; i += 256) {
    const float dlt = xp[i] - mean;
    v = __builtin_fmaf(dlt, dlt, v);
  }
  t0 = (double)v;
  t1 = 0.0;
  block_tree2<256>(t0, t1, red, SumOp{});
  __syncthreads();
  const float rstd = 1.0f / sqrtf((float)(t0 / (double)n) + eps);

  double a1 = 0.0, a2 = 0.0;                                  // sum_c k S1, sum_c k S2: the same value in every thread
  for (int cc = 0; cc < cpg; cc++) {
    const int c = g * cpg + cc;
    const float gm = gamma[c], bt = beta[c];
    const float sc = ss ? 1.0f + ss[(size_t)b * 2 * C + c] : 1.0f, sh = ss ? ss[(size_t)b * 2 * C + C + c] : 0.f;
    const float *xc = xp + (size_t)cc * HW, *dc = dyp + (size_t)cc * HW;
    float s1 = 0.f, s2 = 0.f;
    for (int i = threadIdx.x; i < HW; i += 256) {
      const float xh = (xc[i] - mean) * rstd;
      const float e = act_grad(dc[i], (xh * gm + bt) * sc + sh, act);
      s1 += e;
      s2 = __builtin_fmaf(e, xh, s2);
    }
    double S1 = (double)s1, S2 = (double)s2;
    block_tree2<256>(S1, S2, red, SumOp{});
    __syncthreads();
    if (threadIdx.x == 0) {
      if (dss) {
        dss[(size_t)b * 2 * C + c] = (float)((double)gm * S2 + (double)bt * S1);
        dss[(size_t)b * 2 * C + C + c] = (float)S1;
      }
      if (sums) {
        sums[((size_t)b * C + c) * 2] = (float)S1;
        sums[((size_t)b * C + c) * 2 + 1] = (float)S2;
      }
    }
    const double k = (double)gm * (double)sc;
    a1 += k * S1;
    a2 += k * S2;
  }
  if (!dx) return;
  const float m1 = (float)(a1 / (double)n), m2 = (float)(a2 / (double)n);
  float *dxp = dx + off;
  for (int cc = 0; cc < cpg; cc++) {
    const int c = g * cpg + cc;
    const float gm = gamma[c], bt = beta[c];
    const float sc = ss ? 1.0f + ss[(size_t)b * 2 * C + c] : 1.0f, sh = ss ? ss[(size_t)b * 2 * C + C + c] : 0.f;
    const float k = gm * sc;
    const float *xc = xp + (size_t)cc * HW, *dc = dyp + (size_t)cc * HW;
    float *oc = dxp + (size_t)cc * HW;
    for (int i = threadIdx.x; i < HW; i += 256) {
      const float xh = (xc[i] - mean) * rstd;
      const float e = act_grad(dc[i], (xh * gm + bt) * sc + sh, act);
      oc[i] = rstd * (e * k - m1 - xh * m2);
    }
  }
}

// d beta[c] = sum_b (1 + sc[b][c]) S1[b][c], d gamma[c] = sum_b (1 + sc[b][c]) S2[b][c]: one thread per channel, b ascending, fp64
__global__ void groupnorm_param_kernel(const float *__restrict__ sums, const float *__restrict__ ss, float *__restrict__ dgamma,
                                       float *__restrict__ dbeta, int B, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double g = 0.0, bsum = 0.0;
  for (int b = 0; b < B; b++) {
    const double k = ss ? 1.0 + (double)ss[(size_t)b * 2 * C + c] : 1.0;
    bsum += k * (double)sums[((size_t)b * C + c) * 2];
    g += k * (double)sums[((size_t)b * C + c) * 2 + 1];
  }
  if (dgamma) dgamma[c] = (float)g;
  if (dbeta) dbeta[c] = (float)bsum;
}

// one thread per quad of a sample (blockIdx.y): elements 4 q .. 4 q + 3 below n; scalar accesses (n need not be a multiple of 4, so
// a sample's base has no alignment beyond 4 bytes).  copy != 0 (p = 0): the bits of x.
__global__ __launch_bounds__(256) void dropout_kernel(const float *__restrict__ x, float *__restrict__ y, int n, float p, float s,
                                                      uint64_t seed, uint32_t draw, uint64_t sample_offset, int copy) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if ((size_t)q * 4 >= (size_t)n) return;
  const uint64_t sample = sample_offset + blockIdx.y;
  const size_t base = (size_t)blockIdx.y * n + (size_t)q * 4;
  const int cnt = min(4, n - q * 4);
  if (copy) {
    for (int l = 0; l < cnt; l++) y[base + l] = x[base + l];
    return;
  }
  uint32_t r[4];
  philox4x32_10((uint32_t)q, draw, (uint32_t)sample, (uint32_t)(sample >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    if (l < cnt) {
      const float u = (float)(r[l] >> 8) * 5.9604644775390625e-08f;       // [0, 1), 2^-24
      y[base + l] = u >= p ? x[base + l] * s : 0.f;
    }
  }
}

__global__ void silu_bwd_kernel(const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ dx, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  dx[i] = act_grad(dy[i], x[i], 2);
}

__global__ void qsample_rows_kernel(const float *__restrict__ x0, const float *__restrict__ z, const float *__restrict__ a,
                                    const float *__restrict__ b, float *__restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t o = (size_t)blockIdx.y * n + i;
  out[o] = a[blockIdx.y] * x0[o] + b[blockIdx.y] * z[o];
}

}  // namespace
}  // namespace ap

using namespace ap;

extern "C" size_t ap_groupnorm_train_workspace_bytes(int B, int C) {
  if (B < 1 || C < 1) return 0;
  return (size_t)B * C * 2 * sizeof(float);
}

extern "C" int ap_groupnorm_train_bwd(const float *x, const float *gamma, const float *beta, const float *scale_shift, const float *dy,
                                      float *dx, float *dgamma, float *dbeta, float *dss, void *workspace, size_t ws_bytes, int B, int C,
                                      int HW, int groups, float eps, int act, void *stream) {
  if (!x || !gamma || !beta || !dy || B < 1 || C < 1 || HW < 1 || groups < 1 || C % groups || act < 0 || act > 2) {
    set_error("ap_groupnorm_train_bwd: bad argument");
    return -22;
  }
  if (B > 65535 || (long long)B * groups > 0x7fffffffLL) { set_error("ap_groupnorm_train_bwd: B = %d not served", B); return -22; }
  if (!scale_shift && dss) { set_error("ap_groupnorm_train_bwd: dss without scale_shift"); return -22; }
  if (!dx && !dgamma && !dbeta && !dss) { set_error("ap_groupnorm_train_bwd: no output asked for"); return -22; }
  const bool params = dgamma || dbeta;
  if (params && (!workspace || ws_bytes < ap_groupnorm_train_workspace_bytes(B, C) || ((uintptr_t)workspace & 3))) {
    set_error("ap_groupnorm_train_bwd: workspace of %zu bytes needed, %zu given", ap_groupnorm_train_workspace_bytes(B, C), ws_bytes);
    return -22;
  }
  hipStream_t st = (hipStream_t)stream;
  float *sums = params ? (float *)workspace : nullptr;
  groupnorm_train_bwd_kernel<<<(unsigned)(B * groups), 256, 0, st>>>(x, gamma, beta, scale_shift, dy, dx, dss, sums, C, HW, groups, eps,
                                                                    act);
  if (params) groupnorm_param_kernel<<<(unsigned)((C + 63) / 64), 64, 0, st>>>(sums, scale_shift, dgamma, dbeta, B, C);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_dropout(const float *x, float *y, int B, int n, float p, uint64_t seed, uint32_t draw, uint64_t sample_offset,
                          void *stream) {
  if (!x || !y || B < 1 || n < 1 || B > 65535) { set_error("ap_dropout: bad argument"); return -22; }
  if (!(p >= 0.f) || !(p < 1.f)) { set_error("ap_dropout: p = %g outside [0, 1)", (double)p); return -22; }
  const float s = (float)(1.0 / (1.0 - (double)p));
  const int nq = (n + 3) / 4;
  dropout_kernel<<<dim3((unsigned)((nq + 255) / 256), (unsigned)B), 256, 0, (hipStream_t)stream>>>(x, y, n, p, s, seed, draw,
                                                                                                 sample_offset, p == 0.f);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_silu_bwd(const float *x, const float *dy, float *dx, size_t n, void *stream) {
  if (!x || !dy || !dx || n < 1 || n > ((size_t)0x7fffffff) * 256) { set_error("ap_silu_bwd: bad argument"); return -22; }
  silu_bwd_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, dy, dx, n);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_qsample_rows(const float *x0, const float *z, const float *a, const float *b, float *out, int B, int n, void *stream) {
  if (!x0 || !z || !a || !b || !out || B < 1 || n < 1 || B > 65535) { set_error("ap_qsample_rows: bad argument"); return -22; }
  qsample_rows_kernel<<<dim3((unsigned)((n + 255) / 256), (unsigned)B), 256, 0, (hipStream_t)stream>>>(x0, z, a, b, out, n);
  AP_HIP(hipGetLastError());
  return 0;
}
