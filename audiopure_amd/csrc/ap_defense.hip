// Baseline defenses of the reference's attack scripts (`--defense AS | MS | AT | DS | LPF | BPF`):
// transforms/time_defense.py and transforms/frequency_defense.py, forward and input-gradient (adjoint) launches.
// All fp32 on x[B][L] (any L >= 1), asynchronous on the caller's stream, no host read of device data.
//
//  AS   moving average, one thread per output; the operator is symmetric Toeplitz, so its adjoint is the same launch.
//  MS   median of the zero-padded window, one thread per output over an LDS tile; the forward also writes the offset of the
//       argmedian, and the backward is a gather over those offsets (no atomics, fixed order).
//  AT   one workgroup per clip: power reduction, then y = x + z sqrt(P / snr); the backward carries the term through P.
//  DS   2:1 down then 1:2 up with torchaudio's sinc/Hann^2 kernels, fused: an x tile -> the 8 kHz samples in LDS -> both
//       output phases.  The backward is the transposed pair, fused the same way.
//  IIR  (LPF / BPF) direct-form-II-transposed recurrence, parallel in time: (1) every 128-sample chunk is filtered from zero
//       state (the chunk staged in LDS, one thread per chunk, fp64 state) and its end state kept; (2) one thread per clip carries the
//       state across chunks, S_{c+1} = A^128 S_c + e_c (exact in exact arithmetic: no truncated warm-up); (3) one thread
//       per sample adds the zero-input response H[k] . S_c and clamps.  The adjoint is the same three passes run backwards
//       in time on g * 1[lo <= y_pre <= hi].  The clamp range is decided on the device from a batch min/max (pass 1).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "ap_common.h"

namespace ap {
namespace {

constexpr int MS_MAX_WIN = 63;
constexpr int IIR_MAXCOEF = 16;
constexpr int IIR_CHUNK = AP_IIR_CHUNK;
constexpr int IIR_CPB = 64;          // chunks per pass-1 workgroup (one wave, one chunk per lane)
constexpr int DS_NT = 256;           // 8 kHz-rate output pairs per DS workgroup (512 output samples)
constexpr int DS_ND = DS_NT + 14;    // 8 kHz samples one tile needs (15-tap up kernel)
constexpr int DS_NX = 2 * DS_NT + 54;  // input samples the forward stages (28-tap down kernel, stride 2)
constexpr int DS_NG = 2 * DS_NT + 56;  // cotangent samples the backward stages

int bad(const char *fmt, ...) {
  char buf[400];
  va_list v;
  va_start(v, fmt);
  vsnprintf(buf, sizeof(buf), fmt, v);
  va_end(v);
  set_error("%s", buf);
  return -22;
}

int check_bl(const char *who, const void *a, const void *b, const void *c, int B, int L) {
  if (!a || !b || !c) return bad("%s: NULL tensor argument", who);
  if (B < 1 || B > 65535 || L < 1) return bad("%s: need 1 <= B <= 65535 and L >= 1 (got B = %d, L = %d)", who, B, L);
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ AS
__global__ __launch_bounds__(256) void avg_smooth_kernel(const float *__restrict__ x, float *__restrict__ y, int r, float w,
                                                         int L) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= L) return;
  const float *xb = x + (size_t)blockIdx.y * L;
  const int lo = max(n - r, 0), hi = min(n + r, L - 1);
  float acc = 0.f;
  for (int j = lo; j <= hi; ++j) acc = fmaf(w, xb[j], acc);
  y[(size_t)blockIdx.y * L + n] = acc;
}

// ------------------------------------------------------------------------------------------------------------------ MS
// The argmedian is the window element of rank r in the order (value, then position): rank(j) = #{i : v_i < v_j} +
// #{i < j : v_i == v_j}.  Exactly one element has rank r, so ties go to the middle one of the equal run in window order.
__global__ __launch_bounds__(256) void median_smooth_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                            int8_t *__restrict__ off, int r, int L) {
  __shared__ float s[256 + 2 * MS_MAX_WIN];
  const int b = blockIdx.y, n0 = blockIdx.x * 256, k = 2 * r + 1;
  const float *xb = x + (size_t)b * L;
  for (int i = threadIdx.x; i < 256 + 2 * r; i += 256) {
    const int p = n0 - r + i;
    s[i] = (p >= 0 && p < L) ? xb[p] : 0.f;
  }
  __syncthreads();
  const int n = n0 + threadIdx.x;
  if (n >= L) return;
  const float *v = s + threadIdx.x;
  int pick = r;
  for (int j = 0; j < k; ++j) {
    const float vj = v[j];
    int rank = 0;
    for (int i = 0; i < k; ++i) rank += (v[i] < vj) || (i < j && v[i] == vj);
    if (rank == r) { pick = j; break; }
  }
  y[(size_t)b * L + n] = v[pick];
  off[(size_t)b * L + n] = (int8_t)(pick - r);
}

// dx[m] = sum over n in [m - r, m + r] with n + off[n] == m of g[n], n ascending
__global__ __launch_bounds__(256) void median_smooth_bwd_kernel(const float *__restrict__ g, const int8_t *__restrict__ off,
                                                                float *__restrict__ dx, int r, int L) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= L) return;
  const size_t base = (size_t)blockIdx.y * L;
  float acc = 0.f;
  const int lo = max(m - r, 0), hi = min(m + r, L - 1);
  for (int n = lo; n <= hi; ++n)
    if (n + (int)off[base + n] == m) acc += g[base + n];
  dx[base + m] = acc;
}

// ------------------------------------------------------------------------------------------------------------------ AT
__device__ __forceinline__ float block_sum_1024(float v, float *sh) {   // wave_sum per wave, then over the sixteen waves' sums
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();                                  // sh may still be read by a previous call
  if (lane == 0) sh[wv] = v;
  __syncthreads();
  v = lane < 16 ? sh[lane] : 0.f;
  v = wave_sum<16>(v);
  return __shfl(v, 0);
}

__global__ __launch_bounds__(1024) void at_fwd_kernel(const float *__restrict__ x, const float *__restrict__ z,
                                                      float *__restrict__ y, float snr, int L) {
  __shared__ float sh[16];
  const size_t base = (size_t)blockIdx.x * L;
  float ss = 0.f;
  for (int i = threadIdx.x; i < L; i += 1024) ss = fmaf(x[base + i], x[base + i], ss);
  const float P = block_sum_1024(ss, sh) / (float)L;
  const float s = sqrtf(P / snr);
  for (int i = threadIdx.x; i < L; i += 1024) y[base + i] = x[base + i] + z[base + i] * s;
}

// dx = g + (sum g z) x / (L snr s), s = sqrt(P / snr); a silent clip (s == 0) drops the P term (its factor x is 0 there)
__global__ __launch_bounds__(1024) void at_bwd_kernel(const float *__restrict__ x, const float *__restrict__ z,
                                                      const float *__restrict__ g, float *__restrict__ dx, float snr, int L) {
  __shared__ float sh[16];
  const size_t base = (size_t)blockIdx.x * L;
  float ss = 0.f, gz = 0.f;
  for (int i = threadIdx.x; i < L; i += 1024) {
    ss = fmaf(x[base + i], x[base + i], ss);
    gz = fmaf(g[base + i], z[base + i], gz);
  }
  const float P = block_sum_1024(ss, sh) / (float)L;
  const float GZ = block_sum_1024(gz, sh);
  const float s = sqrtf(P / snr);
  const float c = s > 0.f ? GZ / ((float)L * snr * s) : 0.f;
  for (int i = threadIdx.x; i < L; i += 1024) dx[base + i] = fmaf(c, x[base + i], g[base + i]);
}

// ------------------------------------------------------------------------------------------------------------------ DS
struct DsTaps {
  float kd[AP_DS_DOWN_TAPS];          // 16 k -> 8 k, stride 2, input offset -13
  float ku[2][AP_DS_UP_TAPS];         // 8 k -> 16 k, phase p of output 2n + p, 8 k offset -7
};

// y[2n + p] = sum_j ku[p][j] d[n + j - 7],  d[m] = sum_j kd[j] x[2m + j - 13] for 0 <= m < M (else 0), t < Lout
__global__ __launch_bounds__(256) void ds_fwd_kernel(const float *__restrict__ x, float *__restrict__ y, DsTaps t, int L,
                                                     int M, int Lout) {
  __shared__ float sx[DS_NX], sd[DS_ND];
  const int b = blockIdx.y, n0 = blockIdx.x * DS_NT;
  const float *xb = x + (size_t)b * L;
  const int xbase = 2 * n0 - 27;
  for (int i = threadIdx.x; i < DS_NX; i += 256) {
    const int p = xbase + i;
    sx[i] = (p >= 0 && p < L) ? xb[p] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < DS_ND; i += 256) {
    const int m = n0 - 7 + i;
    float acc = 0.f;
    if (m >= 0 && m < M) {
#pragma unroll
      for (int j = 0; j < AP_DS_DOWN_TAPS; ++j) acc = fmaf(t.kd[j], sx[2 * i + j], acc);
    }
    sd[i] = acc;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int tl = threadIdx.x + 256 * q, tt = 2 * n0 + tl;
    if (tt >= Lout) continue;
    const int ph = tl & 1, nl = tl >> 1;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < AP_DS_UP_TAPS; ++j) acc = fmaf(ph ? t.ku[1][j] : t.ku[0][j], sd[nl + j], acc);
    y[(size_t)b * Lout + tt] = acc;
  }
}

// transpose: dd[m] = sum_{p, j} ku[p][j] g[2(m - j + 7) + p] (0 <= m < M), dx[q] = sum_j kd[j] dd[m], 2m + j - 13 = q
__global__ __launch_bounds__(256) void ds_bwd_kernel(const float *__restrict__ g, float *__restrict__ dx, DsTaps t, int L,
                                                     int M, int Lout) {
  __shared__ float sg[DS_NG], sd[DS_ND];
  const int b = blockIdx.y, n0 = blockIdx.x * DS_NT, p0 = 2 * n0;
  const float *gb = g + (size_t)b * Lout;
  const int gbase = 2 * n0 - 28;
  for (int i = threadIdx.x; i < DS_NG; i += 256) {
    const int tt = gbase + i;
    sg[i] = (tt >= 0 && tt < Lout) ? gb[tt] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < DS_ND; i += 256) {
    const int m = n0 - 7 + i;
    float acc = 0.f;
    if (m >= 0 && m < M) {
#pragma unroll
      for (int j = 0; j < AP_DS_UP_TAPS; ++j) {
        acc = fmaf(t.ku[0][j], sg[2 * (i - j) + 28], acc);
        acc = fmaf(t.ku[1][j], sg[2 * (i - j) + 29], acc);
      }
    }
    sd[i] = acc;
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int ql = threadIdx.x + 256 * h, p = p0 + ql;
    if (p >= L) continue;
    float acc = 0.f;
    for (int i = (ql + 1) >> 1; i <= (ql + 27) >> 1; ++i) acc = fmaf(t.kd[ql + 27 - 2 * i], sd[i], acc);
    dx[(size_t)b * L + p] = acc;
  }
}

// ----------------------------------------------------------------------------------------------------------------- IIR
// The recurrence, the carried states and the zero-input basis are fp64: with poles near the unit circle (an order-2
// low-pass at 8 Hz has |p| = 0.998) an fp32 state loses ~7e-4 of max|y| even sequentially, and the scan's extra roundings
// about 5x that; fp64 state keeps every design within fp32 output rounding.  Input, output and y0 stay fp32.
struct IirCoef {
  double b[IIR_MAXCOEF], a[IIR_MAXCOEF];           // the fp32 design, normalised: a[0] == 1
  double AC[(IIR_MAXCOEF - 1) * (IIR_MAXCOEF - 1)];  // A^128, row-major [N][N]
};

// order-preserving map of a float to an unsigned key (for atomicMax)
__device__ __forceinline__ unsigned fkey(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float funkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// frequency_defense.py:75-80,114-120: [-1, 1] if 0.9 max(x) <= 1 and 0.9 min(x) >= -1 over the batch, else the int range
__device__ __forceinline__ void clip_range(const unsigned *mm, int bits, float &lo, float &hi) {
  const float mx = funkey(mm[0]), mn = -funkey(mm[1]);
  if (0.9f * mx <= 1.f && 0.9f * mn >= -1.f) {
    lo = -1.f; hi = 1.f;
  } else {
    hi = (float)((1 << (bits - 1)) - 1);
    lo = -(float)(1 << (bits - 1));
  }
}

// pass 1: zero-state response of every chunk (scan order; reversed in time when rev) and the chunk's end state.
// Forward: u = x, and the batch min/max is accumulated into mm.  Backward: u = g * 1[lo <= ypre <= hi] (ypre may be NULL).
template <int N>
__global__ __launch_bounds__(64) void iir_chunk_kernel(const float *__restrict__ u, const float *__restrict__ ypre,
                                                       unsigned *__restrict__ mm, int bits, float *__restrict__ y0,
                                                       double *__restrict__ st, IirCoef cf, int L, int nc, int rev,
                                                       int minmax) {
  __shared__ float s[IIR_CPB][IIR_CHUNK + 1];
  const int b = blockIdx.y, c0 = blockIdx.x * IIR_CPB;
  const size_t base = (size_t)b * L;
  const int n_base = c0 * IIR_CHUNK;
  float lo = 0.f, hi = 0.f;
  if (ypre) clip_range(mm, bits, lo, hi);
  float vmax = -INFINITY, vnmax = -INFINITY;
  for (int i = threadIdx.x; i < IIR_CPB * IIR_CHUNK; i += 64) {
    const int n = n_base + i;
    float v = 0.f;
    if (n < L) {
      const int o = rev ? L - 1 - n : n;
      v = u[base + o];
      if (minmax) { vmax = fmaxf(vmax, v); vnmax = fmaxf(vnmax, -v); }
      if (ypre) {
        const float yp = ypre[base + o];
        v = (yp >= lo && yp <= hi) ? v : 0.f;
      }
    }
    s[i / IIR_CHUNK][i % IIR_CHUNK] = v;
  }
  if (minmax) {
    for (int o = 32; o > 0; o >>= 1) {                      // (two max butterflies, interleaved: not a sum, left as it is)
      vmax = fmaxf(vmax, __shfl_xor(vmax, o));
      vnmax = fmaxf(vnmax, __shfl_xor(vnmax, o));
    }
    if (threadIdx.x == 0 && vmax > -INFINITY) {
      atomicMax(mm, fkey(vmax));
      atomicMax(mm + 1, fkey(vnmax));
    }
  }
  __syncthreads();
  const int c = c0 + threadIdx.x;
  if (c < nc) {
    double z[N];
#pragma unroll
    for (int i = 0; i < N; ++i) z[i] = 0.0;
    float *row = s[threadIdx.x];
    for (int k = 0; k < IIR_CHUNK; ++k) {
      const double xv = row[k];
      const double yv = fma(cf.b[0], xv, z[0]);
#pragma unroll
      for (int i = 0; i < N - 1; ++i) z[i] = fma(-cf.a[i + 1], yv, fma(cf.b[i + 1], xv, z[i + 1]));
      z[N - 1] = fma(-cf.a[N], yv, cf.b[N] * xv);
      row[k] = (float)yv;
    }
    double *e = st + ((size_t)b * nc + c) * N;
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = z[i];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < IIR_CPB * IIR_CHUNK; i += 64) {
    const int n = n_base + i;
    if (n < L) y0[base + n] = s[i / IIR_CHUNK][i % IIR_CHUNK];
  }
}

// pass 2: one thread per clip, in place: st[c] <- S_c (the state entering chunk c), S_0 = 0, S_{c+1} = A^128 S_c + e_c
template <int N>
__global__ __launch_bounds__(64) void iir_carry_kernel(double *__restrict__ st, IirCoef cf, int B, int nc) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double S[N];
#pragma unroll
  for (int i = 0; i < N; ++i) S[i] = 0.0;
  double *p = st + (size_t)b * nc * N;
  for (int c = 0; c < nc; ++c, p += N) {
    double e[N], T[N];
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = p[i];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double acc = e[i];
#pragma unroll
      for (int j = 0; j < N; ++j) acc = fma(cf.AC[i * N + j], S[j], acc);
      T[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) { p[i] = S[i]; S[i] = T[i]; }
  }
}

// pass 3: out[o(n)] = clamp(y0[n] + H[n % 128] . S_{n / 128}); ypre_out (forward) keeps the value before the clamp
template <int N>
__global__ __launch_bounds__(256) void iir_fix_kernel(const float *__restrict__ y0, const double *__restrict__ st,
                                                      const double *__restrict__ H, const unsigned *__restrict__ mm, int bits,
                                                      float *__restrict__ ypre_out, float *__restrict__ out, int L, int nc,
                                                      int rev) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= L) return;
  const int b = blockIdx.y, c = n / IIR_CHUNK, k = n % IIR_CHUNK;
  const size_t base = (size_t)b * L;
  const double *S = st + ((size_t)b * nc + c) * N;
  const double *h = H + k * N;
  double zi = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) zi = fma(h[i], S[i], zi);
  float v = (float)((double)y0[base + n] + zi);
  const int o = rev ? L - 1 - n : n;
  if (ypre_out) ypre_out[base + o] = v;
  if (mm) {
    float lo, hi;
    clip_range(mm, bits, lo, hi);
    v = fminf(fmaxf(v, lo), hi);
  }
  out[base + o] = v;
}

int iir_coef(const char *who, const float *b, const float *a, int ncoef, const double *AC, IirCoef &cf) {
  if (!b || !a || !AC) return bad("%s: NULL coefficient array", who);
  if (ncoef < 2 || ncoef > IIR_MAXCOEF)
    return bad("%s: %d filter coefficients; this build takes 2 .. %d (order 1 .. %d)", who, ncoef, IIR_MAXCOEF,
               IIR_MAXCOEF - 1);
  if (!(a[0] != 0.f) || !isfinite(a[0])) return bad("%s: a[0] must be finite and non-zero", who);
  memset(&cf, 0, sizeof(cf));
  for (int i = 0; i < ncoef; ++i) {
    cf.b[i] = (double)b[i] / (double)a[0];
    cf.a[i] = (double)a[i] / (double)a[0];
  }
  const int N = ncoef - 1;
  for (int i = 0; i < N * N; ++i) cf.AC[i] = AC[i];
  return 0;
}

template <int N>
int iir_run(const float *u, const float *ypre_mask, unsigned *mm, int bits, float *ypre_out, float *out, const IirCoef &cf,
            const double *H, float *scratch, int B, int L, int rev, int clamp, int minmax, hipStream_t s) {
  const int nc = (L + IIR_CHUNK - 1) / IIR_CHUNK;
  float *y0 = scratch;
  double *st = reinterpret_cast<double *>(scratch + (((size_t)B * L + 1) & ~(size_t)1));   // 8-byte aligned
  iir_chunk_kernel<N><<<dim3((nc + IIR_CPB - 1) / IIR_CPB, B), 64, 0, s>>>(u, ypre_mask, mm, bits, y0, st, cf, L, nc, rev,
                                                                            minmax);
  AP_HIP(hipGetLastError());
  iir_carry_kernel<N><<<(B + 63) / 64, 64, 0, s>>>(st, cf, B, nc);
  AP_HIP(hipGetLastError());
  iir_fix_kernel<N><<<dim3((L + 255) / 256, B), 256, 0, s>>>(y0, st, H, clamp ? mm : nullptr, bits, ypre_out, out, L, nc,
                                                              rev);
  AP_HIP(hipGetLastError());
  return 0;
}

int iir_dispatch(int N, const float *u, const float *ypre_mask, unsigned *mm, int bits, float *ypre_out, float *out,
                 const IirCoef &cf, const double *H, float *scratch, int B, int L, int rev, int clamp, int minmax,
                 hipStream_t s) {
  switch (N) {
#define AP_IIR_CASE(n) \
  case n: return iir_run<n>(u, ypre_mask, mm, bits, ypre_out, out, cf, H, scratch, B, L, rev, clamp, minmax, s);
    AP_IIR_CASE(1) AP_IIR_CASE(2) AP_IIR_CASE(3) AP_IIR_CASE(4) AP_IIR_CASE(5) AP_IIR_CASE(6) AP_IIR_CASE(7)
    AP_IIR_CASE(8) AP_IIR_CASE(9) AP_IIR_CASE(10) AP_IIR_CASE(11) AP_IIR_CASE(12) AP_IIR_CASE(13) AP_IIR_CASE(14)
    AP_IIR_CASE(15)
#undef AP_IIR_CASE
    default: return bad("iir: order %d out of range", N);
  }
}

int ds_taps(const char *who, const float *kd, const float *ku, DsTaps &t) {
  if (!kd || !ku) return bad("%s: NULL tap array", who);
  memcpy(t.kd, kd, sizeof(t.kd));
  memcpy(t.ku, ku, sizeof(t.ku));
  return 0;
}

}  // namespace
}  // namespace ap

using namespace ap;

extern "C" int ap_avg_smooth(const float *x, float *y, int k, int B, int L, void *stream) {
  if (int rc = check_bl("ap_avg_smooth", x, y, y, B, L)) return rc;
  if (k < 1 || (k & 1) == 0) return bad("ap_avg_smooth: window %d must be odd and >= 1 (time_defense.py:117)", k);
  const float w = (float)(1.0 / (double)k);
  avg_smooth_kernel<<<dim3((L + 255) / 256, B), 256, 0, (hipStream_t)stream>>>(x, y, (k - 1) / 2, w, L);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_median_smooth(const float *x, float *y, int8_t *argoff, int k, int B, int L, void *stream) {
  if (int rc = check_bl("ap_median_smooth", x, y, argoff, B, L)) return rc;
  if (k < 1 || (k & 1) == 0 || k > MS_MAX_WIN)
    return bad("ap_median_smooth: window %d must be odd and in [1, %d]", k, MS_MAX_WIN);
  median_smooth_kernel<<<dim3((L + 255) / 256, B), 256, 0, (hipStream_t)stream>>>(x, y, argoff, (k - 1) / 2, L);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_median_smooth_bwd(const float *g, const int8_t *argoff, float *dx, int k, int B, int L, void *stream) {
  if (int rc = check_bl("ap_median_smooth_bwd", g, argoff, dx, B, L)) return rc;
  if (k < 1 || (k & 1) == 0 || k > MS_MAX_WIN)
    return bad("ap_median_smooth_bwd: window %d must be odd and in [1, %d]", k, MS_MAX_WIN);
  median_smooth_bwd_kernel<<<dim3((L + 255) / 256, B), 256, 0, (hipStream_t)stream>>>(g, argoff, dx, (k - 1) / 2, L);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_at_fwd(const float *x, const float *z, float *y, float snr, int B, int L, void *stream) {
  if (int rc = check_bl("ap_at_fwd", x, z, y, B, L)) return rc;
  if (!(snr > 0.f) || !isfinite(snr)) return bad("ap_at_fwd: snr must be finite and > 0");
  at_fwd_kernel<<<B, 1024, 0, (hipStream_t)stream>>>(x, z, y, snr, L);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_at_bwd(const float *x, const float *z, const float *g, float *dx, float snr, int B, int L, void *stream) {
  if (int rc = check_bl("ap_at_bwd", x, z, g, B, L)) return rc;
  if (!dx) return bad("ap_at_bwd: NULL tensor argument");
  if (!(snr > 0.f) || !isfinite(snr)) return bad("ap_at_bwd: snr must be finite and > 0");
  at_bwd_kernel<<<B, 1024, 0, (hipStream_t)stream>>>(x, z, g, dx, snr, L);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_ds_fwd(const float *x, float *y, const float *kd, const float *ku, int B, int L, int Lout, void *stream) {
  if (int rc = check_bl("ap_ds_fwd", x, y, y, B, L)) return rc;
  const int M = (L + 1) / 2;
  if (Lout != L && Lout != 2 * M) return bad("ap_ds_fwd: Lout %d must be L (%d) or 2 ceil(L / 2) (%d)", Lout, L, 2 * M);
  DsTaps t;
  if (int rc = ds_taps("ap_ds_fwd", kd, ku, t)) return rc;
  ds_fwd_kernel<<<dim3((M + DS_NT - 1) / DS_NT, B), 256, 0, (hipStream_t)stream>>>(x, y, t, L, M, Lout);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_ds_bwd(const float *g, float *dx, const float *kd, const float *ku, int B, int L, int Lout, void *stream) {
  if (int rc = check_bl("ap_ds_bwd", g, dx, dx, B, L)) return rc;
  const int M = (L + 1) / 2;
  if (Lout != L && Lout != 2 * M) return bad("ap_ds_bwd: Lout %d must be L (%d) or 2 ceil(L / 2) (%d)", Lout, L, 2 * M);
  DsTaps t;
  if (int rc = ds_taps("ap_ds_bwd", kd, ku, t)) return rc;
  ds_bwd_kernel<<<dim3((M + DS_NT - 1) / DS_NT, B), 256, 0, (hipStream_t)stream>>>(g, dx, t, L, M, Lout);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" size_t ap_iir_scratch_elems(int ncoef, int B, int L) {
  if (ncoef < 2 || ncoef > IIR_MAXCOEF || B < 1 || L < 1) return 0;
  const size_t nc = ((size_t)L + IIR_CHUNK - 1) / IIR_CHUNK;
  return (((size_t)B * L + 1) & ~(size_t)1) + 2 * (size_t)B * nc * (ncoef - 1);   // y0 (fp32), then fp64 states
}

extern "C" int ap_iir_fwd(const float *x, float *y, float *ypre, unsigned *minmax, const float *b, const float *a, int ncoef,
                          const double *AC, const double *H, float *scratch, int bits, int B, int L, void *stream) {
  if (int rc = check_bl("ap_iir_fwd", x, y, H, B, L)) return rc;
  IirCoef cf;
  if (int rc = iir_coef("ap_iir_fwd", b, a, ncoef, AC, cf)) return rc;
  if (!scratch || !minmax) return bad("ap_iir_fwd: NULL scratch or minmax");
  if (bits < 2 || bits > 31) return bad("ap_iir_fwd: bits %d out of [2, 31]", bits);
  hipStream_t s = (hipStream_t)stream;
  AP_HIP(hipMemsetAsync(minmax, 0, 2 * sizeof(unsigned), s));    // key 0 sorts below every float
  return iir_dispatch(ncoef - 1, x, nullptr, minmax, bits, ypre, y, cf, H, scratch, B, L, 0, 1, 1, s);
}

extern "C" int ap_iir_bwd(const float *g, const float *ypre, const unsigned *minmax, float *dx, const float *b,
                          const float *a, int ncoef, const double *AC, const double *H, float *scratch, int bits, int B, int L,
                          void *stream) {
  if (int rc = check_bl("ap_iir_bwd", g, dx, H, B, L)) return rc;
  IirCoef cf;
  if (int rc = iir_coef("ap_iir_bwd", b, a, ncoef, AC, cf)) return rc;
  if (!scratch) return bad("ap_iir_bwd: NULL scratch");
  if (ypre && !minmax) return bad("ap_iir_bwd: ypre given without the forward's minmax");
  if (bits < 2 || bits > 31) return bad("ap_iir_bwd: bits %d out of [2, 31]", bits);
  return iir_dispatch(ncoef - 1, g, ypre, const_cast<unsigned *>(minmax), bits, nullptr, dx, cf, H, scratch, B, L, 1, 0, 0,
                      (hipStream_t)stream);
}
