// Psychoacoustic masking threshold and the imperceptibility hinge loss of the second, "imperceptible" stage of the white-box
// attack (Qin et al. 2019; robustness_eval/white_box_attack.py:36-273 PsychoacousticMasker, :610-710 the loss, its gradient
// and the stabilised thresholds).  Window 2048 (periodic Hann), hop H, center=False: F = 1 + (L - 2048) / H frames, 1025
// bins.  Every kernel runs one workgroup of 256 threads per (frame, clip); nothing is atomic and every reduction has a fixed
// order, so a clip's outputs do not depend on the batch it runs in.
//
// Arithmetic follows the reference step by step: its spectrum is a float64 FFT rounded to complex64, the
// PSD and the maskers are fp32, the individual and global thresholds fp64, rounded to an fp32 threshold array.  Separate
// roundings matter where a decision compares two values, so nothing in this file is contracted into an fma.
#include <math.h>

#include "ap_common.h"
#include "ap_fft.h"

#pragma clang fp contract(off)

namespace ap {
namespace psy {

constexpr int N = 2048, NB = N / 2 + 1, MAXM = 512;   // local maxima are never adjacent: at most 512 among bins 1 .. 1023
constexpr int T_WIN = 0, T_BARK = N, T_ATH = N + NB;  // offsets in the fp64 table (AP_PSY_TABLE_ELEMS)
constexpr float GAIN = 1.632993161855452f;            // sqrt(8 / 3) as the reference's fp32 product sees it

// |sqrt(8/3) X / N| in dB, floored at -200 (:162-176): X rounded to complex64, products and the hypot as numpy's fp32
// (hypotf is the double-precision sqrt of the exact sum of squares, rounded once).
__device__ __forceinline__ float psd_db(double xr, double xi) {
  const float a = ((float)xr * GAIN) / (float)N, b = ((float)xi * GAIN) / (float)N;
  const float mag = (float)sqrt((double)a * (double)a + (double)b * (double)b);
  const float p = 20.0f * (float)log10((double)mag);
  return fmaxf(p, -200.0f);                      // log10(0) = -inf -> -200, as clip(min=-200)
}

// PSD of one frame in dB [B][F][NB] and its maximum [B][F].  fp64 FFT: 2 x 32 KB data + 16 KB twiddles of LDS.
__global__ __launch_bounds__(256) void psy_psd_kernel(const float *__restrict__ x, const double *__restrict__ tab,
                                                      float *__restrict__ psd, float *__restrict__ fmax_out, int F, int L,
                                                      int hop) {
  __shared__ double2 bufA[N];
  __shared__ double2 bufB[N];
  __shared__ double2 tw[N / 2];
  __shared__ float red[256];
  const int tid = threadIdx.x, f = blockIdx.x, b = blockIdx.y;
  for (int m = tid; m < N / 2; m += 256) {
    double s, c;
    sincospi((double)m / 1024.0, &s, &c);
    tw[m] = make_double2(c, -s);
  }
  const float *xf = x + (size_t)b * L + (size_t)f * hop;       // (F - 1) hop + N <= L
  for (int n = tid; n < N; n += 256) bufA[n] = make_double2(tab[T_WIN + n] * (double)xf[n], 0.0);
  __syncthreads();
  const double2 *X = fft2048_t<double>(bufA, bufB, tw, tid);
  float *out = psd + ((size_t)b * F + f) * NB;
  float mx = -INFINITY;
  for (int k = tid; k < NB; k += 256) {
    const float p = psd_db(X[k].x, X[k].y);
    out[k] = p;
    mx = fmaxf(mx, p);
  }
  mx = block_tree<256>(mx, red, MaxOp{});
  __syncthreads();
  if (tid == 0) fmax_out[(size_t)b * F + f] = mx;
}

// Maskers, filters and the global threshold of one frame (:185-273, :699-705).
__global__ __launch_bounds__(256) void psy_threshold_kernel(const float *__restrict__ psd, const float *__restrict__ fmax_in,
                                                            const double *__restrict__ tab, float *__restrict__ thr_stab,
                                                            float *__restrict__ thr_db, float *__restrict__ pmax_stab,
                                                            float *__restrict__ pmax_db, int F) {
  __shared__ float p[NB];
  __shared__ double bark[NB];
  __shared__ int cnt[256];
  __shared__ int midx[MAXM];
  __shared__ float mval[MAXM];
  __shared__ unsigned char keep[MAXM];
  __shared__ int n_kept;
  const int tid = threadIdx.x, f = blockIdx.x, b = blockIdx.y;
  // 1. the clip's maximum over all bins and frames (fixed order), normalisation at 96 dB (:179-180)
  float mx = -INFINITY;
  for (int g = 0; g < F; g++) mx = fmaxf(mx, fmax_in[(size_t)b * F + g]);
  const float shift = 96.0f - mx;
  const float *in = psd + ((size_t)b * F + f) * NB;
  for (int k = tid; k < NB; k += 256) {
    p[k] = shift + in[k];
    bark[k] = tab[T_BARK + k];
  }
  __syncthreads();
  // 2. strict local maxima (argrelmax, mode 'clip': never bin 0 or 1024), smoothed with both neighbours in fp32 in the
  //    reference's order, kept if above the ATH (fp64 compare); compacted in bin order by a prefix sum.  Bins 4t .. 4t+3.
  float mv[4];
  int nmine = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int k = 4 * tid + i;
    mv[i] = NAN;
    if (k >= 1 && k <= NB - 2 && p[k] > p[k - 1] && p[k] > p[k + 1]) {
      const float e0 = (float)pow(10.0, (double)(p[k - 1] / 10.0f));
      const float e1 = (float)pow(10.0, (double)(p[k] / 10.0f));
      const float e2 = (float)pow(10.0, (double)(p[k + 1] / 10.0f));
      const float m = 10.0f * (float)log10((double)((e0 + e1) + e2));
      if ((double)m > tab[T_ATH + k]) {
        mv[i] = m;
        nmine++;
      }
    }
  }
  cnt[tid] = nmine;
  __syncthreads();
  for (int s = 1; s < 256; s <<= 1) {                          // inclusive Hillis-Steele scan
    const int v = tid >= s ? cnt[tid - s] : 0;
    __syncthreads();
    cnt[tid] += v;
    __syncthreads();
  }
  const int M = cnt[255];
  int o = cnt[tid] - nmine;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (!isnan(mv[i])) {
      midx[o] = 4 * tid + i;
      mval[o] = mv[i];
      o++;
    }
  }
  __syncthreads();
  // 3. bark-distance pass (:220-229) as written: it indexes the bark table by POSITION in the masker list, and deleting
  //    the earlier masker advances i_prev by one.  Sequential, at most 511 steps, then a sequential compaction.
  if (tid == 0) {
    for (int i = 0; i < M; i++) keep[i] = 1;
    int ip = 0;
    for (int i = 1; i < M; i++) {
      if (bark[i] - bark[ip] < 0.5) {
        if (mval[ip] < mval[i]) {
          keep[ip] = 0;
          ip = ip + 1;
        } else {
          keep[i] = 0;
        }
      } else {
        ip = i;
      }
    }
    int K = 0;
    for (int i = 0; i < M; i++) {
      if (keep[i]) {
        midx[K] = midx[i];
        mval[K] = mval[i];
        K++;
      }
    }
    n_kept = K;
  }
  __syncthreads();
  const int K = n_kept;
  // 4. individual thresholds and their fp64 power sum with the ATH (:235-273), one thread per bin, maskers in list order
  for (int k = tid; k < NB; k += 256) {
    const double z = bark[k];
    double s = 0.0;
    for (int j = 0; j < K; j++) {
      const int kj = midx[j];
      const float m = mval[j];
      const double dz = z - bark[kj];
      double spread;
      if (dz > 0.0) {
        const float slope = -27.0f + 0.37f * fmaxf(m - 40.0f, 0.0f);
        spread = (double)slope * dz;
      } else {
        spread = 27.0 * dz;
      }
      const double t = ((double)m + (-6.025 - 0.275 * bark[kj])) + spread;
      s = s + pow(10.0, t / 10.0);
    }
    s = s + pow(10.0, tab[T_ATH + k] / 10.0);
    const float th = (float)(10.0 * log10(s));                 // stored into the fp32 threshold array; -inf if s == 0
    const size_t oi = ((size_t)b * NB + k) * F + f;
    thr_stab[oi] = (float)pow(10.0, (double)(th * 0.1f));     // 10 ** (threshold * 0.1) in fp32; -inf -> 0
    if (thr_db) thr_db[oi] = th;
  }
  if (f == 0 && tid == 0) {
    pmax_stab[b] = (float)pow(10.0, (double)(mx * 0.1f));
    if (pmax_db) pmax_db[b] = mx;
  }
}

// Hinge loss of one frame of the perturbation and its gradient back to the frame's samples (:640-690):
//   P = 10^9.6 / psd_max_stab |sqrt(8/3) X / N|^2,  loss = mean relu(P - theta),
//   dloss/dX[k] = 1[P > theta] 2 c (g / N)^2 X[k] / (NB F),  c = 10^9.6 / psd_max_stab,
//   dseg[n] = w[n] Re sum_k G[k] e^{+2 pi i k n / N} = w[n] Re FFT(conj(G))[n]   (as melspec_bwd_kernel).
// Writes the windowed frame gradient to scratch [B][F][N] and the frame's hinge sum to part [B][F].
__global__ __launch_bounds__(256) void psy_loss_grad_kernel(const float *__restrict__ delta, const float *__restrict__ thr_stab,
                                                            const float *__restrict__ pmax_stab, float *__restrict__ scratch,
                                                            float *__restrict__ part, int F, int L, int hop) {
  __shared__ float2 bufA[N];
  __shared__ float2 bufB[N];
  __shared__ float2 tw[N / 2];
  __shared__ float red[256];
  const int tid = threadIdx.x, f = blockIdx.x, b = blockIdx.y;
  for (int m = tid; m < N / 2; m += 256) {
    float s, c;
    sincospif((float)m * (1.0f / 1024.0f), &s, &c);
    tw[m] = make_float2(c, -s);
  }
  const float *xf = delta + (size_t)b * L + (size_t)f * hop;
  for (int n = tid; n < N; n += 256) {
    const float w = 0.5f - 0.5f * cospif((float)n * (1.0f / 1024.0f));   // torch.hann_window(2048), periodic
    bufA[n] = make_float2(xf[n] * w, 0.f);
  }
  __syncthreads();
  float2 *X = fft2048(bufA, bufB, tw, tid);
  float2 *other = (X == bufA) ? bufB : bufA;
  const float c = (1.0f / pmax_stab[b]) * 3981071705.534972f;   // 10^9.6 / psd_max_stab as torch forms it (reciprocal, product)
  const float gs = 2.0f * c * (GAIN / (float)N) * (GAIN / (float)N) / ((float)NB * (float)F);
  float acc = 0.f;
  for (int k = tid; k < N; k += 256) {
    float2 v = make_float2(0.f, 0.f);
    if (k < NB) {
      const float2 xk = X[k];
      const float a = (GAIN * xk.x) / (float)N, bb = (GAIN * xk.y) / (float)N;
      const float r = sqrtf(a * a + bb * bb);
      const float d = c * (r * r) - thr_stab[((size_t)b * NB + k) * F + f];
      if (d > 0.f) {                                             // relu'(0) = 0
        acc += d;
        v = make_float2(gs * xk.x, -gs * xk.y);                  // conj(G[k])
      }
    }
    other[k] = v;
  }
  acc = block_tree<256>(acc, red, SumOp{});
  if (tid == 0) part[(size_t)b * F + f] = acc;
  float2 *R = fft2048(other, X, tw, tid);                       // X's storage is the scratch buffer now
  float *sc = scratch + ((size_t)b * F + f) * N;
  for (int n = tid; n < N; n += 256) {
    const float w = 0.5f - 0.5f * cospif((float)n * (1.0f / 1024.0f));
    sc[n] = R[n].x * w;
  }
}

// grad[b][t] = sum of the frames f < F with f H <= t < f H + N (increasing f); 0 past the last frame.  The first workgroup
// of each clip also forms loss[b] = (sum_f part[b][f]) / (NB F), summed in fp64 in frame order.
__global__ __launch_bounds__(256) void psy_grad_gather_kernel(const float *__restrict__ scratch, const float *__restrict__ part,
                                                              float *__restrict__ grad, float *__restrict__ loss, int F, int L,
                                                              int hop) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double s = 0.0;
    for (int g = 0; g < F; g++) s += (double)part[(size_t)b * F + g];
    loss[b] = (float)(s / ((double)NB * (double)F));
  }
  if (t >= L) return;
  const int fhi = min(F - 1, t / hop);
  const int flo = t >= N ? (t - N) / hop + 1 : 0;
  float s = 0.f;
  for (int g = flo; g <= fhi; g++) s += scratch[((size_t)b * F + g) * N + (t - g * hop)];
  grad[(size_t)b * L + t] = s;
}

static bool shape_ok(const char *who, int window, int hop, int B, int L) {
  if (window != N) { set_error("%s: window_size %d (only %d has a kernel)", who, window, N); return false; }
  if (hop < 1 || hop > N) { set_error("%s: hop %d outside [1, %d]", who, hop, N); return false; }
  if (B < 1 || L < N) { set_error("%s: B = %d, L = %d (needs B >= 1, L >= %d)", who, B, L, N); return false; }
  return true;
}

}  // namespace psy
}  // namespace ap

extern "C" size_t ap_psy_scratch_elems(int window, int hop, int B, int L) {
  using namespace ap::psy;
  if (window != N || hop < 1 || B < 1 || L < N) return 0;
  const size_t F = 1 + (size_t)(L - N) / hop;
  return (size_t)B * F * (N + 1);
}

extern "C" int ap_psy_threshold(const float *x, const double *tables, float *thr_stab, float *thr_db, float *psd_max_stab,
                                float *psd_max_db, float *scratch, int window, int hop, int B, int L, void *stream) {
  using namespace ap;
  using namespace ap::psy;
  if (!x || !tables || !thr_stab || !psd_max_stab || !scratch) { set_error("ap_psy_threshold: bad argument"); return -22; }
  if (!shape_ok("ap_psy_threshold", window, hop, B, L)) return -22;
  const int F = 1 + (L - N) / hop;
  float *psd = scratch, *fmx = scratch + (size_t)B * F * NB;
  hipStream_t st = (hipStream_t)stream;
  psy_psd_kernel<<<dim3(F, B), 256, 0, st>>>(x, tables, psd, fmx, F, L, hop);
  psy_threshold_kernel<<<dim3(F, B), 256, 0, st>>>(psd, fmx, tables, thr_stab, thr_db, psd_max_stab, psd_max_db, F);
  AP_HIP(hipGetLastError());
  return 0;
}

extern "C" int ap_psy_loss_grad(const float *delta, const float *thr_stab, const float *psd_max_stab, float *grad, float *loss,
                                float *scratch, int window, int hop, int B, int L, void *stream) {
  using namespace ap;
  using namespace ap::psy;
  if (!delta || !thr_stab || !psd_max_stab || !grad || !loss || !scratch) { set_error("ap_psy_loss_grad: bad argument"); return -22; }
  if (!shape_ok("ap_psy_loss_grad", window, hop, B, L)) return -22;
  const int F = 1 + (L - N) / hop;
  float *sc = scratch, *part = scratch + (size_t)B * F * N;
  hipStream_t st = (hipStream_t)stream;
  psy_loss_grad_kernel<<<dim3(F, B), 256, 0, st>>>(delta, thr_stab, psd_max_stab, sc, part, F, L, hop);
  psy_grad_gather_kernel<<<dim3((L + 255) / 256, B), 256, 0, st>>>(sc, part, grad, loss, F, L, hop);
  AP_HIP(hipGetLastError());
  return 0;
}
