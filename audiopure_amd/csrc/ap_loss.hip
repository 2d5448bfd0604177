// The loss head of the classifiers' training loop for gfx950 (include/audiopure.h, "loss head"): what stands between model(inputs)
// and optimizer.step() in train_speech_commands.py:131-163 -- mixup of inputs and targets, CrossEntropyLoss / the mixup cross
// entropy / nll_loss with the seed of loss.backward(), the predictions and the count of correct ones.
//
// ap_class_loss is two launches.  The row kernel gives one wave to a row of K scores (lane l holds element l; past 64 the lanes
// stride): the lowest index of the maximum, then exp(z - max) summed over the wave, then the row's loss and its row of d loss / d in.
// The second kernel is one workgroup: it adds the B row losses in fp64, each lane a run of consecutive rows and lane 0 the 256
// runs, both in index order, and counts pred == labels.  No atomics, every sum has one order: two runs give equal bits.  Plain fp32
// (expf / logf, correctly rounded divide); nothing is allocated.
#include "ap_common.h"

namespace ap {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_WAVE = 64;
constexpr int LOSS_ROWS = LOSS_THREADS / LOSS_WAVE;       // rows per workgroup
constexpr int LOSS_MAX_K = 4096;
constexpr int LOSS_MAX_B = 65535;

template <int MODE>
__global__ __launch_bounds__(LOSS_THREADS) void class_loss_rows_kernel(const float *__restrict__ in, const int64_t *__restrict__ labels,
                                                                      const float *__restrict__ soft, float *__restrict__ loss_rows,
                                                                      float *__restrict__ din, int64_t *__restrict__ pred, int B, int K) {
  const int lane = threadIdx.x & (LOSS_WAVE - 1);
  const int b = blockIdx.x * LOSS_ROWS + (threadIdx.x >> 6);
  if (b >= B) return;                                    // (whole waves leave: no shuffle below misses a partner)
  const float *z = in + (size_t)b * K;
  const float z0 = lane < K ? z[lane] : 0.f;             // K <= 64: the row lives in registers
  auto at = [&](int i) { return i == lane ? z0 : z[i]; };

  // lowest index of the row maximum
  float mv = -INFINITY;
  int mi = 0x7fffffff;
  for (int i = lane; i < K; i += LOSS_WAVE) {
    const float v = at(i);
    if (mi == 0x7fffffff || v > mv) { mv = v; mi = i; }
  }
#pragma unroll
  for (int o = LOSS_WAVE / 2; o > 0; o >>= 1) {            // (not wave_sum: an index travels with the maximum, with a tie rule)
    const float ov = __shfl_xor(mv, o, LOSS_WAVE);
    const int oi = __shfl_xor(mi, o, LOSS_WAVE);
    if (oi != 0x7fffffff && (mi == 0x7fffffff || ov > mv || (ov == mv && oi < mi))) { mv = ov; mi = oi; }
  }
  if (pred && lane == 0) pred[b] = mi;

  const float invB = 1.f / (float)B;
  float *d = din ? din + (size_t)b * K : nullptr;
  int64_t y = 0;
  bool y_ok = true;
  if (MODE != 1) {
    y = labels[b];
    y_ok = y >= 0 && y < K;
  }
  if (MODE == 2) {                                       // F.nll_loss on log-probabilities
    if (lane == 0) loss_rows[b] = y_ok ? -z[y] : NAN;
    if (d)
      for (int i = lane; i < K; i += LOSS_WAVE) d[i] = y_ok ? (i == y ? -invB : 0.f) : NAN;
    return;
  }
  float s = 0.f;
  for (int i = lane; i < K; i += LOSS_WAVE) s += expf(at(i) - mv);
  s = wave_sum(s);
  if (MODE == 0) {                                       // nn.CrossEntropyLoss(): logsumexp(z) - z[y]
    if (lane == 0) loss_rows[b] = y_ok ? (mv - z[y]) + logf(s) : NAN;
    if (d)
      for (int i = lane; i < K; i += LOSS_WAVE) {
        const float p = expf(at(i) - mv) / s;
        d[i] = y_ok ? (p - (i == y ? 1.f : 0.f)) * invB : NAN;
      }
    return;
  }
  // mixup_cross_entropy_loss: -sum_i q_i log(clamp(p_i, 1e-5, 1)); the clamp passes a gradient where 1e-5 <= p_i <= 1
  const float *q = soft + (size_t)b * K;
  float l = 0.f, qm = 0.f;
  for (int i = lane; i < K; i += LOSS_WAVE) {
    const float p = expf(at(i) - mv) / s;
    const float c = fminf(fmaxf(p, 1e-5f), 1.f);
    const float qi = q[i];
    l += qi * logf(c);
    if (p >= 1e-5f && p <= 1.f) qm += qi;
  }
  l = wave_sum(l);
  qm = wave_sum(qm);
  if (lane == 0) loss_rows[b] = -l;
  if (d)
    for (int i = lane; i < K; i += LOSS_WAVE) {
      const float p = expf(at(i) - mv) / s;
      const float live = (p >= 1e-5f && p <= 1.f) ? q[i] : 0.f;
      d[i] = (p * qm - live) * invB;
    }
}

// one workgroup: loss[0] = fp32(sum_b loss_rows[b] / B) with the sum in fp64 in index order, n_correct[0] = #{pred[b] == labels[b]}
__global__ __launch_bounds__(LOSS_THREADS) void class_loss_final_kernel(const float *__restrict__ loss_rows, float *__restrict__ loss,
                                                                       const int64_t *__restrict__ pred, const int64_t *__restrict__ labels,
                                                                       int64_t *__restrict__ n_correct, int B) {
  __shared__ double part[LOSS_THREADS];
  __shared__ int hits[LOSS_THREADS];
  const int run = (B + LOSS_THREADS - 1) / LOSS_THREADS;
  const int lo = (int)threadIdx.x * run, hi = lo + run < B ? lo + run : B;
  double s = 0.0;
  int c = 0;
  for (int b = lo; b < hi; b++) {
    s += (double)loss_rows[b];
    if (n_correct) c += pred[b] == labels[b] ? 1 : 0;
  }
  part[threadIdx.x] = s;
  hits[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    int n = 0;
    for (int i = 0; i < LOSS_THREADS; i++) { t += part[i]; n += hits[i]; }
    loss[0] = (float)(t / (double)B);
    if (n_correct) n_correct[0] = n;
  }
}

// torch's `weight * x1 + (1 - weight) * x2` in fp32: 1 - w rounded, two rounded products, a rounded sum -- never an fma
__device__ __forceinline__ float mix(float w, float omw, float a, float c) { return __fadd_rn(__fmul_rn(w, a), __fmul_rn(omw, c)); }

__global__ __launch_bounds__(LOSS_THREADS) void mixup_rows_kernel(const float *__restrict__ x, const int64_t *__restrict__ index,
                                                                 const float *__restrict__ weight, float *__restrict__ out, int B, int n) {
  const int b = blockIdx.y;
  const int64_t j = index[b];
  const bool ok = j >= 0 && j < B;
  const float w = weight[b], omw = __fsub_rn(1.f, w);
  const float *x1 = x + (size_t)b * n, *x2 = x + (size_t)(ok ? j : 0) * n;
  float *o = out + (size_t)b * n;
  for (size_t i = (size_t)blockIdx.x * LOSS_THREADS + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * LOSS_THREADS)
    o[i] = ok ? mix(w, omw, x1[i], x2[i]) : NAN;
}

__global__ __launch_bounds__(LOSS_THREADS) void mixup_targets_kernel(const int64_t *__restrict__ labels, const int64_t *__restrict__ index,
                                                                    const float *__restrict__ weight, float *__restrict__ out, int B, int K) {
  const int b = blockIdx.x;
  const int64_t j = index[b];
  const bool j_ok = j >= 0 && j < B;
  const int64_t y1 = labels[b], y2 = j_ok ? labels[j] : -1;
  const bool ok = j_ok && y1 >= 0 && y1 < K && y2 >= 0 && y2 < K;
  const float w = weight[b], omw = __fsub_rn(1.f, w);
  float *o = out + (size_t)b * K;
  for (int k = threadIdx.x; k < K; k += LOSS_THREADS) o[k] = ok ? mix(w, omw, k == y1 ? 1.f : 0.f, k == y2 ? 1.f : 0.f) : NAN;
}

// out[i] = x[i] (g[0] factor): the cotangent of a scalar loss, read on the device
__global__ __launch_bounds__(LOSS_THREADS) void scale_by_scalar_kernel(const float *x, const float *g, float factor, float *out, size_t n) {
  const float s = g ? __fmul_rn(g[0], factor) : factor;
  for (size_t i = (size_t)blockIdx.x * LOSS_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * LOSS_THREADS) out[i] = x[i] * s;
}

static bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

static unsigned stream_blocks(size_t n) {
  const size_t want = (n + LOSS_THREADS - 1) / LOSS_THREADS;
  return (unsigned)(want < 1 ? 1 : want > 4096 ? 4096 : want);
}

}  // namespace ap

using namespace ap;

extern "C" {

int ap_class_loss(const float *in, const int64_t *labels, const float *soft, int mode, float *loss_rows, float *loss, float *din,
                  int64_t *pred, int64_t *n_correct, int B, int K, void *stream) {
  if (!in || !loss_rows || !loss) { set_error("ap_class_loss: null in, loss_rows or loss"); return -22; }
  if (mode < 0 || mode > 2) { set_error("ap_class_loss: mode %d is none of 0 (cross entropy), 1 (mixup cross entropy), 2 (nll)", mode); return -22; }
  if (K < 1 || K > LOSS_MAX_K) { set_error("ap_class_loss: K = %d outside [1, %d]", K, LOSS_MAX_K); return -22; }
  if (B < 1 || B > LOSS_MAX_B) { set_error("ap_class_loss: B = %d outside [1, %d]", B, LOSS_MAX_B); return -22; }
  if (mode != 1 && !labels) { set_error("ap_class_loss: mode %d needs labels", mode); return -22; }
  if (mode == 1 && !soft) { set_error("ap_class_loss: mode 1 needs the soft targets"); return -22; }
  if (n_correct && (!labels || !pred)) { set_error("ap_class_loss: n_correct needs labels and pred"); return -22; }
  const size_t bytes = (size_t)B * K * sizeof(float);
  if (din && (overlap(din, bytes, in, bytes) || (soft && overlap(din, bytes, soft, bytes)))) {
    set_error("ap_class_loss: din overlaps in or soft");
    return -22;
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((B + LOSS_ROWS - 1) / LOSS_ROWS)), block(LOSS_THREADS);
  if (mode == 0) class_loss_rows_kernel<0><<<grid, block, 0, st>>>(in, labels, soft, loss_rows, din, pred, B, K);
  else if (mode == 1) class_loss_rows_kernel<1><<<grid, block, 0, st>>>(in, labels, soft, loss_rows, din, pred, B, K);
  else class_loss_rows_kernel<2><<<grid, block, 0, st>>>(in, labels, soft, loss_rows, din, pred, B, K);
  AP_HIP(hipGetLastError());
  class_loss_final_kernel<<<1, block, 0, st>>>(loss_rows, loss, pred, labels, n_correct, B);
  AP_HIP(hipGetLastError());
  return 0;
}

int ap_mixup_rows(const float *x, const int64_t *index, const float *weight, float *out, int B, int n, void *stream) {
  if (!x || !index || !weight || !out) { set_error("ap_mixup_rows: null argument"); return -22; }
  if (B < 1 || B > LOSS_MAX_B || n < 1) { set_error("ap_mixup_rows: B = %d outside [1, %d] or n = %d < 1", B, LOSS_MAX_B, n); return -22; }
  const size_t bytes = (size_t)B * n * sizeof(float);
  if (overlap(x, bytes, out, bytes)) { set_error("ap_mixup_rows: out overlaps x (a row is read after another was written)"); return -22; }
  mixup_rows_kernel<<<dim3(stream_blocks((size_t)n), (unsigned)B), dim3(LOSS_THREADS), 0, (hipStream_t)stream>>>(x, index, weight, out, B, n);
  AP_HIP(hipGetLastError());
  return 0;
}

int ap_mixup_targets(const int64_t *labels, const int64_t *index, const float *weight, float *out, int B, int K, void *stream) {
  if (!labels || !index || !weight || !out) { set_error("ap_mixup_targets: null argument"); return -22; }
  if (B < 1 || B > LOSS_MAX_B || K < 1 || K > LOSS_MAX_K) {
    set_error("ap_mixup_targets: B = %d outside [1, %d] or K = %d outside [1, %d]", B, LOSS_MAX_B, K, LOSS_MAX_K);
    return -22;
  }
  mixup_targets_kernel<<<dim3((unsigned)B), dim3(LOSS_THREADS), 0, (hipStream_t)stream>>>(labels, index, weight, out, B, K);
  AP_HIP(hipGetLastError());
  return 0;
}

int ap_scale_by_scalar(const float *x, const float *g, float factor, float *out, size_t n, void *stream) {
  if (!x || !out) { set_error("ap_scale_by_scalar: null x or out"); return -22; }
  if (n == 0) return 0;
  scale_by_scalar_kernel<<<dim3(stream_blocks(n)), dim3(LOSS_THREADS), 0, (hipStream_t)stream>>>(x, g, factor, out, n);
  AP_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
