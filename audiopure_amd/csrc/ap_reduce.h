// The fixed-order sums of the non-block kernels (training steps, attacks, defenses, optimizer, losses, front-ends), once.  These
// kernels use no floating-point atomics: the order of a sum is part of its result, and tests pin the bits.  Four orders exist, and a
// kernel picks one by calling it here ("Fixed-order sums"):
//   wave_sum         64-lane xor butterfly, offsets 32 .. 1
//   block_tree       LDS halving tree over the workgroup, widths NT/2 .. 1
//   block_wave_sum2  per wave a shuffle-down sum, then the four waves in wave order
//   slice_sum_kernel<T, SLICES> partial results of `slices` workgroups, in slice order, in fp64, rounded once
// Device-only; included by ap_device.h.
#pragma once

namespace ap {

// the operations, as "fold b into a"
struct SumOp {
  template <typename T> __device__ __forceinline__ void operator()(T &a, T b) const { a += b; }
};
struct MaxOp {
  __device__ __forceinline__ void operator()(float &a, float b) const { a = fmaxf(a, b); }
};

// sum over the W lanes of a group (xor butterfly, offsets W/2 .. 1): every lane gets the total, with the same bits (a + b == b + a)
template <int W = 64, typename T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// op over the NT threads of the workgroup through red[NT]; every thread returns it.  No trailing barrier: a caller that writes red
// again synchronises first.
template <int NT, typename T, typename Op>
__device__ __forceinline__ T block_tree(T v, T *red, Op op) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) op(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  return red[0];
}
// two values at once through red[2 NT], one tree each (a's in red[0 .. NT), b's behind it), the barriers shared
template <int NT, typename T, typename Op>
__device__ __forceinline__ void block_tree2(T &a, T &b, T *red, Op op) {
  red[threadIdx.x] = a;
  red[NT + threadIdx.x] = b;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      op(red[threadIdx.x], red[threadIdx.x + w]);
      op(red[NT + threadIdx.x], red[NT + threadIdx.x + w]);
    }
    __syncthreads();
  }
  a = red[0];
  b = red[NT];
}

// sum of (a, b) over the 256 threads of the block: wave shuffles, then the four waves in order; valid in thread 0
__device__ __forceinline__ void block_wave_sum2(double &a, double &b) {
  __shared__ double sm[8];
  for (int d = 32; d; d >>= 1) {
    a += __shfl_down(a, d, 64);
    b += __shfl_down(b, d, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sm[2 * w] = a; sm[2 * w + 1] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = sm[0]; b = sm[1];
    for (int i = 1; i < 4; i++) { a += sm[2 * i]; b += sm[2 * i + 1]; }
  }
}

// out[e] (+)= scale * (slice 0 + slice 1 + ...) of part[slice][e * stride]: in slice order, in fp64, rounded once (the slices' own
// sums were rounded where they were formed; their sum is not rounded again per slice).  T = double with stride 2 reads the first of
// each pair.  256 threads per workgroup.
// (This and the two finalisers below are __global__ templates in a header: several translation units instantiate the same mangled
// name, the weak host stubs merge at link time and the runtime launches the first module registered for the stub.  Sound only
// while every translation unit that instantiates them is compiled with the same flags, as build_hip does for the files that do.)
// The slice count is either a constant of the caller, given as SLICES (M5, KWS: the loop unrolls and every slice's load is in
// flight at once; such a caller passes 0 for `slices`, which is not read), or, with SLICES = 0, the `slices` argument.
template <typename T, int SLICES = 0>
__global__ __launch_bounds__(256) void slice_sum_kernel(const T *__restrict__ part, float *__restrict__ out, size_t total, int slices,
                                                        int stride, float scale, int accumulate) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  double s = 0.0;
  const int ns = SLICES ? SLICES : slices;
  for (int z = 0; z < ns; z++) s += (double)part[((size_t)z * total + e) * stride];
  const float v = (float)(s * (double)scale);
  out[e] = accumulate ? out[e] + v : v;
}

// BatchNorm with batch statistics, the step after the per-slice sums part[slice][c] = (sum x, sum x^2) over n values per channel:
// stat = [mean[C]; 1 / sqrt(biased var + eps)[C]]; running = (1 - m) old + m batch, the variance UNBIASED, n / (n - 1).  The variance
// comes from fp64 sums of fp32 values, so sum x^2 - n mean^2 cancels nothing an fp32 result can see.  rm_in / rv_in may be rm / rv.
template <int SLICES>
__global__ void bn_stats_final_kernel(const double *__restrict__ part, const float *rm_in, const float *rv_in,
                                      float *__restrict__ stat, float *rm, float *rv, int C, double n, float eps, float momentum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int sl = 0; sl < SLICES; sl++) {
    s1 += part[((size_t)sl * C + c) * 2];
    s2 += part[((size_t)sl * C + c) * 2 + 1];
  }
  const double mu = s1 / n;
  double var = s2 / n - mu * mu;
  if (var < 0.0) var = 0.0;
  stat[c] = (float)mu;
  stat[C + c] = (float)(1.0 / sqrt(var + (double)eps));
  const double m = (double)momentum;
  rm[c] = (float)((1.0 - m) * (double)rm_in[c] + m * mu);
  rv[c] = (float)((1.0 - m) * (double)rv_in[c] + m * var * (n / (n - 1.0)));
}

// ... and of the backward, part[slice][c] = (sum dy, sum dy xhat): d beta, d gamma (either may be null) and mean2[c] = their means
template <int SLICES>
__global__ void bn_bstats_final_kernel(const double *__restrict__ part, double *__restrict__ mean2,
                                       float *__restrict__ dgamma, float *__restrict__ dbeta, int C, double n) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int sl = 0; sl < SLICES; sl++) {
    s1 += part[((size_t)sl * C + c) * 2];
    s2 += part[((size_t)sl * C + c) * 2 + 1];
  }
  if (dbeta) dbeta[c] = (float)s1;
  if (dgamma) dgamma[c] = (float)s2;
  mean2[2 * c] = s1 / n;
  mean2[2 * c + 1] = s2 / n;
}

}  // namespace ap
