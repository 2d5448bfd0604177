// 2048-point Stockham radix-2 FFT in LDS, shared by the mel front-end (ap_mel.hip, fp32) and the psychoacoustic
// masker (ap_psy.hip, fp32 for the perturbation's spectrum, fp64 for the masking threshold's).
#pragma once
#include <hip/hip_runtime.h>

namespace ap {

template <typename T> struct Cplx;
template <> struct Cplx<float> {
  typedef float2 type;
  static __device__ __forceinline__ float2 make(float re, float im) { return make_float2(re, im); }
};
template <> struct Cplx<double> {
  typedef double2 type;
  static __device__ __forceinline__ double2 make(double re, double im) { return make_double2(re, im); }
};

// forward 2048-point FFT (exponent sign -1) of bufA, all 256 threads of the workgroup; tw[m] = exp(-2 pi i m / 2048),
// m < 1024.  Returns the buffer holding the result (bufA or bufB; the other one is free afterwards).
template <typename T>
__device__ __forceinline__ typename Cplx<T>::type *fft2048_t(typename Cplx<T>::type *bufA, typename Cplx<T>::type *bufB,
                                                              const typename Cplx<T>::type *tw, int tid) {
  typedef typename Cplx<T>::type C;
  constexpr int N = 2048;
  C *src = bufA, *dst = bufB;
#pragma unroll 1
  for (int Ns = 1; Ns < N; Ns <<= 1) {
    const int tstride = (N / 2) / Ns;
    for (int jj = tid; jj < N / 2; jj += 256) {
      const int k = jj & (Ns - 1);
      const C w = tw[k * tstride];
      const C a = src[jj];
      const C c = src[jj + N / 2];
      const C bw = Cplx<T>::make(c.x * w.x - c.y * w.y, c.x * w.y + c.y * w.x);
      const int o = ((jj - k) << 1) + k;
      dst[o] = Cplx<T>::make(a.x + bw.x, a.y + bw.y);
      dst[o + Ns] = Cplx<T>::make(a.x - bw.x, a.y - bw.y);
    }
    __syncthreads();
    C *t = src; src = dst; dst = t;
  }
  return src;
}

__device__ __forceinline__ float2 *fft2048(float2 *bufA, float2 *bufB, const float2 *tw, int tid) {
  return fft2048_t<float>(bufA, bufB, tw, tid);
}

}  // namespace ap
