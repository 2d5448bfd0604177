// Multi-tensor optimizer step for gfx950: Adam, AdamW, SGD, the exponential moving average of the parameters in the same pass, and
// the squared gradient norm (include/audiopure.h, "optimizer step").  One streaming kernel family over a table of tensors.
//
// The table rides in the kernel arguments, OPT_SLAB descriptors per launch (as many as the 4 KB argument block holds), so a step is
// ceil(tensors / OPT_SLAB) launches and nothing else: no host-to-device copy, no allocation, no synchronise.  A workgroup owns one
// chunk of OPT_CHUNK elements of one tensor and finds the tensor by bisecting the per-descriptor chunk prefixes (uniform over the
// workgroup: scalar loads from the argument block).  Where every pointer of a tensor is 16-byte aligned the chunk moves as float4
// (4 per lane and stream, all loads of a lane issued before its first use); otherwise, and for the tail past the last whole quad, per
// element.  Memory-bound: 28 bytes per parameter for Adam (+ 8 per EMA copy), so the arithmetic -- correctly rounded sqrt and
// divide, torch.optim's own rounding sequence (see `update`) -- is free.  No atomics; every sum of the norm has a fixed order.
#include "ap_common.h"

namespace ap {

constexpr int OPT_CHUNK = 4096;            // elements per workgroup: 256 lanes x 4 float4
constexpr int OPT_THREADS = 256;
constexpr int OPT_SLAB = 47;               // descriptors per launch: 47 x 80 + 48 x 4 + 72 = 4024 bytes of the 4096

struct OptHyper {                          // the launch's scalars, rounded to fp32 once on the host (as torch's kernels receive them)
  int kind, n_ema;
  float lr, omb1, b2, omb2, eps, wd, decay, mu;      // omb_i = 1 - beta_i, decay = 1 - lr wd (both formed in double)
  float rate[AP_OPTIM_MAX_EMA], omrate[AP_OPTIM_MAX_EMA];
};

struct OptArgs {
  ap_optim_tensor t[OPT_SLAB];
  uint32_t first[OPT_SLAB + 1];            // first[i]: chunks of the descriptors before i; first[n]: the grid
  OptHyper h;
};
static_assert(sizeof(ap_optim_tensor) == 80, "descriptor layout is part of the ABI (_native.ApOptimTensor)");
static_assert(sizeof(OptArgs) <= 4096, "the table must fit the kernel argument block");

struct SqnArgs {
  const float *g[OPT_SLAB];
  uint64_t n[OPT_SLAB];
  uint32_t first[OPT_SLAB + 1];
};
static_assert(sizeof(SqnArgs) <= 4096, "the table must fit the kernel argument block");

// descriptor of this workgroup's chunk: the last i with first[i] <= chunk (descriptors without elements own no chunk)
__device__ __forceinline__ int find_tensor(const uint32_t *first, int n, uint32_t chunk) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= chunk) lo = mid; else hi = mid;
  }
  return lo;
}

// One element of torch.optim's update, rounding for rounding what torch's default path on the device computes (its foreach operators
// round to fp32 after every operator, and inside one they fuse: `add(alpha)`, `lerp`, `addcmul`, `addcdiv` are each ONE fma -- of
// alpha and b, of the weight and end - start, of the value and the rounded product g g, of the value and the rounded quotient; sqrt and
// divide are correctly rounded).  The forms are pinned -- contraction off, every fma written out -- so that the result does not depend on
// what the compiler chooses to fuse: a native step then continues a torch.optim run, and runs beside one, bit for bit, which matters
// more than an ulp would suggest -- where a gradient entry is rounding noise around Adam's eps, one differing last bit of a parameter
// flips the next update's sign.
template <int KIND>
__device__ __forceinline__ void update(float &p, float g, float &m, float &v, const OptHyper &h, float step_size, float sqrt_bc2) {
#pragma clang fp contract(off)
  if (KIND == AP_OPTIM_ADAM || KIND == AP_OPTIM_ADAMW) {
    if (KIND == AP_OPTIM_ADAMW) p = p * h.decay;                          // _foreach_mul_(params, 1 - lr wd); decay is 1 at wd = 0
    else if (h.wd != 0.f) g = __builtin_fmaf(h.wd, p, g);                 // _foreach_add(grads, params, alpha=wd)
    const float d = g - m;                                                // _foreach_lerp_(exp_avgs, grads, 1 - beta1): either branch
    m = h.omb1 < 0.5f ? __builtin_fmaf(h.omb1, d, m) : __builtin_fmaf(-d, 1.f - h.omb1, g);
    v = v * h.b2;                                                         // _foreach_mul_(exp_avg_sqs, beta2)
    v = __builtin_fmaf(h.omb2, g * g, v);                                 // _foreach_addcmul_(exp_avg_sqs, grads, grads, 1 - beta2)
    const float denom = sqrtf(v) / sqrt_bc2 + h.eps;                      // _foreach_sqrt, _foreach_div_, _foreach_add_
    p = __builtin_fmaf(-step_size, m / denom, p);                         // _foreach_addcdiv_(params, exp_avgs, denom, -lr / bc1)
  } else {                                 // AP_OPTIM_SGD; m is the momentum buffer (zeros before the first step: mu 0 + g = g)
    if (h.wd != 0.f) g = __builtin_fmaf(h.wd, p, g);
    if (h.mu != 0.f) { m = m * h.mu; m = m + g; g = m; }                  // _foreach_mul_(bufs, mu); _foreach_add_(bufs, grads)
    p = __builtin_fmaf(-h.lr, g, p);                                      // _foreach_add_(params, grads, alpha=-lr)
  }
}

// update_ema (nn.py:65) as torch runs it: targ.mul_(rate) rounds, .add_(src, alpha=1 - rate) is one fma
__device__ __forceinline__ float ema_update(float e, float p, float rate, float omrate) {
#pragma clang fp contract(off)
  const float t = e * rate;
  return __builtin_fmaf(omrate, p, t);
}

template <int KIND>
__global__ __launch_bounds__(OPT_THREADS) void optim_step_kernel(const OptArgs a, int n_tensors) {
  const uint32_t chunk = blockIdx.x;
  const int ti = find_tensor(a.first, n_tensors, chunk);
  const ap_optim_tensor &t = a.t[ti];
  const OptHyper &h = a.h;
  const size_t base = (size_t)(chunk - a.first[ti]) * OPT_CHUNK;
  const int len = (int)(t.n - base < (uint64_t)OPT_CHUNK ? t.n - base : (uint64_t)OPT_CHUNK);
  const int n_ema = h.n_ema;
  float *p = t.param + base;
  const bool live = KIND != AP_OPTIM_EMA_ONLY && t.grad != nullptr;      // grad NULL: the EMA copies only
  const bool two = KIND == AP_OPTIM_ADAM || KIND == AP_OPTIM_ADAMW;
  const bool one = two || (KIND == AP_OPTIM_SGD && h.mu != 0.f);
  const float *g = live ? t.grad + base : nullptr;
  float *s1 = live && one ? t.state1 + base : nullptr;
  float *s2 = live && two ? t.state2 + base : nullptr;
  float *e[AP_OPTIM_MAX_EMA];
  uintptr_t bits = (uintptr_t)t.param | (uintptr_t)g | (uintptr_t)s1 | (uintptr_t)s2;
#pragma unroll
  for (int k = 0; k < AP_OPTIM_MAX_EMA; k++) {
    e[k] = k < n_ema ? t.ema[k] + base : nullptr;
    bits |= (uintptr_t)e[k];
  }
  const float ss = t.step_size, sb = t.sqrt_bc2;
  int done = 0;
  if ((bits & 15) == 0) {                  // every stream 16-byte aligned (a chunk starts 16 KB into its tensor): whole quads as float4
    const int nq = len >> 2;
    constexpr int Q = OPT_CHUNK / 4 / OPT_THREADS;
    float4 P[Q], G[Q], M[Q], V[Q];
#pragma unroll
    for (int j = 0; j < Q; j++) {
      const int q = threadIdx.x + j * OPT_THREADS;
      if (q < nq) {
        P[j] = ((const float4 *)p)[q];
        if (live) {
          G[j] = ((const float4 *)g)[q];
          if (one) M[j] = ((const float4 *)s1)[q];
          if (two) V[j] = ((const float4 *)s2)[q];
        }
      }
    }
    if (live) {
#pragma unroll
      for (int j = 0; j < Q; j++) {
        const int q = threadIdx.x + j * OPT_THREADS;
        if (q < nq) {
          update<KIND>(P[j].x, G[j].x, M[j].x, V[j].x, h, ss, sb);
          update<KIND>(P[j].y, G[j].y, M[j].y, V[j].y, h, ss, sb);
          update<KIND>(P[j].z, G[j].z, M[j].z, V[j].z, h, ss, sb);
          update<KIND>(P[j].w, G[j].w, M[j].w, V[j].w, h, ss, sb);
          ((float4 *)p)[q] = P[j];
          if (one) ((float4 *)s1)[q] = M[j];
          if (two) ((float4 *)s2)[q] = V[j];
        }
      }
    }
    for (int k = 0; k < n_ema; k++) {
      const float r = h.rate[k], om = h.omrate[k];
#pragma unroll
      for (int j = 0; j < Q; j++) {
        const int q = threadIdx.x + j * OPT_THREADS;
        if (q < nq) {
          float4 E = ((const float4 *)e[k])[q];
          E.x = ema_update(E.x, P[j].x, r, om);
          E.y = ema_update(E.y, P[j].y, r, om);
          E.z = ema_update(E.z, P[j].z, r, om);
          E.w = ema_update(E.w, P[j].w, r, om);
          ((float4 *)e[k])[q] = E;
        }
      }
    }
    done = nq << 2;
  }
  for (int i = done + threadIdx.x; i < len; i += OPT_THREADS) {          // a view at any 4-byte offset, and every tail
    float P = p[i];
    if (live) {
      float M = one ? s1[i] : 0.f, V = two ? s2[i] : 0.f;
      update<KIND>(P, g[i], M, V, h, ss, sb);
      p[i] = P;
      if (one) s1[i] = M;
      if (two) s2[i] = V;
    }
    for (int k = 0; k < n_ema; k++) e[k][i] = ema_update(e[k][i], P, h.rate[k], h.omrate[k]);
  }
}

__global__ __launch_bounds__(OPT_THREADS) void optim_sqnorm_kernel(const SqnArgs a, int n_tensors, double *part) {
  __shared__ double red[OPT_THREADS];
  const uint32_t chunk = blockIdx.x;
  const int ti = find_tensor(a.first, n_tensors, chunk);
  const size_t base = (size_t)(chunk - a.first[ti]) * OPT_CHUNK;
  const uint64_t left = a.n[ti] - base;
  const int len = (int)(left < (uint64_t)OPT_CHUNK ? left : (uint64_t)OPT_CHUNK);
  const float *g = a.g[ti] + base;
  double s = 0.0;                          // an fp32 square is exact in fp64
  int done = 0;
  if (((uintptr_t)g & 15) == 0) {
    const int nq = len >> 2;
    for (int q = threadIdx.x; q < nq; q += OPT_THREADS) {
      const float4 G = ((const float4 *)g)[q];
      s += (double)G.x * (double)G.x;
      s += (double)G.y * (double)G.y;
      s += (double)G.z * (double)G.z;
      s += (double)G.w * (double)G.w;
    }
    done = nq << 2;
  }
  for (int i = done + threadIdx.x; i < len; i += OPT_THREADS) s += (double)g[i] * (double)g[i];
  s = block_tree<OPT_THREADS>(s, red, SumOp{});
  if (threadIdx.x == 0) part[chunk] = s;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_sqnorm_final_kernel(const double *part, size_t n, double *out) {
  __shared__ double red[OPT_THREADS];
  double s = 0.0;
  for (size_t i = threadIdx.x; i < n; i += OPT_THREADS) s += part[i];
  s = block_tree<OPT_THREADS>(s, red, SumOp{});
  if (threadIdx.x == 0) out[0] = s;
}

static size_t chunks_of(uint64_t n) { return (size_t)((n + OPT_CHUNK - 1) / OPT_CHUNK); }

}  // namespace ap

using namespace ap;

extern "C" {

int ap_optim_slab(void) { return OPT_SLAB; }
int ap_optim_chunk(void) { return OPT_CHUNK; }

int ap_optim_step(const ap_optim_tensor *tensors, int n_tensors, const ap_optim_hyper *hp, void *stream) {
  if (!hp || n_tensors < 0 || (n_tensors > 0 && !tensors)) { set_error("ap_optim_step: null argument"); return -22; }
  const int kind = hp->kind;
  if (kind != AP_OPTIM_ADAM && kind != AP_OPTIM_ADAMW && kind != AP_OPTIM_SGD && kind != AP_OPTIM_EMA_ONLY) {
    set_error("ap_optim_step: unknown kind %d", kind);
    return -22;
  }
  if (hp->n_ema < 0 || hp->n_ema > AP_OPTIM_MAX_EMA) { set_error("ap_optim_step: n_ema = %d outside [0, %d]", hp->n_ema, AP_OPTIM_MAX_EMA); return -22; }
  if (kind == AP_OPTIM_EMA_ONLY && hp->n_ema < 1) { set_error("ap_optim_step: the EMA-only kind needs n_ema >= 1"); return -22; }
  if (!(hp->beta1 >= 0.0 && hp->beta1 < 1.0) || !(hp->beta2 >= 0.0 && hp->beta2 < 1.0)) {
    set_error("ap_optim_step: betas (%g, %g) outside [0, 1)", hp->beta1, hp->beta2);
    return -22;
  }
  if (!(hp->lr >= 0.0) || !(hp->eps >= 0.0) || !(hp->weight_decay >= 0.0) || !(hp->momentum >= 0.0)) {
    set_error("ap_optim_step: negative lr, eps, weight_decay or momentum (%g, %g, %g, %g)", hp->lr, hp->eps, hp->weight_decay, hp->momentum);
    return -22;
  }
  for (int k = 0; k < hp->n_ema; k++)
    if (!(hp->ema_rate[k] >= 0.0 && hp->ema_rate[k] <= 1.0)) { set_error("ap_optim_step: ema_rate[%d] = %g outside [0, 1]", k, hp->ema_rate[k]); return -22; }
  const bool two = kind == AP_OPTIM_ADAM || kind == AP_OPTIM_ADAMW;
  const bool one = two || (kind == AP_OPTIM_SGD && hp->momentum != 0.0);
  for (int i = 0; i < n_tensors; i++) {
    const ap_optim_tensor &t = tensors[i];
    if (!t.param) { set_error("ap_optim_step: tensor %d: null param", i); return -22; }
    if (kind != AP_OPTIM_EMA_ONLY && t.grad && ((one && !t.state1) || (two && !t.state2))) {
      set_error("ap_optim_step: tensor %d: null state tensor", i);
      return -22;
    }
    for (int k = 0; k < hp->n_ema; k++)
      if (!t.ema[k]) { set_error("ap_optim_step: tensor %d: null ema[%d]", i, k); return -22; }
    if (chunks_of(t.n) > 0x7fffffffu) { set_error("ap_optim_step: tensor %d has %llu elements", i, (unsigned long long)t.n); return -22; }
  }
  OptArgs a;
  a.h.kind = kind;
  a.h.n_ema = hp->n_ema;
  a.h.lr = (float)hp->lr;
  a.h.omb1 = (float)(1.0 - hp->beta1);
  a.h.b2 = (float)hp->beta2;
  a.h.omb2 = (float)(1.0 - hp->beta2);
  a.h.eps = (float)hp->eps;
  a.h.wd = (float)hp->weight_decay;
  a.h.decay = (float)(1.0 - hp->lr * hp->weight_decay);
  a.h.mu = (float)hp->momentum;
  for (int k = 0; k < AP_OPTIM_MAX_EMA; k++) {
    a.h.rate[k] = k < hp->n_ema ? (float)hp->ema_rate[k] : 0.f;
    a.h.omrate[k] = k < hp->n_ema ? (float)(1.0 - hp->ema_rate[k]) : 0.f;
  }
  hipStream_t st = (hipStream_t)stream;
  for (int t0 = 0; t0 < n_tensors; t0 += OPT_SLAB) {
    const int nt = n_tensors - t0 < OPT_SLAB ? n_tensors - t0 : OPT_SLAB;
    size_t total = 0;
    for (int i = 0; i < nt; i++) {
      a.t[i] = tensors[t0 + i];
      a.first[i] = (uint32_t)total;
      total += chunks_of(a.t[i].n);
      if (total > 0x7fffffffu) { set_error("ap_optim_step: more than 2^31 chunks in one launch"); return -22; }
    }
    for (int i = nt; i <= OPT_SLAB; i++) a.first[i] = (uint32_t)total;
    if (total == 0) continue;
    const dim3 grid((unsigned)total), block(OPT_THREADS);
    switch (kind) {
      case AP_OPTIM_ADAM: optim_step_kernel<AP_OPTIM_ADAM><<<grid, block, 0, st>>>(a, nt); break;
      case AP_OPTIM_ADAMW: optim_step_kernel<AP_OPTIM_ADAMW><<<grid, block, 0, st>>>(a, nt); break;
      case AP_OPTIM_SGD: optim_step_kernel<AP_OPTIM_SGD><<<grid, block, 0, st>>>(a, nt); break;
      default: optim_step_kernel<AP_OPTIM_EMA_ONLY><<<grid, block, 0, st>>>(a, nt); break;
    }
    AP_HIP(hipGetLastError());
  }
  return 0;
}

size_t ap_optim_sqnorm_workspace_bytes(const uint64_t *n, int n_tensors) {
  if (!n || n_tensors < 1) return sizeof(double);
  size_t total = 0;
  for (int i = 0; i < n_tensors; i++) total += chunks_of(n[i]);
  return (total ? total : 1) * sizeof(double);
}

int ap_optim_sqnorm(const float *const *grads, const uint64_t *n, int n_tensors, void *workspace, size_t ws_bytes, double *out,
                    void *stream) {
  if (!out || !workspace || n_tensors < 0 || (n_tensors > 0 && (!grads || !n))) { set_error("ap_optim_sqnorm: null argument"); return -22; }
  if (((uintptr_t)workspace & 7) || ((uintptr_t)out & 7)) { set_error("ap_optim_sqnorm: workspace and out must be 8-byte aligned"); return -22; }
  for (int i = 0; i < n_tensors; i++) {
    if (!grads[i]) { set_error("ap_optim_sqnorm: tensor %d: null grad", i); return -22; }
    if (chunks_of(n[i]) > 0x7fffffffu) { set_error("ap_optim_sqnorm: tensor %d has %llu elements", i, (unsigned long long)n[i]); return -22; }
  }
  const size_t need = ap_optim_sqnorm_workspace_bytes(n, n_tensors);
  if (ws_bytes < need) { set_error("ap_optim_sqnorm: workspace holds %zu bytes, %zu needed", ws_bytes, need); return -22; }
  hipStream_t st = (hipStream_t)stream;
  double *part = (double *)workspace;
  size_t done = 0;
  SqnArgs a;
  for (int t0 = 0; t0 < n_tensors; t0 += OPT_SLAB) {
    const int nt = n_tensors - t0 < OPT_SLAB ? n_tensors - t0 : OPT_SLAB;
    size_t total = 0;
    for (int i = 0; i < nt; i++) {
      a.g[i] = grads[t0 + i];
      a.n[i] = n[t0 + i];
      a.first[i] = (uint32_t)total;
      total += chunks_of(a.n[i]);
      if (total > 0x7fffffffu) { set_error("ap_optim_sqnorm: more than 2^31 chunks in one launch"); return -22; }
    }
    for (int i = nt; i < OPT_SLAB; i++) { a.g[i] = nullptr; a.n[i] = 0; }
    for (int i = nt; i <= OPT_SLAB; i++) a.first[i] = (uint32_t)total;
    if (total == 0) continue;
    optim_sqnorm_kernel<<<dim3((unsigned)total), dim3(OPT_THREADS), 0, st>>>(a, nt, part + done);
    AP_HIP(hipGetLastError());
    done += total;
  }
  optim_sqnorm_final_kernel<<<1, OPT_THREADS, 0, st>>>(part, done, out);
  AP_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
