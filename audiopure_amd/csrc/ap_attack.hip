// The bookkeeping of the adversarial-training PGD loops for gfx950 (include/audiopure.h, "PGD attack loop"): what stands between two
// model calls in `pgd` of RCNN_KWS/train.py:84-121 and adv_train_speech_commands.py:139-183 and in stage 1 of the white-box attack
// (white_box_attack.py:362-471) -- the random start, the per-sample "is it adversarial now" test with the copy of the current iterate,
// the signed-gradient or l2 update with its projection and the box step, and the fallback row at the end.  The scripts do this with one
// blocking host read per sample and iteration; here an iteration is one launch (linf) or three (l2) and nothing is read on the host.
//
// Streaming kernels over rows [B][n]: a workgroup owns one chunk of PGD_CHUNK elements of one row (grid = chunks x B).  Where the row
// bases of every stream are 16-byte aligned the chunk moves as float4 (4 per lane and stream, every load of a lane issued before its
// first use), otherwise, and for the tail past the last whole quad, per element.  The row test is uniform over the workgroup: the
// prediction is read, or every workgroup of a row takes the argmax of its K scores itself (K <= 4096: a strided scan and an LDS tree).
// Memory-bound (20 to 28 bytes per element), so the arithmetic is free and is torch's own rounding sequence, one rounding per
// operator and never an fma: the results are the bits of the scripts' loops.  The l2 step needs two row norms, of the gradient and of
// the proposed perturbation, so it is three launches: squares of g per chunk, squares of delta + step g^ per chunk (it adds the first
// launch's partials itself), and the update (it adds both).  Partials are fp64 (an fp32 square is exact there) and are added in index
// order by every lane alike: no atomics, two runs give equal bits.  Nothing is allocated, nothing synchronises.
#include "ap_common.h"

namespace ap {

constexpr int PGD_CHUNK = 4096;            // elements per workgroup: 256 lanes x 4 float4
constexpr int PGD_THREADS = 256;
constexpr int PGD_MAX_K = 4096;
constexpr int PGD_MAX_B = 65535;           // rows ride in gridDim.y

enum { PGD_INIT = 0, PGD_LINF = 1, PGD_L2 = 2 };

struct PgdArgs {
  const float *x, *g;                      // g: the gradient; PGD_INIT: the uniform draws u (NULL: the zero start)
  float *delta, *x_pert, *x_adv;
  uint8_t *found;
  const int64_t *pred, *y;
  const float *scores;
  const float *eps_rows;                   // NULL: `eps` for every row
  const double *part_g, *part_v;           // PGD_L2: [B][chunks] sums of squares per chunk
  float step, eps;
  int K, targeted, last, n, chunks;
};

struct PgdRow {                            // what one row's elements share
  float step, eps, fg, fv;
  bool has_u;
};

// torch.clamp(v, lo, hi): a NaN stays a NaN (both compares fail)
__device__ __forceinline__ float clampf(float v, float lo, float hi) {
  v = v < lo ? lo : v;
  return v > hi ? hi : v;
}
// torch.sign: (0 < g) - (g < 0), so +-0 and NaN give 0
__device__ __forceinline__ float sgn(float g) { return (float)((int)(0.f < g) - (int)(g < 0.f)); }
// torch.min(ones, b): a NaN propagates
__device__ __forceinline__ float min_one(float b) { return b < 1.f ? b : (b != b ? b : 1.f); }
// a row maximum as Tensor.max sees it: a NaN beats every number
__device__ __forceinline__ bool beats(float a, float b) { return a != a ? !(b != b) : a > b; }

// project_to_norm_ball(g, 'l2', 1) scaled by the step and added: fl(delta + fl(step fl(g fg)))
__device__ __forceinline__ float l2_proposal(float g, float delta, const PgdRow &r) {
#pragma clang fp contract(off)
  const float gh = g * r.fg;
  const float t = r.step * gh;
  return delta + t;
}

// One element: the perturbation the iteration proposes, then the box step  delta = fl(clamp(fl(x + d), -1, 1) - x),  x_pert = fl(x + delta)
template <int KIND>
__device__ __forceinline__ void update(float x, float g, float &delta, float &xp, const PgdRow &r) {
#pragma clang fp contract(off)             // (plain operators under the pragma: hipcc's __fmul_rn and its kin are inline functions
                                           //  compiled with contraction on, and fuse with their neighbours once inlined)
  float d;
  if (KIND == PGD_INIT) {
    if (!r.has_u) {                        // stage 1's zeros_like start: no box step there
      delta = 0.f;
      xp = x + 0.f;                        // (-0 + 0 = +0, as the script's x + delta gives)
      return;
    }
    d = r.eps * (2.f * g - 1.f);
  } else if (KIND == PGD_LINF) {
    d = clampf(delta + r.step * sgn(g), -r.eps, r.eps);
  } else {
    d = l2_proposal(g, delta, r) * r.fv;
  }
  delta = clampf(x + d, -1.f, 1.f) - x;
  xp = x + delta;
}

// a row's norm from its per-chunk partials, added in index order by every lane alike; rounded to fp32 as torch.norm's result is
__device__ __forceinline__ float row_norm(const double *part, int chunks) {
  double s = 0.0;
  for (int c = 0; c < chunks; c++) s += part[c];
  return (float)sqrt(s);
}

// lowest index of the row maximum of z[0..K), a NaN counting as the maximum (Tensor.max); every lane returns it
// (not block_tree: the tree carries an index beside the value, with a tie rule)
__device__ __forceinline__ int row_argmax(const float *z, int K, float *sv, int *si) {
  constexpr int NONE = 0x7fffffff;
  float mv = 0.f;
  int mi = NONE;
  for (int i = threadIdx.x; i < K; i += PGD_THREADS) {     // ascending: on a tie the lane keeps its lower index
    const float v = z[i];
    if (mi == NONE || beats(v, mv)) { mv = v; mi = i; }
  }
  sv[threadIdx.x] = mv;
  si[threadIdx.x] = mi;
  __syncthreads();
  for (int w = PGD_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const float ov = sv[threadIdx.x + w], cv = sv[threadIdx.x];
      const int oi = si[threadIdx.x + w], ci = si[threadIdx.x];
      const bool same = ov == cv || (ov != ov && cv != cv);
      if (oi != NONE && (ci == NONE || beats(ov, cv) || (same && oi < ci))) { sv[threadIdx.x] = ov; si[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  return si[0];
}

__device__ __forceinline__ float row_eps(const PgdArgs &a, int b) { return a.eps_rows ? a.eps_rows[b] : a.eps; }

// the scale factors of the l2 step for one row: min(1, 1 / |g|) and, where the second norm is there, min(1, eps / |delta + step g^|)
__device__ __forceinline__ void l2_factors(const PgdArgs &a, int b, PgdRow &r, bool second) {
#pragma clang fp contract(off)
  r.fg = min_one(1.f / row_norm(a.part_g + (size_t)b * a.chunks, a.chunks));
  r.fv = second ? min_one(r.eps / row_norm(a.part_v + (size_t)b * a.chunks, a.chunks)) : 1.f;
}

// PGD_INIT: the random start.  PGD_LINF / PGD_L2: the row test, the copy of the current iterate into x_adv, then the update.
template <int KIND>
__global__ __launch_bounds__(PGD_THREADS) void pgd_step_kernel(const PgdArgs a) {
  __shared__ float sv[PGD_THREADS];
  __shared__ int si[PGD_THREADS];
  const int b = blockIdx.y;
  const size_t base = (size_t)b * a.n + (size_t)blockIdx.x * PGD_CHUNK;
  const int left = a.n - (int)blockIdx.x * PGD_CHUNK;
  const int len = left < PGD_CHUNK ? left : PGD_CHUNK;
  PgdRow r;
  r.step = a.step;
  r.eps = row_eps(a, b);
  r.fg = r.fv = 1.f;
  r.has_u = a.g != nullptr;
  bool copy = false;
  const bool upd = KIND == PGD_INIT || !a.last;
  if (KIND != PGD_INIT) {
    const int64_t p = a.pred ? a.pred[b] : (int64_t)row_argmax(a.scores + (size_t)b * a.K, a.K, sv, si);
    const bool hit = a.targeted ? p == a.y[b] : p != a.y[b];
    // found[b] is written by the row's first workgroup and only on a hit, and read only where there is none: no race within a launch
    copy = hit || (a.last && a.found[b] == 0);
    if (hit && blockIdx.x == 0 && threadIdx.x == 0) a.found[b] = 1;
    if (!copy && !upd) return;
    if (KIND == PGD_L2 && upd) l2_factors(a, b, r, true);
  }
  const float *x = a.x + base;
  const float *g = a.g ? a.g + base : nullptr;
  float *delta = a.delta + base, *xp = a.x_pert + base;
  float *xa = KIND == PGD_INIT ? nullptr : a.x_adv + base;
  const bool read_g = upd && g != nullptr, read_d = KIND != PGD_INIT && upd;
  // (the chunk starts 16 KB into its row: the row bases decide the alignment)
  const uintptr_t bits = (uintptr_t)x | (uintptr_t)g | (uintptr_t)delta | (uintptr_t)xp | (uintptr_t)xa;
  int done = 0;
  if ((bits & 15) == 0) {
    const int nq = len >> 2;
    constexpr int Q = PGD_CHUNK / 4 / PGD_THREADS;
    float4 X[Q], G[Q], D[Q], P[Q];
#pragma unroll
    for (int j = 0; j < Q; j++) {
      const int q = threadIdx.x + j * PGD_THREADS;
      X[j] = G[j] = D[j] = P[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < nq) {
        if (upd) X[j] = ((const float4 *)x)[q];
        if (read_g) G[j] = ((const float4 *)g)[q];
        if (read_d) D[j] = ((const float4 *)delta)[q];
        if (KIND != PGD_INIT) P[j] = ((const float4 *)xp)[q];
      }
    }
#pragma unroll
    for (int j = 0; j < Q; j++) {
      const int q = threadIdx.x + j * PGD_THREADS;
      if (q < nq) {
        if (copy) ((float4 *)xa)[q] = P[j];
        if (upd) {
          update<KIND>(X[j].x, G[j].x, D[j].x, P[j].x, r);
          update<KIND>(X[j].y, G[j].y, D[j].y, P[j].y, r);
          update<KIND>(X[j].z, G[j].z, D[j].z, P[j].z, r);
          update<KIND>(X[j].w, G[j].w, D[j].w, P[j].w, r);
          ((float4 *)delta)[q] = D[j];
          ((float4 *)xp)[q] = P[j];
        }
      }
    }
    done = nq << 2;
  }
  for (int i = done + threadIdx.x; i < len; i += PGD_THREADS) {           // rows at any 4-byte offset, and every tail
    float P = KIND != PGD_INIT ? xp[i] : 0.f;
    if (copy) xa[i] = P;
    if (upd) {
      float D = read_d ? delta[i] : 0.f;
      update<KIND>(x[i], read_g ? g[i] : 0.f, D, P, r);
      delta[i] = D;
      xp[i] = P;
    }
  }
}

// per-chunk sums of squares in fp64: SECOND == 0 of g into part_g, SECOND == 1 of delta + step g^ into part_v (reads part_g)
template <int SECOND>
__global__ __launch_bounds__(PGD_THREADS) void pgd_sqnorm_kernel(const PgdArgs a, double *part) {
  __shared__ double red[PGD_THREADS];
  const int b = blockIdx.y;
  const size_t base = (size_t)b * a.n + (size_t)blockIdx.x * PGD_CHUNK;
  const int left = a.n - (int)blockIdx.x * PGD_CHUNK;
  const int len = left < PGD_CHUNK ? left : PGD_CHUNK;
  PgdRow r;
  r.step = a.step;
  r.eps = row_eps(a, b);
  r.fg = r.fv = 1.f;
  r.has_u = true;
  if (SECOND) l2_factors(a, b, r, false);
  const float *g = a.g + base, *delta = a.delta + base;
  double s = 0.0;
  int done = 0;
  if ((((uintptr_t)g | (SECOND ? (uintptr_t)delta : 0)) & 15) == 0) {
    const int nq = len >> 2;
    for (int q = threadIdx.x; q < nq; q += PGD_THREADS) {
      float4 V = ((const float4 *)g)[q];
      if (SECOND) {
        const float4 D = ((const float4 *)delta)[q];
        V.x = l2_proposal(V.x, D.x, r);
        V.y = l2_proposal(V.y, D.y, r);
        V.z = l2_proposal(V.z, D.z, r);
        V.w = l2_proposal(V.w, D.w, r);
      }
      s += (double)V.x * (double)V.x;
      s += (double)V.y * (double)V.y;
      s += (double)V.z * (double)V.z;
      s += (double)V.w * (double)V.w;
    }
    done = nq << 2;
  }
  for (int i = done + threadIdx.x; i < len; i += PGD_THREADS) {
    const float v = SECOND ? l2_proposal(g[i], delta[i], r) : g[i];
    s += (double)v * (double)v;
  }
  s = block_tree<PGD_THREADS>(s, red, SumOp{});
  if (threadIdx.x == 0) part[(size_t)b * a.chunks + blockIdx.x] = s;
}

static int pgd_chunks(int n) { return (int)(((size_t)n + PGD_CHUNK - 1) / PGD_CHUNK); }

static bool pgd_overlap(const void *a, size_t na, const void *b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// What both steps check before any launch; fills the arguments.  0, or -22 with the error text set.
static int pgd_step_args(const char *who, PgdArgs &a, const float *x, const float *g, float *delta, float *x_pert, float *x_adv,
                         uint8_t *found, const int64_t *pred, const float *scores, int K, const int64_t *y, float step,
                         const float *eps_rows, float eps, int targeted, int last, int B, int n) {
  if (!x || !delta || !x_pert || !x_adv || !found || !y) { set_error("%s: null x, delta, x_pert, x_adv, found or y", who); return -22; }
  if (!last && !g) { set_error("%s: null g (only the last call, which updates nothing, may leave it out)", who); return -22; }
  if ((pred != nullptr) == (scores != nullptr)) { set_error("%s: give pred or scores, one of the two", who); return -22; }
  if (scores && (K < 1 || K > PGD_MAX_K)) { set_error("%s: K = %d outside [1, %d]", who, K, PGD_MAX_K); return -22; }
  if (B < 1 || B > PGD_MAX_B || n < 1) { set_error("%s: B = %d outside [1, %d] or n = %d < 1", who, B, PGD_MAX_B, n); return -22; }
  if (!eps_rows && !(eps >= 0.f)) { set_error("%s: eps = %g is negative or NaN", who, (double)eps); return -22; }
  if (step != step) { set_error("%s: step is NaN", who); return -22; }
  const size_t bytes = (size_t)B * n * sizeof(float);
  const void *out[3] = {delta, x_pert, x_adv};
  const char *name[3] = {"delta", "x_pert", "x_adv"};
  for (int i = 0; i < 3; i++) {
    if (pgd_overlap(out[i], bytes, x, bytes) || pgd_overlap(out[i], bytes, g, bytes)) { set_error("%s: %s overlaps x or g", who, name[i]); return -22; }
    for (int j = i + 1; j < 3; j++)
      if (pgd_overlap(out[i], bytes, out[j], bytes)) { set_error("%s: %s overlaps %s", who, name[i], name[j]); return -22; }
    if (pgd_overlap(out[i], bytes, found, (size_t)B)) { set_error("%s: %s overlaps found", who, name[i]); return -22; }
  }
  a = PgdArgs{};
  a.x = x; a.g = last ? nullptr : g; a.delta = delta; a.x_pert = x_pert; a.x_adv = x_adv; a.found = found;
  a.pred = pred; a.y = y; a.scores = scores; a.eps_rows = eps_rows;
  a.step = step; a.eps = eps; a.K = K; a.targeted = targeted != 0; a.last = last != 0; a.n = n; a.chunks = pgd_chunks(n);
  return 0;
}

}  // namespace ap

using namespace ap;

extern "C" {

int ap_pgd_chunk(void) { return PGD_CHUNK; }

int ap_pgd_init(const float *x, const float *u, float *delta, float *x_pert, float eps, int B, int n, void *stream) {
  if (!x || !delta || !x_pert) { set_error("ap_pgd_init: null x, delta or x_pert"); return -22; }
  if (B < 1 || B > PGD_MAX_B || n < 1) { set_error("ap_pgd_init: B = %d outside [1, %d] or n = %d < 1", B, PGD_MAX_B, n); return -22; }
  if (!(eps >= 0.f)) { set_error("ap_pgd_init: eps = %g is negative or NaN", (double)eps); return -22; }
  const size_t bytes = (size_t)B * n * sizeof(float);
  if (pgd_overlap(delta, bytes, x_pert, bytes) || pgd_overlap(delta, bytes, x, bytes) || pgd_overlap(x_pert, bytes, x, bytes) ||
      pgd_overlap(delta, bytes, u, bytes) || pgd_overlap(x_pert, bytes, u, bytes)) {
    set_error("ap_pgd_init: delta and x_pert must overlap neither each other nor x or u");
    return -22;
  }
  PgdArgs a{};
  a.x = x; a.g = u; a.delta = delta; a.x_pert = x_pert; a.eps = eps; a.n = n; a.chunks = pgd_chunks(n);
  pgd_step_kernel<PGD_INIT><<<dim3((unsigned)a.chunks, (unsigned)B), dim3(PGD_THREADS), 0, (hipStream_t)stream>>>(a);
  AP_HIP(hipGetLastError());
  return 0;
}

int ap_pgd_step_linf(const float *x, const float *g, float *delta, float *x_pert, float *x_adv, uint8_t *found, const int64_t *pred,
                     const float *scores, int K, const int64_t *y, float step, const float *eps_rows, float eps, int targeted, int last,
                     int B, int n, void *stream) {
  PgdArgs a;
  if (pgd_step_args("ap_pgd_step_linf", a, x, g, delta, x_pert, x_adv, found, pred, scores, K, y, step, eps_rows, eps, targeted, last, B, n))
    return -22;
  pgd_step_kernel<PGD_LINF><<<dim3((unsigned)a.chunks, (unsigned)B), dim3(PGD_THREADS), 0, (hipStream_t)stream>>>(a);
  AP_HIP(hipGetLastError());
  return 0;
}

size_t ap_pgd_l2_workspace_bytes(int B, int n) {
  if (B < 1 || n < 1) return 0;
  return (size_t)2 * B * pgd_chunks(n) * sizeof(double);
}

int ap_pgd_step_l2(const float *x, const float *g, float *delta, float *x_pert, float *x_adv, uint8_t *found, const int64_t *pred,
                   const float *scores, int K, const int64_t *y, float step, const float *eps_rows, float eps, int targeted, int last,
                   void *workspace, size_t ws_bytes, int B, int n, void *stream) {
  PgdArgs a;
  if (pgd_step_args("ap_pgd_step_l2", a, x, g, delta, x_pert, x_adv, found, pred, scores, K, y, step, eps_rows, eps, targeted, last, B, n))
    return -22;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)a.chunks, (unsigned)B), block(PGD_THREADS);
  if (!last) {                             // (the last call updates nothing: no norm is needed)
    const size_t need = ap_pgd_l2_workspace_bytes(B, n);
    if (!workspace || ((uintptr_t)workspace & 7) || ws_bytes < need) {
      set_error("ap_pgd_step_l2: workspace null, not 8-byte aligned or %zu bytes where %zu are needed", ws_bytes, need);
      return -22;
    }
    const size_t bytes = (size_t)B * n * sizeof(float);
    const void *t[5] = {x, g, delta, x_pert, x_adv};
    for (int i = 0; i < 5; i++)
      if (pgd_overlap(workspace, need, t[i], bytes)) { set_error("ap_pgd_step_l2: the workspace overlaps a tensor"); return -22; }
    double *part_g = (double *)workspace, *part_v = part_g + (size_t)B * a.chunks;
    a.part_g = part_g;
    a.part_v = part_v;
    pgd_sqnorm_kernel<0><<<grid, block, 0, st>>>(a, part_g);
    AP_HIP(hipGetLastError());
    pgd_sqnorm_kernel<1><<<grid, block, 0, st>>>(a, part_v);
    AP_HIP(hipGetLastError());
  }
  pgd_step_kernel<PGD_L2><<<grid, block, 0, st>>>(a);
  AP_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
