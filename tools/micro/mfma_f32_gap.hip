// What one wave per SIMD can issue beside back-to-back independent v_mfma_f32_32x32x2_f32 (the fp32 F(2,3) block's situation: 512
// registers per wave, nothing else resident): k fillers of one kind behind every MFMA, k = 0..16, shader cycles per MFMA (s_memtime
// around the loop, median over all waves of the chip).  The MFMA alone occupies the matrix pipe for 64 cycles; the k at which the
// figure leaves 64 is the gap's budget for that kind; the grouped columns tell a price per filler from a price per interruption.  Sizes the interleave of DIET_GATE_ / DIET_ROWS_ in ap_resblock_f32w.hip.
// Second table: the same wave with no MFMA at all -- a stream of independent vector-ALU instructions of one kind (sixteen rotating
// destinations), shader cycles per instruction: what a two-wide fp32 instruction costs against a one-wide one where the gate and the
// output transform run (between GEMM1 and GEMM2, the matrix pipe idle).
//   hipcc --offload-arch=gfx950 -O3 tools/micro/mfma_f32_gap.hip -o /tmp/mfma_f32_gap && /tmp/mfma_f32_gap > profiles/f32w_pk_gap_budget.txt
//   (profiles/f32w_edges_gap_budget.txt is the first table's first seven columns, from before the packed columns were added)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

enum { ADD, EXP, DSW, DSR, ST, ADD4, EXP4, PKADD, PKFMA, NKIND };   // ADD4, EXP4: the same fillers in one group of 4 k behind every fourth MFMA
static const char *const KIND_NAME[NKIND] = {"v_add_f32", "v_exp_f32", "ds_write_b32", "ds_read_b128", "buffer_store_dwordx4",
                                             "v_add_f32, grouped", "v_exp_f32, grouped", "v_pk_add_f32", "v_pk_fma_f32"};
enum { S_ADD, S_FMA, S_MUL, S_EXP, S_PKADD, S_PKFMA, S_PKMUL, NSTREAM };   // the no-MFMA streams
static const char *const STREAM_NAME[NSTREAM] = {"v_add_f32", "v_fma_f32", "v_mul_f32", "v_exp_f32", "v_pk_add_f32", "v_pk_fma_f32", "v_pk_mul_f32"};
constexpr int SITERS = 1024;                                      // x 64 instructions
constexpr int ITERS = 512;                                        // x 4 MFMAs
constexpr int WAVE_BYTES = 64 * 16;                               // a wave's own store target: one 16-byte slot per lane

template <int KIND, int K>
__global__ __launch_bounds__(256, 1) void gap_kernel(float *__restrict__ sink, long long *__restrict__ cycles, float seed) {
  __shared__ float lds[256 * 4];
  const int tid = threadIdx.x, wave = (blockIdx.x * 256 + tid) >> 6, lane = tid & 63;
  lds[4 * tid] = lds[4 * tid + 1] = lds[4 * tid + 2] = lds[4 * tid + 3] = seed;
  __syncthreads();
  f32x16 acc[4];
  for (int i = 0; i < 4; i++)
    for (int r = 0; r < 16; r++) acc[i][r] = seed;
  float a = seed + tid, b = seed, c = seed * 3.f, f[16];
  for (int i = 0; i < 16; i++) f[i] = seed * i;
  f32x2 f2[16], c2 = {c, c};
  for (int i = 0; i < 16; i++) f2[i] = f32x2{seed * i, seed};
  f32x4 rd = {seed, seed, seed, seed}, sd = {seed, seed, seed, seed};
  const unsigned ldsaddr = 16u * tid;                             // this lane's own 16 bytes of LDS
  const unsigned voff = 16u * lane;
  // the wave's own WAVE_BYTES of the sink, and not a byte more: a store past them is dropped by the range check
  // (the halves as unsigned: readfirstlane returns an int, and a low half with bit 31 set must not sign-extend into the high one)
  const unsigned long long sbase = (unsigned long long)(sink + wave * (WAVE_BYTES / 4));
  const unsigned slo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)sbase);
  const unsigned shi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(sbase >> 32));
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)shi << 32) | slo), 0, WAVE_BYTES, 0x00020000);
  const long long t0 = __builtin_readcyclecounter();
#pragma unroll 1
  for (int it = 0; it < ITERS; it++) {
#pragma unroll
    for (int m = 0; m < 4; m++) {
      asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+a"(acc[m]) : "v"(a), "v"(b));
#pragma unroll
      for (int k = 0; k < (KIND == ADD4 || KIND == EXP4 ? (m == 3 ? 4 * K : 0) : K); k++) {
        if (KIND == ADD || KIND == ADD4) asm volatile("v_add_f32 %0, %0, %1" : "+v"(f[k & 15]) : "v"(c));   // (c: no operand of the MFMA)
        if (KIND == EXP || KIND == EXP4) asm volatile("v_exp_f32 %0, %0" : "+v"(f[k & 15]));
        if (KIND == PKADD) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(f2[k & 15]) : "v"(c2));
        if (KIND == PKFMA) asm volatile("v_pk_fma_f32 %0, %0, %1, %1" : "+v"(f2[k & 15]) : "v"(c2));
        if (KIND == DSW) asm volatile("ds_write_b32 %0, %1" : : "v"(ldsaddr), "v"(b) : "memory");
        if (KIND == DSR) asm volatile("ds_read_b128 %0, %1" : "=v"(rd) : "v"(ldsaddr) : "memory");
        if (KIND == ST) asm volatile("buffer_store_dwordx4 %0, %1, %2, 0 offen" : : "v"(sd), "v"(voff), "s"(rs) : "memory");
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15" : "+v"(rd)::"memory");   // (and past the last MFMA's result hazard)
  const long long t1 = __builtin_readcyclecounter();
  float s = rd[0] + rd[1] + rd[2] + rd[3];
  for (int i = 0; i < 16; i++) s += f[i] + f2[i][0] + f2[i][1];
  for (int i = 0; i < 4; i++)
    for (int r = 0; r < 16; r++) s += acc[i][r];
  if (s == 12345.678f) sink[wave * (WAVE_BYTES / 4) + lane] = s;  // (keeps the results alive; inside the wave's own slot)
  if (lane == 0) cycles[wave] = t1 - t0;
}

// no MFMA: 64 independent instructions of one kind per iteration (destination k & 15: a result is read again sixteen issues later)
template <int KIND>
__global__ __launch_bounds__(256, 1) void stream_kernel(float *__restrict__ sink, long long *__restrict__ cycles, float seed) {
  const int tid = threadIdx.x, wave = (blockIdx.x * 256 + tid) >> 6, lane = tid & 63;
  float c = seed * 3.f, f[16];
  f32x2 f2[16], c2 = {c, seed};
  for (int i = 0; i < 16; i++) f[i] = seed * i, f2[i] = f32x2{seed * i, seed + tid};
  const long long t0 = __builtin_readcyclecounter();
#pragma unroll 1
  for (int it = 0; it < SITERS; it++) {
#pragma unroll
    for (int k = 0; k < 64; k++) {
      if (KIND == S_ADD) asm volatile("v_add_f32 %0, %0, %1" : "+v"(f[k & 15]) : "v"(c));
      if (KIND == S_FMA) asm volatile("v_fma_f32 %0, %0, %1, %1" : "+v"(f[k & 15]) : "v"(c));
      if (KIND == S_MUL) asm volatile("v_mul_f32 %0, %0, %1" : "+v"(f[k & 15]) : "v"(c));
      if (KIND == S_EXP) asm volatile("v_exp_f32 %0, %0" : "+v"(f[k & 15]));
      if (KIND == S_PKADD) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(f2[k & 15]) : "v"(c2));
      if (KIND == S_PKFMA) asm volatile("v_pk_fma_f32 %0, %0, %1, %1" : "+v"(f2[k & 15]) : "v"(c2));
      if (KIND == S_PKMUL) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(f2[k & 15]) : "v"(c2));
    }
  }
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
  const long long t1 = __builtin_readcyclecounter();
  float s = 0.f;
  for (int i = 0; i < 16; i++) s += f[i] + f2[i][0] + f2[i][1];
  if (s == 12345.678f) sink[wave * (WAVE_BYTES / 4) + lane] = s;  // (keeps the results alive; inside the wave's own slot)
  if (lane == 0) cycles[wave] = t1 - t0;
}

template <int KIND>
static double run_stream(float *sink, long long *cyc, int nblk, std::vector<long long> &host) {
  for (int rep = 0; rep < 2; rep++) stream_kernel<KIND><<<nblk, 256>>>(sink, cyc, 0.f);
  if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "kernel failed\n"); exit(1); }
  (void)hipMemcpy(host.data(), cyc, host.size() * sizeof(long long), hipMemcpyDeviceToHost);
  std::sort(host.begin(), host.end());
  return (double)host[host.size() / 2] / (64.0 * SITERS);
}

template <int KIND, int K>
static void run_one(float *sink, long long *cyc, int nblk, std::vector<long long> &host, double *out) {
  for (int rep = 0; rep < 2; rep++) gap_kernel<KIND, K><<<nblk, 256>>>(sink, cyc, 0.f);
  if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "kernel failed\n"); exit(1); }
  (void)hipMemcpy(host.data(), cyc, host.size() * sizeof(long long), hipMemcpyDeviceToHost);
  std::sort(host.begin(), host.end());
  out[K] = (double)host[host.size() / 2] / (4.0 * ITERS);
}

template <int KIND, int K = 0>
static void run_kind(float *sink, long long *cyc, int nblk, std::vector<long long> &host, double *out) {
  run_one<KIND, K>(sink, cyc, nblk, host, out);
  if constexpr (K < 16) run_kind<KIND, K + 1>(sink, cyc, nblk, host, out);
}

int main() {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
  const int nblk = prop.multiProcessorCount, nwave = nblk * 4;
  float *sink;
  long long *cyc;
  (void)hipMalloc(&sink, (size_t)nwave * WAVE_BYTES);
  (void)hipMalloc(&cyc, nwave * sizeof(long long));
  (void)hipMemset(sink, 0, (size_t)nwave * WAVE_BYTES);
  std::vector<long long> host(nwave);
  double res[NKIND][17];
  run_kind<ADD>(sink, cyc, nblk, host, res[ADD]);
  run_kind<EXP>(sink, cyc, nblk, host, res[EXP]);
  run_kind<DSW>(sink, cyc, nblk, host, res[DSW]);
  run_kind<DSR>(sink, cyc, nblk, host, res[DSR]);
  run_kind<ST>(sink, cyc, nblk, host, res[ST]);
  run_kind<ADD4>(sink, cyc, nblk, host, res[ADD4]);
  run_kind<EXP4>(sink, cyc, nblk, host, res[EXP4]);
  run_kind<PKADD>(sink, cyc, nblk, host, res[PKADD]);
  run_kind<PKFMA>(sink, cyc, nblk, host, res[PKFMA]);
  const double st[NSTREAM] = {run_stream<S_ADD>(sink, cyc, nblk, host),   run_stream<S_FMA>(sink, cyc, nblk, host),
                              run_stream<S_MUL>(sink, cyc, nblk, host),   run_stream<S_EXP>(sink, cyc, nblk, host),
                              run_stream<S_PKADD>(sink, cyc, nblk, host), run_stream<S_PKFMA>(sink, cyc, nblk, host),
                              run_stream<S_PKMUL>(sink, cyc, nblk, host)};
  printf("v_mfma_f32_32x32x2_f32 back to back (four independent accumulators), one wave per SIMD, %d CUs: shader cycles per MFMA with k\n", nblk);
  printf("fillers of one kind issued behind every MFMA (median over the chip's waves, %d MFMAs per wave; tools/micro/mfma_f32_gap.hip)\n\n", 4 * ITERS);
  printf("%3s", "k");
  for (int kind = 0; kind < NKIND; kind++) printf(" %21s", KIND_NAME[kind]);
  printf("\n");
  for (int k = 0; k <= 16; k++) {
    printf("%3d", k);
    for (int kind = 0; kind < NKIND; kind++) printf(" %21.1f", res[kind][k]);
    printf("\n");
  }
  printf("\nno MFMA: a stream of independent instructions of one kind, one wave per SIMD: shader cycles per instruction (%d per wave)\n\n", 64 * SITERS);
  for (int kind = 0; kind < NSTREAM; kind++) printf("%14s %6.2f\n", STREAM_NAME[kind], st[kind]);
  return 0;
}
