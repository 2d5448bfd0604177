// What one wave per SIMD can issue beside back-to-back independent v_mfma_f32_32x32x2_f32 (the fp32 F(2,3) block's situation: 512
// registers per wave, nothing else resident): k fillers of one kind behind every MFMA, k = 0..16, shader cycles per MFMA (s_memtime
// around the loop, median over all waves of the chip).  The MFMA alone occupies the matrix pipe for 64 cycles; the k at which the
// figure leaves 64 is the gap's budget for that kind; the grouped columns tell a price per filler from a price per interruption.  Sizes the interleave of DIET_GATE_ / DIET_ROWS_ in ap_resblock_f32w.hip.
// Second table: the same wave with no MFMA at all -- a stream of independent vector-ALU instructions of one kind (sixteen rotating
// destinations), shader cycles per instruction: what a two-wide fp32 instruction costs against a one-wide one where the gate and the
// output transform run (between GEMM1 and GEMM2, the matrix pipe idle).
// Third table: how far ahead of its use an LDS B fragment has to be read.  One ds_read_b128 per 16 MFMAs on a conflict-free image of
// 144-byte rows (the block's X image), all four waves of the workgroup reading the same rows, the fragment consumed as the MFMAs' B
// operand D MFMAs after the read's issue; and an s_barrier among the four waves once per 256 MFMAs.  Sizes DIET_SEAM_ (and the two bits measured beside it: docs/HISTORY.md I.14).
// Load-pattern columns: the X request's own address patterns over rows 64 000 bytes apart (L = 16 000) -- the present 4-byte loads
// (32 lanes 4 or 8 bytes apart, two rows per wave) and the quad staging's 16-byte pieces (8 rows x 8 pieces, 16 rows x 4 pieces, the
// latter with the row or the piece as the fast lane index).  Fourth table: a unit of 16 MFMAs on four accumulators in the present
// order (the four in turn) and by row tile (four in a row on each), with its four weight loads behind the 16th MFMA or one behind
// every fourth, and with the quad staging's sixteen ds_write_b32, two per gap, on the X image's addresses.  Sizes DIET_QUAD_ / DIET_WROW_.
//   hipcc --offload-arch=gfx950 -O3 tools/micro/mfma_f32_gap.hip -o /tmp/mfma_f32_gap && /tmp/mfma_f32_gap > profiles/f32w_quad_gap_budget.txt
//   (profiles/f32w_seam_gap_budget.txt is the output from before the pattern columns and the fourth table were added,
//   profiles/f32w_pk_gap_budget.txt the output from before the load columns and the third table were,
//   profiles/f32w_edges_gap_budget.txt the first table's first seven columns, from before the packed columns were)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

enum { ADD, EXP, DSW, DSR, ST, ADD4, EXP4, PKADD, PKFMA, LD1, LD4, LD1R4, LD1R8, LD4Q88, LD4Q164, LD4Q164P, NKIND };   // ADD4, EXP4: the same fillers in one group of 4 k behind every fourth MFMA
static const char *const KIND_NAME[NKIND] = {"v_add_f32", "v_exp_f32", "ds_write_b32", "ds_read_b128", "buffer_store_dwordx4",
                                             "v_add_f32, grouped", "v_exp_f32, grouped", "v_pk_add_f32", "v_pk_fma_f32", "buffer_load_dword",
                                             "buffer_load_dwordx4", "dword 2 rows x 32 x 4 B", "dword 2 rows x 32 x 8 B", "dwordx4 8 rows x 8",
                                             "dwordx4 16 rows x 4", "dwordx4 16 x 4, piece fast"};
constexpr unsigned ROW_BYTES = 64000;                             // a channel row of a clip of 16 000 samples
constexpr unsigned SRC_BYTES = 20 * ROW_BYTES;                    // the read-only source of the pattern columns and the unit table
enum { S_ADD, S_FMA, S_MUL, S_EXP, S_PKADD, S_PKFMA, S_PKMUL, NSTREAM };   // the no-MFMA streams
static const char *const STREAM_NAME[NSTREAM] = {"v_add_f32", "v_fma_f32", "v_mul_f32", "v_exp_f32", "v_pk_add_f32", "v_pk_fma_f32", "v_pk_mul_f32"};
constexpr int SITERS = 1024;                                      // x 64 instructions
constexpr int ITERS = 512;                                        // x 4 MFMAs
constexpr int WAVE_BYTES = 64 * 16;                               // a wave's own store target: one 16-byte slot per lane

template <int KIND, int K>
__global__ __launch_bounds__(256, 1) void gap_kernel(float *__restrict__ sink, long long *__restrict__ cycles, float seed, const float *__restrict__ src) {
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
  f32x4 rd = {seed, seed, seed, seed}, sd = {seed, seed, seed, seed}, l4 = {seed, seed, seed, seed};
  float l1 = seed;
  const unsigned ldsaddr = 16u * tid;                             // this lane's own 16 bytes of LDS
  const unsigned voff = 16u * lane;
  // the wave's own WAVE_BYTES of the sink, and not a byte more: a store past them is dropped by the range check
  // (the halves as unsigned: readfirstlane returns an int, and a low half with bit 31 set must not sign-extend into the high one)
  const unsigned long long sbase = (unsigned long long)(sink + wave * (WAVE_BYTES / 4));
  const unsigned slo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)sbase);
  const unsigned shi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(sbase >> 32));
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)shi << 32) | slo), 0, WAVE_BYTES, 0x00020000);
  // the pattern columns read the shared source; every offset below ends inside SRC_BYTES (the largest: 15 rows + 64 bytes)
  const unsigned long long xbase = (unsigned long long)src;
  const unsigned xlo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)xbase);
  const unsigned xhi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(xbase >> 32));
  const __amdgpu_buffer_rsrc_t xs = __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)xhi << 32) | xlo), 0, SRC_BYTES, 0x00020000);
  const unsigned xoff = KIND == LD1R4     ? 4u * (lane & 31) + 4u * ROW_BYTES * (lane >> 5)
                        : KIND == LD1R8   ? 8u * (lane & 31) + 4u * ROW_BYTES * (lane >> 5)
                        : KIND == LD4Q88  ? ROW_BYTES * (lane & 7) + 16u * (lane >> 3)
                        : KIND == LD4Q164 ? ROW_BYTES * (lane & 15) + 16u * (lane >> 4)
                                          : ROW_BYTES * (lane >> 2) + 16u * (lane & 3);
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
        // (loads of the wave's own slot: in range, one 16-byte slot per lane)
        if (KIND == LD1) asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(l1) : "v"(voff), "s"(rs) : "memory");
        if (KIND == LD4) asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(l4) : "v"(voff), "s"(rs) : "memory");
        if (KIND == LD1R4 || KIND == LD1R8) asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "=v"(l1) : "v"(xoff), "s"(xs) : "memory");
        if (KIND == LD4Q88 || KIND == LD4Q164 || KIND == LD4Q164P)
          asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(l4) : "v"(xoff), "s"(xs) : "memory");
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15" : "+v"(rd), "+v"(l1), "+v"(l4)::"memory");   // (and past the last MFMA's result hazard)
  const long long t1 = __builtin_readcyclecounter();
  float s = rd[0] + rd[1] + rd[2] + rd[3] + l1 + l4[0] + l4[1] + l4[2] + l4[3];
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


// One ds_read_b128 per 16 MFMAs, consumed as their B operand D MFMAs after its issue (D < 0: no read at all, the table's base row).
// The image has the X image's 144-byte rows; the address does not depend on the wave: all four read the same rows.  Two fragment
// registers alternate, as in the block.  BAR: an s_barrier among the workgroup's four waves behind every 256th MFMA instead.
constexpr int DITERS = 64;                                        // x 32 MFMAs
template <int D, bool BAR>
__global__ __launch_bounds__(256, 1) void dist_kernel(float *__restrict__ sink, long long *__restrict__ cycles, float seed) {
  __shared__ __attribute__((aligned(16))) float img[32 * 36];
  const int tid = threadIdx.x, wave = (blockIdx.x * 256 + tid) >> 6, lane = tid & 63;
  for (int i = tid; i < 32 * 36; i += 256) img[i] = seed;
  __syncthreads();
  f32x16 acc[4];
  for (int i = 0; i < 4; i++)
    for (int r = 0; r < 16; r++) acc[i][r] = seed;
  const float a = seed + tid;
  f32x4 rd[2] = {{seed, seed, seed, seed}, {seed, seed, seed, seed}};
  const unsigned addr = (unsigned)(size_t)img + 144u * (lane & 31) + 16u * (lane >> 5);
  const long long t0 = __builtin_readcyclecounter();
#pragma unroll 1
  for (int it = 0; it < DITERS; it++) {
#pragma unroll
    for (int half = 0; half < 2; half++) {
#pragma unroll
      for (int m = 0; m < 16; m++) {
        asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+a"(acc[m & 3]) : "v"(a), "v"(rd[half][m & 3]));
        if (D >= 0 && m == 15 - D) asm volatile("ds_read_b128 %0, %1" : "=v"(rd[half ^ 1]) : "v"(addr) : "memory");
      }
      if (D >= 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rd[half ^ 1])::"memory");
    }
    if (BAR && (it & 7) == 7) asm volatile("s_barrier" ::: "memory");
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15" : "+v"(rd[0]), "+v"(rd[1])::"memory");
  const long long t1 = __builtin_readcyclecounter();
  float s = rd[0][0] + rd[1][1];
  for (int i = 0; i < 4; i++)
    for (int r = 0; r < 16; r++) s += acc[i][r];
  if (s == 12345.678f) sink[wave * (WAVE_BYTES / 4) + lane] = s;  // (keeps the results alive; inside the wave's own slot)
  if (lane == 0) cycles[wave] = t1 - t0;
}

// A unit as GEMM1 runs it: 16 MFMAs on four accumulators (one product's four row tiles), UITERS units per wave.
enum { U_BASE, U_ROWS, U_LD_16TH, U_LD_4TH, U_ROWS_LD_4TH, U_DSW, NUNIT };
static const char *const UNIT_NAME[NUNIT] = {"present order (the four accumulators in turn), nothing beside",
                                             "by row tile (four MFMAs in a row on each accumulator), nothing beside",
                                             "present order, four buffer_load_dwordx4 behind the 16th MFMA",
                                             "present order, one buffer_load_dwordx4 behind every 4th MFMA",
                                             "by row tile, one buffer_load_dwordx4 behind every 4th MFMA",
                                             "present order, sixteen ds_write_b32 on the quad image, two per gap in gaps 8..15"};
constexpr int UITERS = 128;                                       // x 16 MFMAs
template <int MODE>
__global__ __launch_bounds__(256, 1) void unit_kernel(float *__restrict__ sink, long long *__restrict__ cycles, float seed, const float *__restrict__ src) {
  __shared__ __attribute__((aligned(16))) float img[4 * 32 * 36];  // one chunk's X image: [product][column][k], 144-byte rows
  const int tid = threadIdx.x, wave = (blockIdx.x * 256 + tid) >> 6, lane = tid & 63;
  for (int i = tid; i < 4 * 32 * 36; i += 256) img[i] = seed;
  __syncthreads();
  f32x16 acc[4];
  for (int i = 0; i < 4; i++)
    for (int r = 0; r < 16; r++) acc[i][r] = seed;
  const float a = seed + tid, b = seed;
  f32x4 w[4] = {{seed, seed, seed, seed}, {seed, seed, seed, seed}, {seed, seed, seed, seed}, {seed, seed, seed, seed}};
  const unsigned long long xbase = (unsigned long long)src;
  const unsigned xlo = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)xbase);
  const unsigned xhi = (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(xbase >> 32));
  const __amdgpu_buffer_rsrc_t xs = __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)xhi << 32) | xlo), 0, SRC_BYTES, 0x00020000);
  const unsigned woff = 16u * lane;                               // a weight unit: 4 row tiles x 64 lanes x 16 B (+ 1024 rt below: < SRC_BYTES)
  // the quad staging's write address: channel 16 (wave & 1) + (lane & 15), quad 4 (wave >> 1) + (lane >> 4); + 144 i + 4608 comp below
  const unsigned daddr = (unsigned)(size_t)img + 4u * ((4 * (4 * ((tid >> 6) >> 1) + (lane >> 4))) * 36 + 16 * ((tid >> 6) & 1) + (lane & 15));
  const long long t0 = __builtin_readcyclecounter();
#pragma unroll 1
  for (int it = 0; it < UITERS; it++) {
#pragma unroll
    for (int m = 0; m < 16; m++) {
      const int rt = (MODE == U_ROWS || MODE == U_ROWS_LD_4TH) ? m >> 2 : m & 3;
      asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+a"(acc[rt]) : "v"(a), "v"(b));
      if (MODE == U_LD_16TH && m == 15) {
#pragma unroll
        for (int r = 0; r < 4; r++)
          asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen offset:%3" : "=v"(w[r]) : "v"(woff), "s"(xs), "i"(1024 * r) : "memory");
      }
      if ((MODE == U_LD_4TH || MODE == U_ROWS_LD_4TH) && (m & 3) == 3)
        asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen offset:%3" : "=v"(w[m >> 2]) : "v"(woff), "s"(xs), "i"(1024 * (m >> 2)) : "memory");
      if (MODE == U_DSW && m >= 8) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const int n = 2 * (m - 8) + h;                          // write n: product n >> 2, pair n & 3 of the quad
          asm volatile("ds_write_b32 %0, %1 offset:%2" : : "v"(daddr), "v"(b), "i"(4608 * (n >> 2) + 144 * (n & 3)) : "memory");
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3])::"memory");
  const long long t1 = __builtin_readcyclecounter();
  float s = w[0][0] + w[1][1] + w[2][2] + w[3][3];
  for (int i = 0; i < 4; i++)
    for (int r = 0; r < 16; r++) s += acc[i][r];
  if (s == 12345.678f) sink[wave * (WAVE_BYTES / 4) + lane] = s;  // (keeps the results alive; inside the wave's own slot)
  if (lane == 0) cycles[wave] = t1 - t0;
}

template <int MODE>
static double run_unit(float *sink, long long *cyc, int nblk, std::vector<long long> &host, const float *src) {
  for (int rep = 0; rep < 2; rep++) unit_kernel<MODE><<<nblk, 256>>>(sink, cyc, 0.f, src);
  if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "kernel failed\n"); exit(1); }
  (void)hipMemcpy(host.data(), cyc, host.size() * sizeof(long long), hipMemcpyDeviceToHost);
  std::sort(host.begin(), host.end());
  return (double)host[host.size() / 2] / (16.0 * UITERS);
}

template <int D, bool BAR>
static double run_dist(float *sink, long long *cyc, int nblk, std::vector<long long> &host) {
  for (int rep = 0; rep < 2; rep++) dist_kernel<D, BAR><<<nblk, 256>>>(sink, cyc, 0.f);
  if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "kernel failed\n"); exit(1); }
  (void)hipMemcpy(host.data(), cyc, host.size() * sizeof(long long), hipMemcpyDeviceToHost);
  std::sort(host.begin(), host.end());
  return (double)host[host.size() / 2] / (32.0 * DITERS);
}

template <int KIND>
static double run_stream(float *sink, long long *cyc, int nblk, std::vector<long long> &host) {
  for (int rep = 0; rep < 2; rep++) stream_kernel<KIND><<<nblk, 256>>>(sink, cyc, 0.f);
  if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "kernel failed\n"); exit(1); }
  (void)hipMemcpy(host.data(), cyc, host.size() * sizeof(long long), hipMemcpyDeviceToHost);
  std::sort(host.begin(), host.end());
  return (double)host[host.size() / 2] / (64.0 * SITERS);
}

static float *g_src;                                              // SRC_BYTES of zeros, read only

template <int KIND, int K>
static void run_one(float *sink, long long *cyc, int nblk, std::vector<long long> &host, double *out) {
  for (int rep = 0; rep < 2; rep++) gap_kernel<KIND, K><<<nblk, 256>>>(sink, cyc, 0.f, g_src);
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
  if (hipMalloc(&g_src, SRC_BYTES) != hipSuccess || hipMemset(g_src, 0, SRC_BYTES) != hipSuccess) return 1;
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
  run_kind<LD1>(sink, cyc, nblk, host, res[LD1]);
  run_kind<LD4>(sink, cyc, nblk, host, res[LD4]);
  run_kind<LD1R4>(sink, cyc, nblk, host, res[LD1R4]);
  run_kind<LD1R8>(sink, cyc, nblk, host, res[LD1R8]);
  run_kind<LD4Q88>(sink, cyc, nblk, host, res[LD4Q88]);
  run_kind<LD4Q164>(sink, cyc, nblk, host, res[LD4Q164]);
  run_kind<LD4Q164P>(sink, cyc, nblk, host, res[LD4Q164P]);
  const double st[NSTREAM] = {run_stream<S_ADD>(sink, cyc, nblk, host),   run_stream<S_FMA>(sink, cyc, nblk, host),
                              run_stream<S_MUL>(sink, cyc, nblk, host),   run_stream<S_EXP>(sink, cyc, nblk, host),
                              run_stream<S_PKADD>(sink, cyc, nblk, host), run_stream<S_PKFMA>(sink, cyc, nblk, host),
                              run_stream<S_PKMUL>(sink, cyc, nblk, host)};
  printf("v_mfma_f32_32x32x2_f32 back to back (four independent accumulators), one wave per SIMD, %d CUs: shader cycles per MFMA with k\n", nblk);
  printf("fillers of one kind issued behind every MFMA (median over the chip's waves, %d MFMAs per wave; tools/micro/mfma_f32_gap.hip)\n\n", 4 * ITERS);
  printf("%3s", "k");
  for (int kind = 0; kind < NKIND; kind++) printf(" %26s", KIND_NAME[kind]);
  printf("\n");
  for (int k = 0; k <= 16; k++) {
    printf("%3d", k);
    for (int kind = 0; kind < NKIND; kind++) printf(" %26.1f", res[kind][k]);
    printf("\n");
  }
  printf("\nno MFMA: a stream of independent instructions of one kind, one wave per SIMD: shader cycles per instruction (%d per wave)\n\n", 64 * SITERS);
  for (int kind = 0; kind < NSTREAM; kind++) printf("%14s %6.2f\n", STREAM_NAME[kind], st[kind]);
  const int dist[7] = {0, 1, 2, 3, 4, 8, 15};
  const double dres[7] = {run_dist<0, false>(sink, cyc, nblk, host), run_dist<1, false>(sink, cyc, nblk, host),
                          run_dist<2, false>(sink, cyc, nblk, host), run_dist<3, false>(sink, cyc, nblk, host),
                          run_dist<4, false>(sink, cyc, nblk, host), run_dist<8, false>(sink, cyc, nblk, host),
                          run_dist<15, false>(sink, cyc, nblk, host)};
  const double dbase = run_dist<-1, false>(sink, cyc, nblk, host), dbar = run_dist<-1, true>(sink, cyc, nblk, host);
  printf("\nread-to-use distance: one ds_read_b128 per 16 MFMAs (144-byte rows, the four waves of a workgroup on the same rows), consumed as\n");
  printf("the B operand D MFMAs after its issue: shader cycles per MFMA (%d MFMAs per wave) and stall per read\n\n", 32 * DITERS);
  printf("%8s %10.1f\n", "no read", dbase);
  for (int i = 0; i < 7; i++) printf("D = %4d %10.1f   %+7.1f cycles per read\n", dist[i], dres[i], 16.0 * (dres[i] - dbase));
  printf("\ns_barrier among the four waves behind every 256th MFMA (no read): %.1f cycles per MFMA, %+.1f cycles per barrier\n", dbar,
         256.0 * (dbar - dbase));
  const double ures[NUNIT] = {run_unit<U_BASE>(sink, cyc, nblk, host, g_src),     run_unit<U_ROWS>(sink, cyc, nblk, host, g_src),
                              run_unit<U_LD_16TH>(sink, cyc, nblk, host, g_src), run_unit<U_LD_4TH>(sink, cyc, nblk, host, g_src),
                              run_unit<U_ROWS_LD_4TH>(sink, cyc, nblk, host, g_src), run_unit<U_DSW>(sink, cyc, nblk, host, g_src)};
  printf("\na unit of 16 MFMAs on four accumulators (%d units per wave): shader cycles per MFMA and per unit against the first row\n\n", UITERS);
  for (int i = 0; i < NUNIT; i++) printf("%-82s %6.1f   %+7.1f cycles per unit\n", UNIT_NAME[i], ures[i], 16.0 * (ures[i] - ures[0]));
  return 0;
}
