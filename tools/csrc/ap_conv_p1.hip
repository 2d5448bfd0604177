// Tools library only (never shipped): round 6 attempt at VERDICT r5 item 5a.  Correct (tests of round 6: 6 shapes vs torch at 3e-6, slices, residual), but
// SLOWER than conv2d_f32_big2_kernel<128,64> on every layer of configs[4] it serves: 0.41-0.83 against 0.64-0.84 of the fp32 MFMA peak in place, 0.80 in its
// steady-state loop with a 13 us fixed cost per launch (K sweep) -- the 16-byte operand loads land in VGPRs beside a single wave's MFMAs and
// nothing hides them (profiles/r6_conv_pointwise_streaming_ab.txt).  Enable with ap_debug_conv_p1(1).
//
// Pointwise (1 x 1, stride 1, ungrouped) convolutions of the conv-as-GEMM family -- the UNet's attention projections, skip
// connections and ResNeXt's bottleneck layers (improved_diffusion/unet.py:222-252,184-197; models/resnext.py:67-142) -- as a plain
// fp32 GEMM  out[b][Cout][HW] = W [Cout x Cin] . x[b][Cin][HW]  on v_mfma_f32_32x32x2_f32 WITHOUT LDS and without a barrier:
//
//   * the activations already are the B operand: sample axis contiguous, so lane (j, h) of a k-step loads x[k = .. + h][n0 + 4 j .. + 3]
//     with ONE 16-byte load (512 contiguous bytes per k row and half wave) -- the four columns become the lane's column of FOUR
//     32-column MFMA tiles (tile t = columns n0 + 4 j + t), i.e. one load feeds 4 column tiles x 4 row tiles = 16 MFMAs;
//   * the weights come as the family's existing A-fragment image (conv_pack_frag_kernel: [row tile][k / 8][lane][4]; element e of octet q
//     is k = 8 q + 4 h + e): one 16-byte load per row tile and octet = four k-steps;
//   * a wave owns 128 rows x 128 columns = 256 accumulator registers, one wave per SIMD (512 registers: a ring of four octets of both
//     operands, 128 registers, hides the L2 round trip); per octet 8 loads feed 64 MFMAs (4 096 matrix-pipe cycles);
//   * the epilogue needs no transpose either: a lane holds, per row, four CONSECUTIVE samples -> 16-byte stores, the residual as
//     16-byte loads; bias / residual / ReLU / channel slices of wider tensors as the family's other kernels (ConvArgs contract).
// Taken for layers with at least one 128 x 128 wave tile per SIMD of the chip (the 16 x 16 and 32 x 32 maps at B = 256); the 8 x 8
// and 4 x 4 maps stay on conv2d_f32_big2_kernel (tile quantisation: they have fewer tiles than the chip has SIMDs).
#include "ap_common.h"

namespace ap {

// grid: (column blocks of 256, row blocks of 256); 4 waves = 2 row halves x 2 column halves.  Cout % 128 == 0, Cin % 8 == 0, HW % 4 == 0.
// xbytes / obytes: byte sizes of the tensors x / out (and res) live in (below 2^31: buffer descriptors).
__global__ __launch_bounds__(256, 1) void conv1x1_stream_kernel(const float *__restrict__ x, const float *__restrict__ afrag,
                                                                const float *__restrict__ bias, const float *__restrict__ res,
                                                                float *__restrict__ out, int Cin, int HW, int Cout, long long N, int relu,
                                                                int x_cstride, int x_coff, int o_cstride, int o_coff, unsigned xbytes,
                                                                unsigned abytes, unsigned obytes) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int KQ = Cin >> 3;
  // wave -> (row half, column half) of the workgroup's 256 x 256 tile; a 128-row layer (Cout = 128) has one row half: 128 x 512
  const int rows_wg = Cout >= 256 ? 256 : 128;
  const int wr = rows_wg == 256 ? (wave >> 1) : 0, wc = rows_wg == 256 ? (wave & 1) : wave;
  const int cols_wg = rows_wg == 256 ? 256 : 512;
  const int m0 = blockIdx.y * rows_wg + 128 * wr;                // first output channel of this wave
  const long long n0 = (long long)blockIdx.x * cols_wg + 128 * wc;
  if (m0 >= Cout || n0 >= N) return;                             // (whole-wave exit: no barrier in this kernel)
  auto uni_rsrc = [&](const void *base, unsigned bytes) {
    const uint64_t hb = (uint64_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)hb);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(hb >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), 0, (int)bytes, 0x00020000);
  };
  const __amdgpu_buffer_rsrc_t xrs = uni_rsrc(x, xbytes), wrs = uni_rsrc(afrag, abytes), ors = uni_rsrc(out, obytes);
  // this lane's four samples: n = n0 + 4 j .. + 3 (inside one image: HW % 4 == 0)
  const long long n = n0 + 4 * j;
  const bool nok = n < N;
  const int b = nok ? (int)(n / HW) : 0, p = nok ? (int)(n % HW) : 0;
  // B operand of k-step (q, e): row k = 8 q + 4 h + e of image b
  const unsigned xv = nok ? (unsigned)((((size_t)b * x_cstride + x_coff + 4 * h) * HW + p) * 4) : 0x80000000u;
  const unsigned wv = (unsigned)lane * 16u;
  const unsigned wrow = (unsigned)(m0 >> 5) * (unsigned)KQ * 1024u;   // byte offset of this wave's first row tile in the fragment image

  f32x16 acc[4][4];                                              // [row tile][column tile]
#pragma unroll
  for (int rt = 0; rt < 4; rt++)
#pragma unroll
    for (int ct = 0; ct < 4; ct++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[rt][ct][r] = 0.f;

  // the activations (HBM / L2 on a first touch) ride a ring three octets ahead, the weight fragments (L2-resident: 256 KB per 256-row
  // layer) one octet ahead: 96 operand registers beside the 256 accumulators -- with both rings four deep the allocator spilled, and a
  // scratch reload in this loop is a vector-memory load whose wait (vmcnt(0)) drains the whole ring
#ifndef AP_P1_BRING
#define AP_P1_BRING 4
#endif
  constexpr int BR = AP_P1_BRING;                                // activation ring depth (octets): a power of two dividing the unroll
  f32x4 A[2][4], Bq[BR][4];                                      // [ring slot][row tile], [ring slot][k-step e]: four columns each
  auto load_a = [&](int slot, int q) {
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
      A[slot][rt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, wv + wrow + (unsigned)rt * (unsigned)KQ * 1024u, q * 1024, 0));
  };
  auto load_b = [&](int slot, int q) {
#pragma unroll
    for (int e = 0; e < 4; e++)
      Bq[slot][e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, xv, (8 * q + e) * HW * 4, 0));
  };
  auto compute = [&](int sa, int sb) {
#pragma unroll
    for (int e = 0; e < 4; e++)
#pragma unroll
      for (int ct = 0; ct < 4; ct++)
#pragma unroll
        for (int rt = 0; rt < 4; rt++)
          acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[sa][rt][e], Bq[sb][e][ct], acc[rt][ct], 0, 0, 0);
  };
  load_b(0, 0);
  load_a(0, 0);
#pragma unroll
  for (int i = 1; i < BR - 1; i++) load_b(i, i < KQ ? i : KQ - 1);
#pragma unroll 1
  for (int q0 = 0; q0 < KQ; q0 += BR) {                          // KQ % BR == 0 (the launcher's condition)
#pragma unroll
    for (int s = 0; s < BR; s++) {
      const int q = q0 + s;
      load_a((s + 1) & 1, q + 1 < KQ ? q + 1 : KQ - 1);          // (past the end: the last octet again, unused)
      load_b((s + BR - 1) & (BR - 1), q + BR - 1 < KQ ? q + BR - 1 : KQ - 1);
      __builtin_amdgcn_sched_barrier(0);
      compute(s & 1, s);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- epilogue: register r of tile (rt, ct) is row 32 rt + (r & 3) + 8 (r >> 2) + 4 h, sample n + ct: per row four consecutive samples
  // (the residual is a plain [B][Cout][H][W] tensor even where `out` is a channel slice of a wider one: its own offsets)
  const __amdgpu_buffer_rsrc_t rrs = uni_rsrc(res ? res : out, res ? (unsigned)((size_t)(N / HW) * Cout * HW * 4) : obytes);
  const unsigned ov = nok ? (unsigned)((((size_t)b * o_cstride + o_coff + m0 + 4 * h) * HW + p) * 4) : 0x80000000u;
  const unsigned rv = nok ? (unsigned)((((size_t)b * Cout + m0 + 4 * h) * HW + p) * 4) : 0x80000000u;
#pragma unroll
  for (int rt = 0; rt < 4; rt++) {
    // (pins this row tile's four accumulator tiles in the accumulator registers up to here: the allocator otherwise moves all 256 to
    // VGPRs at the loop's exit -- there is no room -- and spills; a scratch reload anywhere costs a vmcnt(0))
    asm volatile("" : "+a"(acc[rt][0]), "+a"(acc[rt][1]), "+a"(acc[rt][2]), "+a"(acc[rt][3]));
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int row = 32 * rt + rowoff(r, 0);          // (+ 4 h: in ov)
      const unsigned off = ov + (unsigned)row * (unsigned)HW * 4u;
      f32x4 v = {acc[rt][0][r], acc[rt][1][r], acc[rt][2][r], acc[rt][3][r]};
      if (bias) {
        const float bv = bias[m0 + row + 4 * h];
        v += bv;
      }
      if (res) v += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrs, rv + (unsigned)row * (unsigned)HW * 4u, 0, 0));
      if (relu) {
        v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ors, off, 0, 0);
    }
  }
}

bool conv_p1_serves(int B, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int groups) {
  if (kh != 1 || kw != 1 || stride != 1 || pad != 0 || groups != 1) return false;
  if (Cin % 32 || Cout % 128 || (H * W) % 4) return false;
  // one 128 x 128 wave tile per SIMD of the chip at least (1 024 tiles): below that the 64-column tiles of the direct kernels fill it better
  return (long long)B * H * W * Cout >= 1024ll * 128 * 128;
}

int launch_conv_p1(const float *x, const float *afrag, const float *bias, const float *res, float *out, int B, int Cin, int H, int W, int Cout,
                   int relu, int x_cstride, int x_coff, int o_cstride, int o_coff, size_t abytes, hipStream_t st) {
  const int HW = H * W;
  const long long N = (long long)B * HW;
  const size_t xbytes = (size_t)B * x_cstride * HW * sizeof(float), obytes = (size_t)B * o_cstride * HW * sizeof(float);
  if (xbytes >= ((size_t)1 << 31) || obytes >= ((size_t)1 << 31) || abytes >= ((size_t)1 << 31)) return 1;   // (caller: the pointer-form kernels)
  const int rows_wg = Cout >= 256 ? 256 : 128, cols_wg = rows_wg == 256 ? 256 : 512;
  dim3 grid((unsigned)((N + cols_wg - 1) / cols_wg), (unsigned)((Cout + rows_wg - 1) / rows_wg));
  conv1x1_stream_kernel<<<grid, 256, 0, st>>>(x, afrag, bias, res, out, Cin, HW, Cout, N, relu, x_cstride, x_coff, o_cstride, o_coff,
                                              (unsigned)xbytes, (unsigned)abytes, (unsigned)obytes);
  AP_HIP(hipGetLastError());
  return 0;
}

}  // namespace ap
