// What only kernels need, once: the vector types, the accumulator row map, the gates, the three-way bf16 split, the XCD-contiguous
// workgroup numbering and the bf16 block kernels' tile constants.  Sibling kernels whose results must agree bit for bit (the bf16
// block family; the fp32 family) agree because they call the one definition here.  Included by ap_common.h under hipcc.
#pragma once
#include <type_traits>

namespace ap {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

using I0 = std::integral_constant<int, 0>;
using I1 = std::integral_constant<int, 1>;
using I2 = std::integral_constant<int, 2>;
using I3 = std::integral_constant<int, 3>;

// The bf16 block kernels' LDS images and weight fragments (ap_resblock_bf16p / bf16s / bf16u / bf16us.hip)
constexpr int BF_XS = 3 * 32 + 8;        // bf16 per column row of the X chunk image (3 taps x 32 channels; 208-B rows: conflict-free ds_read_b128 B fragments)
constexpr int BF_GS = 256 + 8;           // bf16 per column row of the g image (528-B rows)
constexpr unsigned BF_FR = 64 * 16;      // bytes of one row tile's fragment of a k-step

// row of accumulator register r of a 32x32 MFMA tile held by lane half hh
__device__ __forceinline__ int rowoff(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// position p of a 32-channel row of the bf16 u image holds channel swap23(p) of the chunk (bits 2 and 3 swapped: the order of a
// 32 x 32 accumulator tile's registers, ap_resblock_bf16u.hip)
__host__ __device__ __forceinline__ int swap23(int p) { return (p & ~12) | ((p & 4) << 1) | ((p & 8) >> 1); }

// XCD-contiguous workgroup numbering: workgroups b, b + 8, ... share an XCD (round-robin dispatch), so XCD x takes the x-th
// contiguous run of the nblk logical indices.  Placement only -- any bijection gives the same results.
__device__ __forceinline__ int xcd_logical(int bid, int nblk) {
  const int xcd = bid & 7, idx = bid >> 3, q = nblk >> 3, r = nblk & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// Which (clip, tile) a workgroup of a one-tile-per-workgroup block kernel takes.  Placement only; for the per-XCD L2s: each XCD
// takes a contiguous run of (clip, position) work (xcd_logical), and inside a clip position p maps to tile r + k s (residue classes
// r = 0 .. s-1 in turn, s = dilation / tile width capped at 16): the tiles an XCD holds at one time then include the ones d columns
// away, whose centre columns are this tile's +-d taps.
__device__ __forceinline__ void ap_tile_of_block(int bid, int nblk, int ntiles, int d, int tile_cols, int &b, int &tile) {
  const int logical = xcd_logical(bid, nblk);
  b = logical / ntiles;
  int p = logical % ntiles;
  const int s = min(max(d / tile_cols, 1), 16);
  if (s > 1) {
    const int wq = ntiles / s, wrem = ntiles % s, cut = wrem * (wq + 1);
    const int cls = p < cut ? p / (wq + 1) : wrem + (p - cut) / wq;
    const int k = p < cut ? p % (wq + 1) : (p - cut) % wq;
    p = cls + k * s;
  }
  tile = p;
}

// ---- the fp32 modes' gate (AP_PREC_F32, AP_PREC_F32_SPLIT: the gate is not where the two differ) --------------------------------
// exp(x) on the hardware exp2 with a compensated argument: ~2 ulp over the range the gate uses.
__device__ __forceinline__ float exp_acc(float x) {
  const float L2E_HI = 1.44269502162933349609375f;   // float(log2 e)
  const float L2E_LO = 1.92596299e-8f;               // log2 e - L2E_HI
  float t = x * L2E_HI;
  float r = __builtin_fmaf(x, L2E_HI, -t);
  r = __builtin_fmaf(x, L2E_LO, r);
  float e = __builtin_amdgcn_exp2f(t);
  return __builtin_fmaf(e, r * 0.693147182464599609375f, e);
}

// tanh(a) * sigmoid(b) = (E - 1) / ((E + 1) (1 + F)),  E = e^{2a}, F = e^{-b}   (WaveNet.py:90)
__device__ __forceinline__ float gate(float a, float b) {
  a = fminf(fmaxf(a, -15.0f), 15.0f);    // tanh(+-15) == +-1 in fp32
  b = fmaxf(b, -80.0f);                  // keep F finite: sigmoid(-80) ~ 1.8e-35
  float E = exp_acc(2.0f * a);
  float F = exp_acc(-b);
  return (E - 1.0f) * __builtin_amdgcn_rcpf((E + 1.0f) * (1.0f + F));
}

// gate() on a pair of values, element for element the same operations (ap_resblock_f32w.hip's 16-byte forms, whose gate phase runs
// with the matrix pipe idle: a v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 is one issue slot for two gates, each element with the
// bits of the one-wide instruction).  The clamps and the three transcendentals stay per element.  gate()'s 2 a and -b are folded
// into exp_acc's constants -- (2 a) c and a (2 c) are the same real number, so every product and fma rounds to the same float:
// hi, lo = 2 L2E_HI, 2 L2E_LO for E and -L2E_HI, -L2E_LO for F.  No contraction: gate() has no mul feeding an add outside its
// written fma's, and the pair form must not grow one.
__device__ __forceinline__ f32x2 exp_acc2(f32x2 x, float hi, float lo) {
#pragma clang fp contract(off)
  const f32x2 h2 = {hi, hi}, l2 = {lo, lo};
  const f32x2 t = x * h2;
  f32x2 r = __builtin_elementwise_fma(x, h2, -t);
  r = __builtin_elementwise_fma(x, l2, r);
  const f32x2 e = {__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
  return __builtin_elementwise_fma(e, r * 0.693147182464599609375f, e);
}

__device__ __forceinline__ f32x2 gate2(f32x2 a, f32x2 b) {
#pragma clang fp contract(off)
  const float L2E_HI = 1.44269502162933349609375f, L2E_LO = 1.92596299e-8f;   // exp_acc's
  const f32x2 ac = {fminf(fmaxf(a[0], -15.0f), 15.0f), fminf(fmaxf(a[1], -15.0f), 15.0f)};
  const f32x2 bc = {fmaxf(b[0], -80.0f), fmaxf(b[1], -80.0f)};
  const f32x2 E = exp_acc2(ac, 2.0f * L2E_HI, 2.0f * L2E_LO);
  const f32x2 F = exp_acc2(bc, -L2E_HI, -L2E_LO);
  const f32x2 den = (E + 1.0f) * (1.0f + F);
  const f32x2 rc = {__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
  return (E - 1.0f) * rc;
}

// ---- the bf16 modes' gate, on a pair of values ---------------------------------------------------------------------------------
// tanh(a) sigmoid(b) = (1 - E) / ((1 + E)(1 + F)), E = e^(-2a), F = e^(-b).  a is clamped to [-16, 16] first (one v_med3;
// tanh(+-16) rounds to +-1 in fp32, so the clamp changes no result): E stays finite, the sign comes out of 1 - E, and no
// abs / copysign pair is needed.  F may overflow to +inf: the denominator is +inf then and the gate 0, which is the limit.
// The same arithmetic, element for element, as the scalar gate_fast of tools/csrc/ap_resblock_bf16.hip (the A/B baseline).
// On a pair of values: plain arithmetic as two-wide fp32 operations (v_pk_mul_f32 / v_pk_add_f32: one issue slot for two
// gates; every file that calls it is built with -fno-slp-vectorize, so the pairing is written out), the three transcendentals
// per gate stay scalar; the caller converts the pair to bf16 with one v_cvt_pk_bf16_f32.
__device__ __forceinline__ f32x2 gate_fast2(f32x2 a, f32x2 b) {
  const f32x2 ac = {__builtin_amdgcn_fmed3f(a[0], -16.0f, 16.0f), __builtin_amdgcn_fmed3f(a[1], -16.0f, 16.0f)};
  const f32x2 ea = ac * -2.885390081777926815f;
  const f32x2 eb = b * -1.442695040888963407f;
  const f32x2 E = {__builtin_amdgcn_exp2f(ea[0]), __builtin_amdgcn_exp2f(ea[1])};
  const f32x2 F = {__builtin_amdgcn_exp2f(eb[0]), __builtin_amdgcn_exp2f(eb[1])};
  const f32x2 den = (E + 1.0f) * (F + 1.0f);
  const f32x2 r = {__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
  return (1.0f - E) * r;
}

// gate_fast2 that also hands out the gate's two derivative factors (the white-box backward's operands: ap_resblock_bwd_bf16.hip):
// f1 = d(tanh . sigmoid)/d(tanh arg) = sg (1 - th^2), f2 = d/d(sigmoid arg) = th sg (1 - sg), from the quantities the gate forms anyway
// (sg = (1 + E) r, th = g (1 + F), th sg = g).  The returned gate is gate_fast2's, operation for operation: a forward pass that keeps
// the factors writes the same h' and g image as one that does not.  F = +inf (sigmoid argument below -88): g = sg = 0 and 0 . inf is
// taken as 0.
__device__ __forceinline__ f32x2 gate_fast2_save(f32x2 a, f32x2 b, f32x2 &f1, f32x2 &f2) {
#pragma clang fp contract(off)                                  // one operation order in every instantiation (1 - th th as an fma in some, not in others: seen)
  const f32x2 ac = {__builtin_amdgcn_fmed3f(a[0], -16.0f, 16.0f), __builtin_amdgcn_fmed3f(a[1], -16.0f, 16.0f)};
  const f32x2 ea = ac * -2.885390081777926815f;
  const f32x2 eb = b * -1.442695040888963407f;
  const f32x2 E = {__builtin_amdgcn_exp2f(ea[0]), __builtin_amdgcn_exp2f(ea[1])};
  const f32x2 F = {__builtin_amdgcn_exp2f(eb[0]), __builtin_amdgcn_exp2f(eb[1])};
  const f32x2 opE = E + 1.0f, opF = F + 1.0f;
  const f32x2 den = opE * opF;
  const f32x2 r = {__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
  const f32x2 g = (1.0f - E) * r;
  const f32x2 sg = opE * r;
  f32x2 th = g * opF;
  th[0] = F[0] > 3.0e38f ? 0.f : th[0];
  th[1] = F[1] > 3.0e38f ? 0.f : th[1];
  f1 = sg * (1.0f - th * th);
  f2 = g * (1.0f - sg);
  return g;
}

// ---- the three-way bf16 split of AP_PREC_F32_SPLIT ----------------------------------------------------------------------------
// x = p[0] + p[1] + p[2] exactly (fp32 has 24 mantissa bits, each part carries 8)
__device__ __forceinline__ void split3(float x, __bf16 (&p)[3]) {
  p[0] = (__bf16)x;
  const float r1 = x - (float)p[0];
  p[1] = (__bf16)r1;
  p[2] = (__bf16)(r1 - (float)p[1]);
}

// four values at once, the parts packed two per dword; written so the conversions lower to v_cvt_pk_bf16_f32 (two per
// instruction) and the widenings to one shift / mask: 11 VALU per pair instead of ~20
__device__ __forceinline__ void split3x4(const float (&x)[4], u32x2 (&out)[3]) {
#pragma unroll
  for (int pr = 0; pr < 2; pr++) {
    float v0 = x[2 * pr], v1 = x[2 * pr + 1];
#pragma unroll
    for (int s = 0; s < 3; s++) {
      const unsigned pk = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{v0, v1}, bf16x2));
      out[s][pr] = pk;
      if (s < 2) {
        v0 -= __builtin_bit_cast(float, pk << 16);
        v1 -= __builtin_bit_cast(float, pk & 0xffff0000u);
      }
    }
  }
}

// the six partial products kept of the nine, as (weight split, activation split)
#define AP_SPLIT_TERMS(F) F(0, 0) F(0, 1) F(1, 0) F(0, 2) F(2, 0) F(1, 1)

// ---- the non-block kernels' activations and counter-based random numbers -------------------------------------------------------
__device__ __forceinline__ float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float silu(float x) { return x / (1.0f + expf(-x)); }

// d * act'(y1) for the activation codes of the GroupNorm entry points: 0 none, 1 ReLU, 2 SiLU (silu' = sg (1 + y (1 - sg)))
__device__ __forceinline__ float act_grad(float d, float y1, int act) {
  if (act == 2) {
    const float sg = sigmoid(y1);
    return d * (sg * (1.0f + y1 * (1.0f - sg)));
  }
  if (act == 1) return y1 > 0.f ? d : 0.f;
  return d;
}

// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

}  // namespace ap

#include "ap_reduce.h"   // the fixed-order sums of the non-block kernels
