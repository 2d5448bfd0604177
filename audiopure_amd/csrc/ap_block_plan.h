// The WaveNet residual block's dispatch as a pure function: which kernel serves one launch, in which instantiation, on which grid --
// and the same for the skip GEMM and the final conv.  Host-only (no HIP header, plain g++ -std=c++17 compiles it), so the rule under
// the headline number is pinned on the CPU: tests/test_block_plan_cpu.py against tests/golden/block_dispatch_v1.json.  launch_resblock
// and launch_resblock_bf16u fill a BlockAsk, ask block_plan and switch on the family; run_net asks block_drops_last_h.
#pragma once
#include <stddef.h>
#include "../../include/audiopure.h"

namespace ap {
// ---- tile sizes the plan and the kernels share (the kernel files name them locally: PT_, NP_, ...) ----
constexpr int BLOCK_PT = 128;      // bf16 persistent blocks, fp32 tensor and u image: samples per tile
constexpr int BLOCK_ST = 64;       // bf16 small-tile blocks: samples per tile (*)
constexpr int BLOCK_NP = 32;       // fp32 F(2,3) block: output pairs per tile
constexpr int BLOCK_NPT = 64;      // split F(2,3), gate launch: output pairs per tile
constexpr int BLOCK_BT = 128;      // split direct block: samples per tile
constexpr int BLOCK_BT2 = 128;     // split F(2,3), output launch: samples per tile
constexpr int BLOCK_SPT = 128;     // skip GEMM: samples per tile
constexpr int BLOCK_FT = 64;       // final conv at 256 skip channels, fp32 and bf16: samples per tile (*)
constexpr int BLOCK_TT = 128;      // final conv at 64 / 128 skip channels (the fused kernels' time tile)
constexpr size_t BLOCK_FACTOR_TILE_BYTES = 131072;   // gate factors (SAVEF): 128 KB per 128-sample tile (ap_gate_factor_bytes) (*)
// (*) a second copy, and not tied by a static_assert: resblock_bf16s_kernel / resblock_bf16us_kernel (NT = 64), final_bf16_kernel (FT = 64)
// and the SAVEF stores hold these numbers as locals inside __global__ functions, where no file-scope name reaches them
// the small-tile kernels take launches of at most one 128-sample tile per CU of a 256-CU device: their duration on the persistent
// kernel is one tile's latency (a constant, not the device's CU count: the threshold was swept on the MI355X)
constexpr long long BLOCK_SMALL_MAX_TILES = 256;
inline bool block_is_small(int B, int L) { return (long long)B * ((L + BLOCK_PT - 1) / BLOCK_PT) <= BLOCK_SMALL_MAX_TILES; }

// ---- the 2^31 limits: buffer descriptors carry 32-bit byte ranges, and offset 0x80000000 is the out-of-clip sentinel ----
constexpr size_t BLOCK_2G = (size_t)1 << 31;
inline bool g_image_fits(int L) { return (size_t)L * 512 < BLOCK_2G; }                    // a clip's bf16 g / u image, [L][256]
inline bool skip_rows_fit(int L) { return (size_t)L * 1024 < BLOCK_2G; }                  // a clip's 256 fp32 rows
inline bool pre_gate_rows_fit(int L) { return (size_t)2 * 256 * (size_t)L * 4 < BLOCK_2G; }   // the SAVE form's 2C fp32 rows per clip
inline bool factor_image_fits(long long ntiles) { return (size_t)ntiles * BLOCK_FACTOR_TILE_BYTES < BLOCK_2G; }
inline bool tile_count_fits(long long n) { return n < (1ll << 31); }

// switches of the -DAP_TOOLS build (ap_debug_*), constexpr defaults in the product build
struct BlockTune {
  int tile = 64;          // ap_debug_tile: time tile of the direct fp32 block, 64 (4 waves, 2 WG/CU) or 128 (8 waves, 1 WG/CU)
  int force_direct = 0;   // the direct-form fp32 block even where the minimal-filtering one is built
  int no_bf16s = 0;       // ap_debug_no_bf16s: 1 = small deferred-skip launches stay on the persistent kernel, 2 = all on the small-tile one
  int force_f32 = 0;      // ap_debug_force_f32: the fp32 kernel even in a bf16 context (A/B timing in one process)
  int no_bf16us = 0;      // ap_debug_no_bf16us: as no_bf16s, for the u-image interface
  int no_q16 = 0;         // ap_debug_f32w_q16(0): the 4-byte epilogue for every clip length
  int diet = -1;          // ap_debug_f32w_diet(mask): the h'-writing 16-byte F(2,3) block with another DIET mask (-1: the product's)
};

struct BlockAsk {
  int precision, C, S, NL, cycle, f32_form;   // of the context (cycle: dilation_cycle)
  bool w1w, w1w_s, w2p_bf, wf1p_bf;           // which weight images exist
  int layer, B, L, n_cu;                      // n_cu: CUs of the launching device (the launcher passes the context's count)
  bool hout, skip, aout, gout, fout;          // outputs asked for: h' (u' on the u-image interface), skip, pre-gate save, g image, gate factors
  bool u;                                     // the u-image interface (ap_resblock_fwd_u / _u_save) calls, not the fp32-tensor one
};

enum BlockFamily {
  BLOCK_F32_DIRECT,     // ap_kernels.hip resblock_f32_kernel<C, tile, SAVE>
  BLOCK_F32_F23,        // ap_resblock_f32w.hip resblock_f32w_kernel<NOH, SAVE, Q16, DIET, DCLS>, persistent
  BLOCK_SPLIT_DIRECT,   // ap_resblock_f32s.hip resblock_f32s_kernel<256, E4>
  BLOCK_SPLIT_F23,      // ap_resblock_f32s2.hip f32s_gate_kernel, then f32s_out_kernel
  BLOCK_BF16_P,         // ap_resblock_bf16p.hip resblock_bf16p_kernel<WS, RAG, DS, NOH, SAVEF>, persistent
  BLOCK_BF16_S,         // ap_resblock_bf16s.hip resblock_bf16s_kernel<NOH>
  BLOCK_BF16U_P,        // ap_resblock_bf16u.hip resblock_bf16u_kernel<NOH, SAVEF>, persistent
  BLOCK_BF16U_S,        // ap_resblock_bf16us.hip resblock_bf16us_kernel<NOH>
  BLOCK_SKIPGEMM,       // skipgemm_plan: ap_skipgemm_bf16.hip skipgemm_bf16_kernel<RAG>, persistent
  BLOCK_FINAL_BF16, BLOCK_FINAL_F32   // final_plan: ap_kernels.hip final_bf16_kernel / final_f32_kernel<S, tile>
};

struct BlockPlan {
  int family;
  int tile;                     // samples per tile (F(2,3) families: 2 x pairs)
  bool save, noh;               // SAVE: + the pre-gate rows; NOH: the net's last layer, no res_conv and no h' / u'
  bool q16;                     // BLOCK_F32_F23: the 16-byte epilogue form (L % 4 == 0)
  int dcls, diet;               //   its quad dilation class (1: d = 1, 2: d = 2, 4: the rest; used where the mask stages by quads) and DIET mask (-1: the product's)
  int ws;                       // BLOCK_BF16_P: staging form, 1 / 2 = one window at d = 1 / 2, 0 = one window at d = 4 .. 32, -1 = three tap loads
  bool rag, ds, savef;          //   ragged clip length (L % 4); deferred skip (g image out, no skip GEMM); + the gate's derivative factors (also BLOCK_BF16U_P)
  bool e4;                      // BLOCK_SPLIT_DIRECT: the aligned form (L % 4 == 0 and L >= 4)
  int d, logd;                  // the layer's dilation
  long long np;                 // F(2,3) families: output pairs whose first output is inside the clip
  int ntiles, ntiles2;          // tiles per clip (2: the second launch of BLOCK_SPLIT_F23)
  long long nblk, nblk2;        // tiles of the launch
  unsigned grid, grid2, wg;     // workgroups per launch, threads per workgroup
  const char *err;              // where block_plan returns non-zero: set_error's format and its arguments
  int err_arg[4];
};

struct BlockPlanSlot { int key = -1, B = 0, L = 0; BlockPlan plan; };   // one kept plan of a context (ap_common.h planned_block)

inline int block_refuse(BlockPlan *p, const char *err, int a = 0, int b = 0, int c = 0, int d = 0, int rc = -22) {
  p->err = err; p->err_arg[0] = a; p->err_arg[1] = b; p->err_arg[2] = c; p->err_arg[3] = d;
  return rc;
}
// grid of the persistent bf16 blocks: one workgroup per CU, whole groups of 8 (one per XCD) from 8 on
inline unsigned block_grid8(long long nblk, int n_cu) {
  long long g = nblk < n_cu ? nblk : n_cu;
  if (g >= 8) g &= ~7ll;
  return (unsigned)g;
}
// F(2,3) along time at dilation d: pairs (t, t + d) whose first output is inside the clip
inline long long block_pairs(int L, int logd) {
  const long long d = 1ll << logd, r = L % (2 * d);
  return (L / (2 * d)) * d + (r < d ? r : d);
}
// which contexts and shapes the two F(2,3) blocks and the u-image block are built for, as views of the ask (ap_init_conv_u and the
// tools build read them too)
inline bool block_f32w_serves(const BlockAsk &a) {
  if (a.precision != AP_PREC_F32 || a.f32_form != 1 || a.C != 256 || a.S != 256 || !a.w1w) return false;
  return pre_gate_rows_fit(a.L) && tile_count_fits((long long)a.B * ((a.L + 2 * BLOCK_NP - 1) / (2 * BLOCK_NP) + 1));
}
inline bool block_split23_serves(const BlockAsk &a) {
  if (a.precision != AP_PREC_F32_SPLIT || a.C != 256 || a.S != 256 || a.f32_form != 1 || !a.w1w_s) return false;
  return skip_rows_fit(a.L) && tile_count_fits((long long)a.B * ((a.L + BLOCK_NPT - 1) / BLOCK_NPT + 2) * 2);
}
inline bool block_bf16u_serves(const BlockAsk &a) { return a.precision == AP_PREC_BF16_STORE && a.C == 256 && a.S == 256 && a.L >= 1 && g_image_fits(a.L); }

// The whole decision.  0: launch what *p says; otherwise the return code of the refusal (-22) with p->err set.
inline int block_plan(const BlockAsk &a, const BlockTune &t, BlockPlan *p) {
  *p = BlockPlan{};
  p->diet = -1; p->wg = 512;
  p->logd = a.layer % a.cycle; p->d = 1 << p->logd;
  const int B = a.B, L = a.L;
  const bool c256 = a.C == 256 && a.S == 256;
  // one launch of B x ceil(L / tile) tiles, one workgroup each unless the caller caps the grid.  (The kernels take the tile count as
  // an int and the direct-form launchers multiplied in 32 bits: past 2^31 tiles -- tensors beyond any device's memory -- a launch
  // used to fail with a zero or wrapped grid; it is refused here.)
  const auto tiles = [&](int family, int tile, const char *many = "resblock: too many tiles (B x tiles per clip must stay below 2^31)") {
    p->family = family; p->tile = tile; p->ntiles = (L + tile - 1) / tile;
    p->nblk = (long long)B * p->ntiles; p->grid = (unsigned)p->nblk;
    return tile_count_fits(p->nblk) ? 0 : block_refuse(p, many);
  };
  if (a.u) {                                                    // ---- AP_PREC_BF16_STORE: the residual stream as bf16 u images
    if (!block_bf16u_serves(a))
      return block_refuse(p, "AP_PREC_BF16_STORE: built for res = skip = 256 channels, clips shorter than 2^22 samples (got %d / %d, L = %d)", a.C, a.S, L);
    p->ds = true; p->noh = !a.hout; p->savef = a.fout;
    // at most one tile per CU (one- and two-clip calls): 64-sample tiles on twice as many workgroups, bit-identical results.  (This
    // kernel asks L * 512 < 2^31, which the refusal above has settled; its fp32-tensor sibling below asks L * 1024: kept as found.)
    if (!a.fout && t.no_bf16us != 1 && g_image_fits(L) && (t.no_bf16us == 2 || block_is_small(B, L))) {
      return tiles(BLOCK_BF16U_S, BLOCK_ST, "AP_PREC_BF16_STORE: too many tiles");
    }
    if (int e = tiles(BLOCK_BF16U_P, BLOCK_PT)) return e;
    p->grid = block_grid8(p->nblk, a.n_cu);
    if (a.fout && !factor_image_fits(p->ntiles)) return block_refuse(p, "AP_PREC_BF16_STORE: clip too long for the gate-factor image");
    return 0;
  }
  if (a.aout && a.precision != AP_PREC_F32)
    return block_refuse(p, "ap_resblock_fwd_save: AP_PREC_F32 only (the other modes recompute the pre-gate activations)");
  if (a.precision == AP_PREC_BF16_STORE)
    return block_refuse(p, "AP_PREC_BF16_STORE: the residual stream is a bf16 image in this mode (ap_init_conv_u / ap_resblock_fwd_u), not an fp32 tensor; "
                           "the fp32-tensor block serves AP_PREC_F32, AP_PREC_F32_SPLIT and AP_PREC_BF16");
  if (a.gout && (a.precision != AP_PREC_BF16 || t.force_f32)) return block_refuse(p, "deferred-skip form: AP_PREC_BF16 only");
  if (a.precision == AP_PREC_BF16 && !t.force_f32) {            // ---- AP_PREC_BF16
    // small deferred-skip launches: half-size tiles, bit-identical (tools: no_bf16s = 2 lifts the tile rule only)
    if (a.gout && !a.fout && t.no_bf16s != 1 && c256 && skip_rows_fit(L) && (t.no_bf16s == 2 || block_is_small(B, L))) {
      p->ds = true; p->noh = !a.hout;
      return tiles(BLOCK_BF16_S, BLOCK_ST);
    }
    if (!c256) return block_refuse(p, "AP_PREC_BF16 is built for res_channels = skip_channels = 256 only (got %d / %d)", a.C, a.S);
    if (int e = tiles(BLOCK_BF16_P, BLOCK_PT)) return e;
    p->grid = block_grid8(p->nblk, a.n_cu);
    p->rag = L % 4 != 0;
    // staging form: one window for the three taps where they overlap (d <= 32), else three tap loads; d = 4 .. 32 ragged: the
    // three-tap form, one instantiation fewer
    p->ws = p->d == 1 ? 1 : p->d == 2 ? 2 : (p->d <= 32 && !p->rag) ? 0 : -1;
    if (a.gout) {                                               // deferred skip; + no h' -> NOH, + factors -> SAVEF
      if (!g_image_fits(L)) return block_refuse(p, "AP_PREC_BF16: clip too long for the bf16 g image");
      if (a.fout && !factor_image_fits(p->ntiles)) return block_refuse(p, "AP_PREC_BF16: clip too long for the gate-factor image");
      p->ds = true; p->noh = !a.hout; p->savef = a.fout;
    }
    return 0;
  }
  if (a.precision != AP_PREC_F32 && !t.force_f32) {             // ---- AP_PREC_F32_SPLIT
    if (!c256) return block_refuse(p, "AP_PREC_F32_SPLIT is built for res_channels = skip_channels = 256 only (got %d, %d)", a.C, a.S);
    if (a.hout && block_split23_serves(a)) {                    // the dilated conv in F(2,3) form where built and selected: two launches
      p->family = BLOCK_SPLIT_F23; p->tile = 2 * BLOCK_NPT;
      p->np = block_pairs(L, p->logd);
      p->ntiles = (int)((p->np + BLOCK_NPT - 1) / BLOCK_NPT); p->nblk = (long long)B * p->ntiles * 2;
      p->ntiles2 = (L + BLOCK_BT2 - 1) / BLOCK_BT2; p->nblk2 = (long long)B * p->ntiles2;
      p->grid = (unsigned)p->nblk; p->grid2 = (unsigned)p->nblk2;
      return 0;
    }
    p->e4 = L % 4 == 0 && L >= 4;
    return tiles(BLOCK_SPLIT_DIRECT, BLOCK_BT);
  }
  // ---- AP_PREC_F32
  if (!t.force_direct && block_f32w_serves(a)) {                // F(2,3) form of the dilated conv
    p->family = BLOCK_F32_F23; p->tile = 2 * BLOCK_NP; p->wg = 256;
    p->np = block_pairs(L, p->logd);
    p->ntiles = (int)((p->np + BLOCK_NP - 1) / BLOCK_NP); p->nblk = (long long)B * p->ntiles;
    if (!tile_count_fits(p->nblk)) return block_refuse(p, "resblock: too many tiles for the minimal-filtering block", 0, 0, 0, 0, 1);   // (1, as found)
    p->grid = (unsigned)(p->nblk < a.n_cu ? p->nblk : a.n_cu);
    if (a.aout && !a.hout) return block_refuse(p, "resblock (save): needs an h' buffer");
    p->q16 = (L & 3) == 0 && !t.no_q16;
    p->save = a.aout; p->noh = !a.hout;
    p->dcls = p->q16 ? (p->logd == 0 ? 1 : p->logd == 1 ? 2 : 4) : 4;
    if (p->q16 && a.hout && !a.aout) p->diet = t.diet;          // (every other form keeps the product's mask; the 4-byte form has none)
    return 0;
  }
  if (!a.hout) return block_refuse(p, "resblock: the direct-form block needs an h' buffer");
  if (a.aout ? (a.C != 64 && a.C != 256) : (a.C != 64 && a.C != 128 && a.C != 256))
    return block_refuse(p, a.aout ? "resblock (save): unsupported res_channels %d (need 64 or 256)" : "resblock: unsupported res_channels %d (need 64, 128 or 256)", a.C);
  p->save = a.aout;
  if (int e = tiles(BLOCK_F32_DIRECT, (t.tile == 64 || (a.aout && a.C == 64)) ? 64 : 128)) return e;   // (SAVE at 64 channels: 64-sample tiles only)
  p->wg = (unsigned)(a.C / 64 * p->tile);
  return 0;
}

// run_net: the last layer's h' is never read (the net returns the skip sum only), so it is dropped where the launch has a form
// without res_conv and its store
inline bool block_drops_last_h(BlockAsk a, const BlockTune &t) {
  BlockPlan p;
  a.layer = a.NL - 1; a.hout = false;
  return block_plan(a, t, &p) == 0 && p.noh;
}

// ---- the skip GEMM of the deferred-skip form: ragged or not (L % 4), one workgroup per CU (not rounded to groups of 8) ----
inline int skipgemm_plan(const BlockAsk &a, int layer0, int nl, BlockPlan *p) {
  *p = BlockPlan{};
  if (a.C != 256 || a.S != 256 || !a.w2p_bf) return block_refuse(p, "skip GEMM: AP_PREC_BF16 context with res = skip = 256 channels only");
  if (nl < 1 || layer0 < 0 || layer0 + nl > a.NL || a.B < 1 || a.L < 1) return block_refuse(p, "skip GEMM: layers [%d, %d) B=%d L=%d", layer0, layer0 + nl, a.B, a.L);
  // (a clip's fp32 skip rows: the out-of-clip sentinel offset 0x80000000 of the epilogue must lie beyond them)
  if (!skip_rows_fit(a.L)) return block_refuse(p, "skip GEMM: clip too long (L * 1024 bytes of skip rows per clip must stay below 2^31)");
  p->family = BLOCK_SKIPGEMM; p->tile = BLOCK_SPT; p->rag = a.L % 4 != 0; p->wg = 512;
  p->ntiles = (a.L + BLOCK_SPT - 1) / BLOCK_SPT; p->nblk = (long long)a.B * p->ntiles;
  p->grid = (unsigned)(p->nblk < a.n_cu ? p->nblk : a.n_cu);
  return 0;
}

// ---- final_conv + clip update: the bf16-operand kernel in the bf16 modes at 256 skip channels, else the fp32 kernel of S channels ----
inline int final_plan(const BlockAsk &a, BlockPlan *p) {
  *p = BlockPlan{};
  const bool bf16 = (a.precision == AP_PREC_BF16 || a.precision == AP_PREC_BF16_STORE) && a.S == 256 && a.wf1p_bf;
  if (!bf16 && a.S != 64 && a.S != 128 && a.S != 256) return block_refuse(p, "final: unsupported skip_channels %d", a.S);
  p->family = bf16 ? BLOCK_FINAL_BF16 : BLOCK_FINAL_F32;
  p->tile = a.S == 256 ? BLOCK_FT : BLOCK_TT;                   // 64 columns at S = 256: two workgroups share a CU
  p->ntiles = (a.L + p->tile - 1) / p->tile; p->nblk = (long long)a.B * p->ntiles;
  p->grid = (unsigned)p->nblk; p->wg = (unsigned)a.S;
  return 0;
}

}  // namespace ap
