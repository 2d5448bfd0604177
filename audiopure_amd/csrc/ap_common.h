// Shared declarations for the gfx950 kernels and the C-ABI (include/audiopure.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>

#include "../../include/audiopure.h"
#include "ap_block_plan.h"   // the residual block's dispatch rule and the tile sizes it shares with the kernels (host-only)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace ap {

void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what);

#define AP_HIP(x)                                  \
  do {                                             \
    hipError_t _e = (x);                           \
    if (_e != hipSuccess) return ap::hip_fail(_e, #x); \
  } while (0)

// CU count of the calling thread's current HIP device (the persistent kernels launch one workgroup per CU).  One table entry per
// device: a process may drive several devices, and their CU counts / partition modes may differ.  A racing first call writes the
// same value twice.
inline int device_cu_count() {
  static int n_cu_of[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (n_cu_of[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8) n = 256;
    n_cu_of[dev] = n;
  }
  return n_cu_of[dev];
}

// Timing-only hooks (ablation masks, phase stamps, dispatch overrides: tools/*.py) exist only in a -DAP_TOOLS build
// (`python __graft_entry__.py --tools` -> tools/lib/libaudiopure_hip_tools.so).  The shipped library has no `ablate` kernel
// argument, no ap_debug_* symbol and no stamped instantiation.
#ifdef AP_TOOLS
#define AP_ABLATE_PARAM , int ablate
#define AP_ABLATE_ARG(x) , (x)
#define AP_ABLATE_DECL
extern BlockTune g_block_tune;   // (ap_kernels.hip) the one set of block-dispatch switches the ap_debug_* hooks write
constexpr bool g_keep_plans = false;   // (the switches move under a context: plan every time)
#else
#define AP_ABLATE_PARAM
#define AP_ABLATE_ARG(x)
#define AP_ABLATE_DECL constexpr int ablate = 0;
constexpr BlockTune g_block_tune{};
constexpr bool g_keep_plans = true;
#endif

constexpr int TT = BLOCK_TT;   // time-tile (samples) of the fused kernels
constexpr int KC = 32;    // channels per staged K-chunk of the dilated conv (x3 taps = 96 K rows)

// Offsets (in floats) of the reference state-dict tensors inside the weight blob.
struct BlobLayout {
  size_t init_b, init_g, init_v;
  size_t fc1_w, fc1_b, fc2_w, fc2_b;
  size_t blk0, blk_stride;
  // inside a block
  size_t fct_w, fct_b, dil_b, dil_g, dil_v, res_b, res_g, res_v, skip_b, skip_g, skip_v;
  size_t f1_b, f1_g, f1_v, f2_w, f2_b;
  size_t total;
};
BlobLayout blob_layout(const ap_config &c);

}  // namespace ap

struct ap_ctx {
  ap_config cfg;
  int C, S, NL, NW;
  bool loaded;
  // schedule (host), reference: util.py:96-123 and diffwave_sde.py:56-60
  std::vector<float> Beta, Alpha, Alpha_bar, Sigma;
  std::vector<float> sde_beta, sde_ac;
  // device weights
  float *slab;            // one allocation holding everything below
  size_t slab_elems;
  float *emb_freq;        // [Ein/2]
  float *fc1_w, *fc1_b, *fc2_w, *fc2_b;
  float *fct_w, *fct_b;   // [NL][C][Eout], [NL][C]
  float *w0, *b0;         // folded init conv [C], bias [C]
  float *w1f;             // [NL][2C][C][3] folded
  float *w2f;             // [NL][C+S][C] folded (res rows then skip rows)
  float *wf1f;            // [S][S] folded
  float *b1;              // [NL][2C]
  float *b2;              // [NL][C+S]
  float *bf1, *wf2, *bf2; // [S], [S], [1]
  float *w1p, *w2p, *wf1p;  // packed fp32 MFMA A-operand images
  void *w1p_bf, *w2p_bf;    // packed bf16 images (AP_PREC_BF16), own allocation
  void *wf1p_bf;            // final conv's first 1x1 as a bf16 image (same allocation)
  void *slab_bf;
  void *w1p_s, *w2p_s;      // 3-way bf16-split images (AP_PREC_F32_SPLIT), own allocation
  void *w1w_s;              // ... and the F(2,3)-transformed, 3-way-split GEMM1 image of ap_resblock_f32s2.hip (same allocation)
  void *slab_s;
  float *w1w, *w2w;         // AP_PREC_F32, C = S = 256: F(2,3)-transformed GEMM1 image and GEMM2 image of ap_resblock_f32w.hip, own allocation
  void *slab_w;
  float *w2t, *w1b;         // backward images of ap_resblock_bwd.hip (ap_ctx_prepare_backward), own allocation
  void *slab_b;
  void *slab_bb;            // bf16 backward images of ap_resblock_bwd_bf16.hip (ap_ctx_prepare_backward)
  bool bwd_ready;           // the backward images of this context's precision are built from the weights now loaded
  int f32_form;             // AP_PREC_F32 / AP_PREC_F32_SPLIT: 1 = minimal-filtering (F(2,3)) block where built (default), 0 = direct-form block
  float *norms;           // scratch for row norms
  // optional per-launch timing of the residual-block kernel (bench.py roofline leg)
  bool profile;
  std::vector<hipEvent_t> ev;   // pairs (start, stop), one pair per launch since the last reset
  std::vector<char> ev_kind;    // per pair: 0 residual-block launch, 1 skip-GEMM launch of the deferred-skip form
  size_t ev_used;
  int skip_group;               // AP_PREC_BF16: layers per skip GEMM of the deferred-skip form (0: fused block, skip per layer)
  int n_cu;                     // CUs of the device the weights were loaded on (ap_ctx_load_wavenet): what the block plans read, not a runtime call per launch
  std::vector<ap::BlockPlanSlot> plans;   // [NL][4] kept block plans (planned_block); with drop_*: emptied by forget_plans
  int drop_B, drop_L, drop_defer;         // run_net's last (B, L, deferred skip?) and whether the last layer then drops h'
  bool drop_last;
};

namespace ap {
// One launch's (start, stop) event pair for ap_profile_read / ap_profile_read_split (bench.py's roofline leg).  Events are created
// lazily and reused after a reset, one pair per launch; with ctx->profile off nothing is taken and nothing recorded.
struct ProfileSpan {
  hipEvent_t stop = nullptr;
  hipStream_t st = nullptr;
  int begin(ap_ctx *ctx, int kind, hipStream_t stream) {        // kind: ap_ctx::ev_kind
    if (!ctx->profile) return 0;
    if (ctx->ev_used + 2 > ctx->ev.size())
      for (int i = 0; i < 2; i++) {
        hipEvent_t e;
        AP_HIP(hipEventCreate(&e));
        ctx->ev.push_back(e);
      }
    const hipEvent_t start = ctx->ev[ctx->ev_used];
    stop = ctx->ev[ctx->ev_used + 1];
    st = stream;
    if (ctx->ev_kind.size() < ctx->ev.size() / 2) ctx->ev_kind.resize(ctx->ev.size() / 2, 0);
    ctx->ev_kind[ctx->ev_used / 2] = (char)kind;
    ctx->ev_used += 2;
    AP_HIP(hipEventRecord(start, st));
    return 0;
  }
  int end() {
    if (stop) AP_HIP(hipEventRecord(stop, st));
    return 0;
  }
};

// What block_plan reads, from a context and one call's arguments (hout: u' on the u-image interface)
inline BlockAsk block_ask(const ap_ctx *ctx, int layer, int B, int L, bool hout = true, bool skip = true, bool aout = false, bool gout = false,
                          bool fout = false, bool u = false) {
  return BlockAsk{ctx->cfg.precision, ctx->C, ctx->S, ctx->NL, ctx->cfg.dilation_cycle, ctx->f32_form, ctx->w1w != nullptr, ctx->w1w_s != nullptr,
                  ctx->w2p_bf != nullptr, ctx->wf1p_bf != nullptr, layer, B, L, ctx->n_cu, hout, skip, aout, gout, fout, u};
}
// a launcher's first step: the plan's return code, with the refusal's text set
inline int plan_refused(int rc, const BlockPlan &p) {
  if (rc) set_error(p.err, p.err_arg[0], p.err_arg[1], p.err_arg[2], p.err_arg[3]);
  return rc;
}
// The plan of one block launch (rc: 0, or the refusal's code with its text set).  Kept in the context per (layer, h' asked, save asked)
// and reused while the outputs asked, B and L repeat: a chain launches the same shapes step after step.  Refusals are not kept.
// forget_plans: on reload and on an f32_form change.  The tools build, whose switches move under a context, plans every time.
inline void forget_plans(ap_ctx *ctx) { ctx->plans.clear(); ctx->drop_B = 0; }
inline const BlockPlan &planned_block(ap_ctx *ctx, int layer, int B, int L, bool hout, bool skip, bool aout, bool gout, bool fout, bool u, int *rc) {
  const int key = hout | skip << 1 | aout << 2 | gout << 3 | fout << 4 | u << 5;
  if (ctx->plans.empty()) ctx->plans.resize((size_t)ctx->NL * 4);
  BlockPlanSlot &s = ctx->plans[(size_t)layer * 4 + (hout | (aout || fout) << 1)];
  if (g_keep_plans && s.key == key && s.B == B && s.L == L) { *rc = 0; return s.plan; }
  *rc = plan_refused(block_plan(block_ask(ctx, layer, B, L, hout, skip, aout, gout, fout, u), g_block_tune, &s.plan), s.plan);
  s.key = *rc ? -1 : key; s.B = B; s.L = L;
  return s.plan;
}
// bf16 persistent blocks: one buffer descriptor per parameter slab (the bf16 images; the fp32 biases), a layer's tensors at byte offsets
struct BlockSlabs {
  const char *wlo; unsigned wbytes, w1_off, w2_off;
  const float *blo; unsigned bbytes, b1_off, b2_off;
};
inline BlockSlabs block_slabs(const ap_ctx *ctx, int layer) {
  const int C = ctx->C, S = ctx->S;
  const size_t n1 = (size_t)2 * C * C * 3, n2 = (size_t)(C + S) * C;
  const char *w1 = (const char *)ctx->w1p_bf, *w2 = (const char *)ctx->w2p_bf;
  const float *blo = ctx->b1 < ctx->b2 ? ctx->b1 : ctx->b2, *bhi = ctx->b1 < ctx->b2 ? ctx->b2 : ctx->b1;
  BlockSlabs s{w1 < w2 ? w1 : w2, 0, 0, 0, blo, 0, 0, 0};
  s.w1_off = (unsigned)(w1 - s.wlo + layer * n1 * 2);
  s.w2_off = (unsigned)(w2 - s.wlo + layer * n2 * 2);
  s.wbytes = (unsigned)(((size_t)ctx->NL * (n1 + n2) + (size_t)S * S) * 2);   // the whole bf16 slab
  s.b1_off = (unsigned)((ctx->b1 - blo + (size_t)layer * 2 * C) * 4);
  s.b2_off = (unsigned)((ctx->b2 - blo + (size_t)layer * (C + S)) * 4);
  s.bbytes = (unsigned)((bhi - blo + (size_t)ctx->NL * 2 * C) * 4);
  return s;
}

// What every block entry point of the C-ABI checks first (`who` is its name): the context is loaded and no required pointer is
// null (`ptrs`), layer and shape are in range, the output does not alias the input.  0, or -22 with the error text set.
inline int check_block_args(const char *who, const ap_ctx *ctx, bool ptrs, int layer, int B, int L, const void *in, const char *in_name,
                            const void *out, const char *out_name) {
  if (!ctx || !ctx->loaded || !ptrs) { set_error("%s: not loaded / null", who); return -22; }
  if (layer < 0 || layer >= ctx->NL || B < 1 || L < 1) { set_error("%s: layer=%d B=%d L=%d", who, layer, B, L); return -22; }
  if (in == out) { set_error("%s: %s must not alias %s", who, out_name, in_name); return -22; }
  return 0;
}
}  // namespace ap

struct ap_m5 {
  int n_output, n_channel, k1, stride;
  float eps;              // BatchNorm eps as given to ap_m5_create (the train-mode launchers read it; the eval images have it folded in)
  float *slab;
  float *w[4], *b[4];
  float *fcw, *fcb;
};

#ifdef __HIPCC__
#include "ap_device.h"   // what only kernels need
#endif

// kernel launchers (defined in the .hip files)
namespace ap {
int launch_fold_and_pack(ap_ctx *ctx, const float *blob, hipStream_t st);
int launch_embed(ap_ctx *ctx, float step, float *part_t, hipStream_t st);
int launch_init_conv(ap_ctx *ctx, const float *x, float *h, int B, int L, hipStream_t st);
int launch_resblock(ap_ctx *ctx, int layer, const float *hin, const float *pt, float *hout, float *skip,
                    int accumulate, int B, int L, hipStream_t st, float *aout = nullptr, void *gout = nullptr, void *fout = nullptr);
int launch_final_affine(ap_ctx *ctx, const float *skip, const float *x, float *eps_out, float *out, float ca,
                        float cb, float cs, const float *z, uint64_t seed, uint32_t draw, uint64_t utt_offset,
                        int B, int L, hipStream_t st);
int launch_affine_noise(const float *x, float *out, float ca, float cs, const float *z, uint64_t seed,
                        uint32_t draw, uint64_t utt_offset, int B, int L, hipStream_t st);
int launch_pack_bf16(ap_ctx *ctx, hipStream_t st);
// The residual block: launch_resblock (fp32 tensors) and launch_resblock_bf16u (bf16 u images, AP_PREC_BF16_STORE; uout null: the net's
// last layer) plan (ap_block_plan.h), time the launch (profile kind 0) and switch on the family; launch_block_* are the families' leaves.
// `gout` non-null: the deferred-skip form -- the block writes h' and its gate output as a bf16 image [clip][L][256] to gout and leaves
// `skip` alone (launch_skipgemm_bf16 adds a group of layers' skip_conv outputs in one GEMM); fout: + the gate's derivative factors
int launch_resblock_bf16u(ap_ctx *ctx, int layer, const void *uin, const float *pt_next, void *uout, void *gout, int B, int L, hipStream_t st,
                          void *fout = nullptr);
int launch_block_f32w(ap_ctx *ctx, const BlockPlan &p, int layer, const float *hin, const float *pt, float *hout, float *skip, int accumulate, int L,
                      hipStream_t st, float *aout);
int launch_block_split(ap_ctx *ctx, const BlockPlan &p, int layer, const float *hin, const float *pt, float *hout, float *skip, int accumulate, int L,
                       hipStream_t st);
int launch_block_split23(ap_ctx *ctx, const BlockPlan &p, int layer, const float *hin, const float *pt, float *hout, float *skip, int accumulate, int L,
                         hipStream_t st);
int launch_block_bf16p(ap_ctx *ctx, const BlockPlan &p, int layer, const float *hin, const float *pt, float *hout, float *skip, int accumulate, int L,
                       hipStream_t st, void *gout, void *fout);
int launch_block_bf16s(ap_ctx *ctx, const BlockPlan &p, int layer, const float *hin, const float *pt, float *hout, void *gout, int L, hipStream_t st);
int launch_block_bf16us(ap_ctx *ctx, const BlockPlan &p, int layer, const void *uin, const float *pt_next, void *uout, void *gout, int L, hipStream_t st);
int launch_init_conv_u(ap_ctx *ctx, const float *x, const float *pt0, void *u, int B, int L, hipStream_t st);
int launch_skipgemm_bf16(ap_ctx *ctx, int layer0, int nl, const void *gimg, float *skip, int accumulate, int B, int L, hipStream_t st);
int launch_pack_f32w(ap_ctx *ctx, hipStream_t st);
int launch_pack_split(ap_ctx *ctx, hipStream_t st);
int launch_pack_split23(ap_ctx *ctx, hipStream_t st);            // ap_resblock_f32s2.hip: AP_PREC_F32_SPLIT with the dilated conv in F(2,3) form
int prepare_bwd_f32(ap_ctx *ctx, hipStream_t st);                // ap_ctx_prepare_backward, per precision (allocate + pack + synchronise)
int prepare_bwd_bf16(ap_ctx *ctx, hipStream_t st);
// ap_conv_w3.hip: 3 x 3 / stride 1 / pad 1 / ungrouped layers in F(2,3) form along W (which layers: ap_conv_plan.h)
int launch_conv_pack_w3(const float *w, const float *scale, float *out, int Cout, int Cin, hipStream_t st);
int launch_conv_w3(const float *x, const float *wimg, const float *bias, const float *res, float *out, int B, int Cin, int H, int W,
                   int Cout, int relu, int x_cstride, int x_coff, int o_cstride, int o_coff, hipStream_t st, int splits = 1, float *part = nullptr);
#ifdef AP_TOOLS
// tools/csrc/ap_conv_p1.hip (tools library only): pointwise layers of the high-resolution maps as an LDS-free streaming GEMM on the
// family's A-fragment image -- round 6's attempt at VERDICT r5 item 5a, measured slower than the 128 x 64 tiles (profiles/r6_conv_pointwise_streaming_ab.txt)
bool conv_p1_serves(int B, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int groups);
int launch_conv_p1(const float *x, const float *afrag, const float *bias, const float *res, float *out, int B, int Cin, int H, int W, int Cout,
                   int relu, int x_cstride, int x_coff, int o_cstride, int o_coff, size_t abytes, hipStream_t st);   // 1: not served (tensor too large)
#endif
int launch_m5(ap_m5 *m, const float *x, float *logprobs, int B, int L, hipStream_t st);
int launch_m5_bwd(ap_m5 *m, const float *x, const float *dlogp, float *dx, int B, int L, hipStream_t st);
int launch_m5_fold(ap_m5 *m, const float *blob, float bn_eps, hipStream_t st);
// ap_m5_train.hip: train-mode M5 (batch-statistics BatchNorm), forward and the parameter / input gradients
size_t m5_train_workspace_bytes(const ap_m5 *m, int B, int L);   // 0 with the error text set where the shape is refused
int launch_m5_train_fwd(ap_m5 *m, const float *blob, const float *x, float *logprobs, float *new_running, float momentum, void *ws,
                        size_t ws_bytes, int keep, int B, int L, hipStream_t st);
int launch_m5_train_bwd(ap_m5 *m, const float *blob, const float *x, const float *dlogp, float *grads, float *dx, void *ws, size_t ws_bytes,
                        int B, int L, hipStream_t st);
}  // namespace ap
