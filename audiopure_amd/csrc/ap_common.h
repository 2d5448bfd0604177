// Shared declarations for the gfx950 kernels and the C-ABI (include/audiopure.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>

#include "../../include/audiopure.h"

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
#define AP_TOOLS_VAR static int
#else
#define AP_ABLATE_PARAM
#define AP_ABLATE_ARG(x)
#define AP_ABLATE_DECL constexpr int ablate = 0;
#define AP_TOOLS_VAR static constexpr int
#endif

constexpr int TT = 128;   // time-tile (samples) of the fused kernels
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
int launch_final_affine_bf16(ap_ctx *ctx, const float *skip, const float *x, float *eps_out, float *out, float ca, float cb,
                             float cs, const float *z, uint64_t seed, uint32_t draw, uint64_t utt_offset, int B, int L,
                             hipStream_t st);                    // returns 1 if the shape is not served (caller: fp32 kernel)
// `gout` non-null: the deferred-skip form -- the block writes h' and its gate output as a bf16 image [clip][L][256] to gout and
// leaves `skip` alone; launch_skipgemm_bf16 then adds a group of layers' skip_conv outputs in one GEMM (ap_skipgemm_bf16.hip)
// ap_resblock_bf16s.hip: the deferred-skip block for launches of at most one 128-sample tile per CU (64-sample tiles, bit-identical results)
bool resblock_bf16s_serves(const ap_ctx *ctx, int B, int L);
int launch_resblock_bf16s(ap_ctx *ctx, int layer, const float *hin, const float *pt, float *hout, void *gout, int B, int L, hipStream_t st);
int launch_resblock_bf16(ap_ctx *ctx, int layer, const float *hin, const float *pt, float *hout, float *skip,
                         int accumulate, int B, int L, hipStream_t st, void *gout = nullptr, void *fout = nullptr);
int launch_resblock_bf16p(ap_ctx *ctx, int layer, const float *hin, const float *pt, float *hout, float *skip,
                          int accumulate, int B, int L, hipStream_t st, void *gout = nullptr, void *fout = nullptr);   // persistent form; returns 1 if the shape is not served
                                                                  // (fout, with gout: + the gate's derivative factors, 128 KB per 128-sample tile)
// AP_PREC_BF16_STORE (ap_resblock_bf16u.hip): the residual stream as bf16 images of u = h + part_t, [clip][C / 32][L][32]
bool resblock_bf16u_serves(const ap_ctx *ctx, int L);
int launch_init_conv_u(ap_ctx *ctx, const float *x, const float *pt0, void *u, int B, int L, hipStream_t st);
bool resblock_bf16us_serves(const ap_ctx *ctx, int B, int L);     // AP_PREC_BF16_STORE, at most one 128-sample tile per CU: 64-sample tiles (ap_resblock_bf16us.hip)
int launch_resblock_bf16us(ap_ctx *ctx, int layer, const void *uin, const float *pt_next, void *uout, void *gout, int B, int L, hipStream_t st);
int launch_resblock_bf16u(ap_ctx *ctx, int layer, const void *uin, const float *pt_next, void *uout, void *gout, int B, int L, hipStream_t st,
                          void *fout = nullptr);                  // uout null: the net's last layer; fout: + the gate's derivative factors
int launch_skipgemm_bf16(ap_ctx *ctx, int layer0, int nl, const void *gimg, float *skip, int accumulate, int B, int L, hipStream_t st);
int launch_resblock_bf16w(ap_ctx *ctx, int layer, const float *hin, const float *pt, float *hout, float *skip,
                          int accumulate, int B, int L, hipStream_t st);   // one wave per SIMD; returns 1 if the shape is not served
int launch_pack_f32w(ap_ctx *ctx, hipStream_t st);
bool resblock_f32w_serves(const ap_ctx *ctx, int B, int L);       // AP_PREC_F32 in minimal-filtering form, and this shape is built
int launch_resblock_f32w(ap_ctx *ctx, int layer, const float *hin, const float *pt, float *hout, float *skip,
                         int accumulate, int B, int L, hipStream_t st, float *aout = nullptr);   // hout null: the net's last layer (no res_conv, no h'); returns 1 if the shape is not served
int launch_pack_split(ap_ctx *ctx, hipStream_t st);
int launch_pack_split23(ap_ctx *ctx, hipStream_t st);            // ap_resblock_f32s2.hip: AP_PREC_F32_SPLIT with the dilated conv in F(2,3) form
bool resblock_split23_serves(const ap_ctx *ctx, int B, int L);
int launch_resblock_split23(ap_ctx *ctx, int layer, const float *hin, const float *pt, float *hout, float *skip, int accumulate, int B, int L,
                            hipStream_t st);
int launch_resblock_split(ap_ctx *ctx, int layer, const float *hin, const float *pt, float *hout, float *skip,
                          int accumulate, int B, int L, hipStream_t st);
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
