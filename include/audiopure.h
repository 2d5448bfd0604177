/*
 * audiopure.h — C-ABI of the MI355X-native diffusion-purification hot path.
 *
 * The reference (cychomatica/AudioPure) has no FFI layer: its boundary is Python
 * class identity.  This header is the boundary a maintainer
 * would bind from the reference's Python classes (ctypes stub: INTEGRATION.md);
 * each entry point names the reference code it replaces (file:line relative to
 * the reference checkout).
 *
 * Conventions
 *  - plain C, no C++/torch types; every function returns 0 on success or a
 *    negative errno-style code and never throws; ap_last_error() gives the text.
 *  - every `*_dev` / float* tensor argument is a DEVICE pointer owned by the
 *    caller (e.g. the PyTorch caching allocator); the library allocates device
 *    memory only inside ap_ctx_load_wavenet / ap_ctx_prepare_backward / ap_m5_create.
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *    All work is enqueued asynchronously on it; nothing synchronises the host
 *    (ap_ctx_load_wavenet / ap_ctx_prepare_backward / ap_m5_create excepted), so every
 *    launch function is hipGraph-capturable.
 *  - tensors are fp32, layout [B][C][L] row-major with the sample axis contiguous,
 *    exactly the reference's `[B,1,16000]` / `[B,C,L]` tensors.
 *  - noise: `z` arguments may be NULL; then N(0,1) samples come from the library's
 *    counter-based Philox4x32-10 keyed on (seed, draw, GLOBAL utterance index
 *    = utt_offset + b, sample index), so results do not depend on how a batch
 *    is sharded over GPUs.  Non-NULL z is used as given (parity tests inject it;
 *    the reference draws torch.normal on the global RNG, diffwave_ddpm.py:66,100).
 */
#ifndef AUDIOPURE_H
#define AUDIOPURE_H

#include <stddef.h>
#include <stdint.h>

#define AP_CONV_SPLIT 0x100
#define AP_CONV_1D 0x200
#define AP_CONV_SPLIT_F16 0x400
#define AP_CONV_DILATION(d) ((d) << 16)

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ap_ctx ap_ctx;
typedef struct ap_m5 ap_m5;

/* arithmetic mode of the two residual-block GEMMs */
enum {
  AP_PREC_F32 = 0,   /* v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate   */
  AP_PREC_BF16 = 1,  /* bf16 operands (RNE), fp32 accumulate; activations stay fp32 in HBM.  Built for the shipped
                        configuration only: res_channels == skip_channels == 256 (any dilation of a power-of-two cycle,
                        any clip length); other shapes return -EINVAL at the first launch (ap_last_error says which) */
  AP_PREC_F32_SPLIT = 2, /* fp32 operands split exactly into three bf16 parts, the six partial products >= 2^-16 of
                            each product on v_mfma_f32_32x32x16_bf16, fp32 accumulate: fp32-class results (dropped
                            terms < 2^-23 of a product) at 6/16 of the fp32 matrix instruction's time; C = 256.  Held to the
                            fp32 kernels' tolerances, and on adversarial operands (cancellation, a 2^40 dynamic range)
                            to <= 2 x the direct fp32 kernel's error against fp64
                            (tests/test_gpu_parity.py::test_fp32_class_modes_bound_their_error_on_adversarial_operands) */
  /* (value 3, AP_PREC_F32_SPLIT_F16 -- two fp16 parts per operand -- was removed in round 5: fp16's exponent range loses
     channels a 2^20 dynamic range apart outright, profiles/r5_fp32_class_adversarial_error.txt) */
  AP_PREC_BF16_STORE = 4  /* AP_PREC_BF16's arithmetic with the residual stream kept in HBM as bf16 (third precision
                             row): each layer hands the next one u = bf16(h' + part_t of that layer) -- the dilated conv's operand
                             and, by the reference's in-place alias (WaveNet.py:77,84), the value the residual carries -- as an
                             image [B][C/32][L][32] (ap_resblock_fwd_u); skip stays fp32 (deferred-skip form).  One more rounding
                             per layer than AP_PREC_BF16 (the residual sees bf16(u) instead of fp32 u).  Input gradients through
                             ap_resblock_fwd_u_save + ap_resblock_bwd_bf16_saved (the bf16 backward kernels).  C = 256. */
};

/* configs/config.json "wavenet_config" + "diffusion_config" (reference: configs/config.json:2-17) */
typedef struct ap_config {
  int32_t res_channels;     /* C  (256) */
  int32_t skip_channels;    /* S  (256); this build requires S == C, C % 64 == 0, C <= 256 */
  int32_t num_res_layers;   /* 36 */
  int32_t dilation_cycle;   /* 12 -> dilation 2^(n mod 12) */
  int32_t embed_dim_in;     /* 128 */
  int32_t embed_dim_mid;    /* 512 */
  int32_t embed_dim_out;    /* 512 */
  int32_t T;                /* 200 */
  float beta_0;             /* 1e-4 */
  float beta_T;             /* 0.02 */
  int32_t precision;        /* AP_PREC_* */
} ap_config;

const char *ap_last_error(void);
int ap_version(void);

/* ---- context -------------------------------------------------------------------------------
 * replaces: create_diffwave_model (diffusion_models/diffwave_ddpm.py:395-411) +
 *           calc_diffusion_hyperparams (DiffWave_Unconditional/util.py:96-123).
 * Host-only (no device allocation, usable without a GPU).  The default schedule tables are the
 * closed form evaluated in double and rounded to fp32; a caller that holds the reference's own
 * fp32 tables (the `diffusion_hyperparams` dict every reference caller passes to DiffWave,
 * diffwave_ddpm.py:18-32) installs them with ap_ctx_set_schedule so both sides use identical
 * coefficients. */
int ap_ctx_create(const ap_config *cfg, ap_ctx **out);
int ap_ctx_destroy(ap_ctx *ctx);

/* Install T-entry host tables Beta, Alpha, Alpha_bar, Sigma (util.py:111-122). */
int ap_ctx_set_schedule(ap_ctx *ctx, const float *beta, const float *alpha, const float *alpha_bar,
                        const float *sigma, int T);
/* Install the VP-SDE tables discrete_betas, alphas_cumprod (diffwave_sde.py:56-58). */
int ap_ctx_set_sde_schedule(ap_ctx *ctx, const float *discrete_betas, const float *alphas_cumprod, int T);

/* Number of fp32 elements of the weight blob for this config. */
size_t ap_wavenet_blob_elems(const ap_config *cfg);

/* Load the epsilon-network weights.  `blob_dev` is the concatenation (fp32, device) of the
 * reference checkpoint's `model_state_dict` tensors IN STATE-DICT ORDER, un-folded
 * (`weight_g`/`weight_v` as stored by nn.utils.weight_norm; WaveNet.py:23-34,138-172):
 *   init_conv.0.conv.{bias,weight_g,weight_v}, residual_layer.fc_t1.{weight,bias},
 *   residual_layer.fc_t2.{weight,bias}, then per block n: fc_t.{weight,bias},
 *   dilated_conv_layer.conv.{bias,weight_g,weight_v}, res_conv.{bias,weight_g,weight_v},
 *   skip_conv.{bias,weight_g,weight_v}; final_conv.0.conv.{bias,weight_g,weight_v},
 *   final_conv.2.conv.{weight,bias}.
 * `embed_freq_dev`: the embed_dim_in/2 frequencies exp(-j ln(1e4)/(half-1)) as the host
 * computes them (util.py:86-88).  Allocates the device weight slab, folds W = g*v/||v|| on device (replaces the 110
 * _weight_norm_interface calls per forward) and packs the MFMA
 * operand images.  Synchronises `stream` before returning. */
int ap_ctx_load_wavenet(ap_ctx *ctx, const float *blob_dev, size_t n_elems,
                        const float *embed_freq_dev, void *stream);

/* Copy the folded (un-packed) weight of one conv back out, for fold-parity tests.
 * which: 0 = dilated conv of `layer` [2C][C][3], 1 = res_conv [C][C], 2 = skip_conv [S][C],
 *        3 = final_conv.0 [S][S], 4 = init_conv [C]. */
int ap_ctx_get_folded(ap_ctx *ctx, int which, int layer, float *out_dev, size_t n_elems, void *stream);

/* Host copies of the schedule (T floats each): which 0=Beta 1=Alpha 2=Alpha_bar 3=Sigma. */
int ap_ctx_get_schedule(ap_ctx *ctx, int which, float *out_host, int n);

/* Measurement hook (bench.py roofline leg): while enabled, every residual-block launch is bracketed by a
 * pair of HIP events on the launch stream; ap_profile_read waits for them, returns the summed kernel time
 * and the number of launches since ap_profile_enable, and resets the counter.  Not graph-capturable while on. */
int ap_profile_enable(ap_ctx *ctx, int enable);
int ap_profile_read(ap_ctx *ctx, double *total_ms, int64_t *launches);
int ap_profile_is_enabled(ap_ctx *ctx);   /* 1 while the hook records events (the launches are then not graph-capturable) */
/* The same reading split by kernel: [0] residual-block launches, [1] skip-GEMM launches of the deferred-skip form (whose time
 * ap_profile_read folds into total_ms while counting only the block launches, so "ms per layer" stays comparable). */
int ap_profile_read_split(ap_ctx *ctx, double *ms_by_kind, int64_t *launches_by_kind);

/* The same hook for the conv-as-GEMM family (BASELINE configs[4]; replaces nothing in the reference -- it times the kernels
 * that stand in for nn.Conv2d / nn.Conv1d / nn.Linear of improved_diffusion/unet.py:462-491 and models/resnext.py:67-142):
 * while enabled every ap_conv2d_fwd launch is bracketed by HIP events on its stream.  ap_conv_profile_read sums kernel
 * time, algorithmic flops (2 N M K) and launches per kernel class (conv_class, csrc/ap_conv_plan.h) -- 0 conv2d_f32_big2<128,128>, 1 big2<64,128>,
 * 2 big2<128,64>, <64,64> and every split-K launch, 3 split-operand kernels, 4 conv2d_f32_big, 5 generic / few-output, 6 conv2d_w3 (3 x 3 layers in F(2,3)
 * form along W: flops are the DIRECT form's 2 N M K, of which it executes two thirds), 7 tools build only -- into caller arrays of n_classes >= 7, and resets.
 * A measurement aid with process-global state: enable it from ONE host thread, for launches of ONE device on ONE stream at a time
 * (bench.py's use); it is off by default and the compute entry points never depend on it. */
/* Caller-owned device buffer for the split-K partial sums of low-resolution conv layers (K sliced over workgroups when a layer
 * has too few output tiles for the chip; slices are summed in order by a second kernel: deterministic).  NULL / 0 disables
 * split-K; a layer whose partial sums do not fit runs un-split.  The library allocates nothing itself.
 * The buffer is registered for the HIP device that is CURRENT at the call (it must be that device's memory, else -EINVAL) and a
 * launch only ever uses the buffer of the device it is issued on; one buffer serves one stream at a time (a split-K layer
 * and its reduce own it between them). */
int ap_conv2d_set_workspace(float *ws, size_t bytes);
int ap_conv_profile_enable(int enable);
int ap_conv_profile_read(double *ms_by_class, double *flop_by_class, int64_t *launches_by_class, int n_classes);
/* Launch i of the current recording (call before ap_conv_profile_read): time, flops, [B Cin H W Cout kh kw stride groups class];
 * returns 1 past the last launch. */
int ap_conv_profile_launch(int i, double *ms, double *flop, int *shape10);

/* Workspace the eps/purify entry points need for a batch of B clips of L samples. */
size_t ap_workspace_bytes(const ap_ctx *ctx, int B, int L);

/* ---- per-layer / per-step pieces -------------------------------------------------------------
 * ap_embed: replaces calc_diffusion_step_embedding + fc_t1/fc_t2 swish MLP + every block's fc_t
 *   (util.py:68-93, WaveNet.py:82-83,124-126).  `step` is the (shared) diffusion step as the
 *   reference passes it: float(t) (diffwave_ddpm.py:157).  part_t_dev: num_res_layers*C + embed_dim_out
 *   floats: [num_res_layers][C] FiLM vectors, then the shared 512-d embedding (scratch). */
int ap_embed(ap_ctx *ctx, float step, float *part_t_dev, void *stream);

/* ap_init_conv: ReLU(Conv1x1 1->C) (WaveNet.py:147,168).  x [B][1][L] -> h [B][C][L].  Every precision mode and width: an fp32
 * primitive (in AP_PREC_BF16_STORE it forms the fp32 h_0 that the input gradient's ap_init_conv_bwd reads). */
int ap_init_conv(ap_ctx *ctx, const float *x, float *h, int B, int L, void *stream);

/* ap_resblock_fwd: one Residual_block.forward (WaveNet.py:75-97), fused:
 *   u = h_in + part_t[c]; y = DilConv_{k=3,d}(u) + b; g = tanh(y[:C]) * sigmoid(y[C:]);
 *   h_out = (u + W_res g + b_res) * sqrt(.5); skip (+)= W_skip g + b_skip.
 * part_t_layer: [C] for this layer.  accumulate_skip = 0 writes skip (layer 0), else adds.
 * h_out must not alias h_in (taps at t +- d read other tiles).  Serves AP_PREC_F32 (res_channels 64, 128 or 256), AP_PREC_F32_SPLIT
 * and AP_PREC_BF16 (res = skip = 256); -22 in AP_PREC_BF16_STORE (below). */
int ap_resblock_fwd(ap_ctx *ctx, int layer, const float *h_in, const float *part_t_layer,
                    float *h_out, float *skip, int accumulate_skip, int B, int L, void *stream);

/* Deferred-skip form of the block (AP_PREC_BF16, res = skip = 256 channels; round 4).  WaveNet.py:90-97,131-135: skip_conv only
 * ever sees bf16(g) in this mode, so the block can hand g on as that bf16 image and the sum over layers `skip += skip_n`
 * (:131-133) can be taken inside one K-concatenated GEMM per group of layers instead of one read-modify-write of the fp32
 * skip tensor per layer.
 *   ap_resblock_fwd_gate: the block of ap_resblock_fwd without skip_conv: writes h_out (bit-identical to ap_resblock_fwd's) and
 *                         g_image [B][L][C] bf16 (512 bytes per sample, channels contiguous); `skip` is not touched.
 *                         h_out may be NULL: res_conv and the h' store are left out (the net's last layer, whose h' nobody reads).
 *   ap_skip_gemm:         skip (+)= sum_{n = layer0 .. layer0 + n_layers - 1} (W_skip,n g_n + b_skip,n) with
 *                         g_images [n_layers][B][L][C] bf16 (slot n - layer0); accumulate_skip = 0 writes skip.
 *   ap_ctx_set_skip_group(G): G > 0 makes ap_eps_fwd / ap_purify_* run this form with groups of G layers (the workspace grows
 *                         by G x B x L x C x 2 bytes: ap_workspace_bytes follows); 0 (default) = the fused block per layer.
 * Results: h identical bit for bit; skip differs from the per-layer form by fp32 summation order only (the bf16 products are
 * the same; a group's K = G x 256 is accumulated in the matrix pipe's fp32 accumulators).
 * ap_resblock_fwd_gate launches of at most 256 128-sample tiles -- one per CU of the MI355X; one or two 1 s clips -- run on 64-sample
 * tiles (ap_resblock_bf16s.hip; the rule: block_plan, csrc/ap_block_plan.h) with bit-identical results: a clip's h' and g image do not depend on the batch it travels in.
 * ap_resblock_fwd_gate: AP_PREC_BF16 only.  ap_skip_gemm and ap_ctx_set_skip_group(G > 0): AP_PREC_BF16 and AP_PREC_BF16_STORE,
 * res = skip = 256 channels; -22 in every other mode (ap_ctx_set_skip_group(0) is accepted everywhere). */
int ap_resblock_fwd_gate(ap_ctx *ctx, int layer, const float *h_in, const float *part_t_layer, float *h_out,
                         void *g_image, int B, int L, void *stream);
int ap_skip_gemm(ap_ctx *ctx, int layer0, int n_layers, const void *g_images, float *skip, int accumulate_skip,
                 int B, int L, void *stream);
int ap_ctx_set_skip_group(ap_ctx *ctx, int layers_per_group);

/* AP_PREC_BF16_STORE block interface (ap_resblock_bf16u.hip).  The u image of a layer: [B][C / 32][L][32] bf16 -- a sample's 32
 * channels of one 32-channel chunk are one 64-byte row, and inside a row position p holds the chunk's channel (p with bits 2 and 3
 * swapped: the register order of a 32 x 32 MFMA accumulator tile, so the epilogue stores straight from its accumulators).
 *   ap_init_conv_u:    u_0 = bf16(ReLU(W0 x + b0) + part_t of layer 0)        (WaveNet.py:147,168 then :82-84)
 *   ap_resblock_fwd_u: y = DilConv(u_in) + b;  g = tanh . sigmoid;  h' = (u_in + W_res bf16(g) + b_res) sqrt(1/2)   (WaveNet.py:87-97);
 *                      u_out = bf16(h' + part_t_next) (part_t_next: [C] of layer + 1), g_image [B][L][C] bf16 for ap_skip_gemm.
 *                      u_out NULL (the net's last layer, whose h' nobody reads: WaveNet.py:131-135): res_conv and the store are left out.
 * ap_resblock_fwd / _gate / _save return -22 in this mode (their h tensors are fp32; ap_resblock_bwd_bf16 recomputes from an fp32
 * layer input this mode never forms: use ap_resblock_fwd_u_save + ap_resblock_bwd_bf16_saved).
 * ap_eps_fwd / ap_purify_* run the whole sweep.  ap_init_conv_u, ap_resblock_fwd_u and ap_resblock_fwd_u_save return -22 in every other
 * mode and width.  ap_resblock_fwd_u launches of at most 256 128-sample tiles run on 64-sample tiles (ap_resblock_bf16us.hip) with
 * bit-identical results, as ap_resblock_fwd_gate's do (block_plan, csrc/ap_block_plan.h). */
int ap_init_conv_u(ap_ctx *ctx, const float *x, const float *part_t_layer0, void *u_out, int B, int L, void *stream);
int ap_resblock_fwd_u(ap_ctx *ctx, int layer, const void *u_in, const float *part_t_next, void *u_out, void *g_image, int B, int L,
                      void *stream);
/* ... and the form that also keeps the gate's derivative factors for ap_resblock_bwd_bf16_saved (see ap_resblock_fwd_gate_save): the
 * gradient of the bf16-storage forward is the bf16 backward's with the rounding of u passed straight through. */
int ap_resblock_fwd_u_save(ap_ctx *ctx, int layer, const void *u_in, const float *part_t_next, void *u_out, void *g_image,
                           void *gate_factors, int B, int L, void *stream);

/* AP_PREC_F32 arithmetic form of the dilated conv (WaveNet.py:87).  1 (default where built: res = skip = 256 channels): the
 * F(2,3) minimal-filtering form over the dilation pair -- outputs t and t + d share their four taps, so the pair costs four
 * [2C x C] products instead of six (block: 12.58 GFLOP per clip instead of 16.78) on the exact-fp32 matrix instruction;
 * transformed weights are computed in double at load, results differ from the direct form by fp32 rounding only and meet the
 * same tolerances against the reference's vectors.  0: the direct form (every other shape always runs it).
 * AP_PREC_F32_SPLIT contexts take the same switch (round 6) but default to 0: form 1 runs the block as two launches -- GEMM1 in
 * F(2,3) form over half of the gate channels per workgroup + the gate, g handed on as fp32 through h_out, then [res_conv; skip_conv] g
 * with the block's epilogues in place (ap_resblock_f32s2.hip) -- 3/4 of the direct split kernel's matrix work at the same 5e-6
 * block tolerance, but only 3-4 % faster (both forms sit at the board's power cap; the second launch's traffic and the doubled
 * staging eat the saved matrix energy) and, like the fp32 F(2,3) form, up to 3 x the direct fp32 kernel's error on a 2^40 dynamic
 * range (the direct split form stays within 2 x): opt-in, not the default.
 * ap_ctx_get_f32_form returns the form the block launches of this context will use.  ap_ctx_set_f32_form: AP_PREC_F32 and
 * AP_PREC_F32_SPLIT contexts (-22 in the bf16 modes); at a width without a minimal-filtering kernel (res != 256) form 1 is accepted
 * and ap_ctx_get_f32_form reports 0, the form that runs. */
int ap_ctx_set_f32_form(ap_ctx *ctx, int form);
int ap_ctx_get_f32_form(ap_ctx *ctx);

/* ap_resblock_fwd_save: ap_resblock_fwd that also writes the pre-gate activations y = DilConv(u) + b (WaveNet.py:87) to
 * pre_gate [B][2C][L] (rows 0..C-1 the tanh half, C..2C-1 the sigmoid half): what the backward of :90 needs, kept by the
 * differentiable purifier (the reference's autograd keeps it too) so that the adjoint does not recompute the dilated conv.
 * AP_PREC_F32 contexts only, res_channels 64 or 256 (-22 otherwise). */
int ap_resblock_fwd_save(ap_ctx *ctx, int layer, const float *h_in, const float *part_t_layer, float *h_out, float *skip,
                         float *pre_gate, int accumulate_skip, int B, int L, void *stream);

/* ap_final_affine: final_conv (WaveNet.py:160-162,170) on skip*sqrt(1/N) (WaveNet.py:135) fused
 * with an affine update of the clip:  eps = W_f2 ReLU(W_f1 (skip*sqrt(1/N)) + b_f1) + b_f2;
 *   out = ca * x + cb * eps + cs * z.
 * eps_out and/or out may be NULL.  z: see header comment (NULL + cs != 0 -> Philox draw `draw`).  Every precision mode and width;
 * the bf16 modes run the S x S 1x1 on bf16 operands (fp32 accumulate), as their blocks do. */
/* ap_resblock_bwd: input gradient of one Residual_block.forward (WaveNet.py:75-97; the reference's autograd does this for
 * robustness_eval/white_box_attack.py:392,437-439), two fused launches (ap_resblock_bwd.hip):
 *   dy = gate'(pre_gate) . ([W_res sqrt(1/2); W_skip]^T [dh_out; dskip])       -> dy_scratch [B][2C][L]
 *   dh_in = sqrt(1/2) dh_out + DilConv^T(dy)                                    (F(2,3) form of the transposed dilated conv)
 * dh_out = d loss / d h' [B][C][L] (zeros for the net's last layer, whose h' is unused), dskip = d loss / d skip_n [B][S][L] (the
 * same tensor for every layer: skip is their sum), pre_gate: what ap_resblock_fwd_save kept for this layer.  The parameters' own
 * gradients are formed from the same cotangents by ap_wgrad_corr / ap_rowsum (below).  AP_PREC_F32, res = skip = 256 channels;
 * ap_resblock_bwd_available returns 1 exactly where ap_resblock_bwd serves (B, L) in this context. */
int ap_resblock_bwd(ap_ctx *ctx, int layer, const float *dh_out, const float *dskip, const float *pre_gate, float *dy_scratch,
                    float *dh_in, int B, int L, void *stream);
/* The backward kernels read their own weight images (fp32: 94 MB, bf16: 47 MB at the shipped shape).  ap_ctx_prepare_backward
 * allocates and packs them for the context's precision and synchronises the host -- like ap_ctx_load_wavenet it is NOT a launch
 * function (call it outside stream capture, once after every ap_ctx_load_wavenet; a second call is a no-op).  ap_resblock_bwd /
 * ap_resblock_bwd_bf16 return -22 until it has been called: they allocate nothing and stay hipGraph-capturable.
 * ap_ctx_prepare_backward serves AP_PREC_F32, AP_PREC_BF16 and AP_PREC_BF16_STORE at res = skip = 256 channels; -22 for
 * AP_PREC_F32_SPLIT and other widths. */
int ap_ctx_prepare_backward(ap_ctx *ctx, void *stream);
int ap_resblock_bwd_available(ap_ctx *ctx, int B, int L);
/* The same gradient in AP_PREC_BF16 (bf16 MFMA operands, fp32 accumulate), from the layer INPUT instead of kept pre-gate activations --
 * on the bf16 matrix pipe the dilated conv is cheaper to recompute than a [B][2C][L] fp32 store per layer is to write:
 *   y = DilConv(bf16(h_in + part_t)) + b;  dy = gate'(y) . ([W_res sqrt(1/2); W_skip]^T [dh_out; dskip])  -> dy_scratch: a bf16 image
 *   [B][L][2C] (B L 1024 bytes);   dh_in = sqrt(1/2) dh_out + DilConv^T(dy).
 * AP_PREC_BF16 contexts only, res = skip = 256 channels.  AP_PREC_BF16_STORE returns -22 (that mode packs the forward's GEMM1 image
 * in the u image's permuted channel order, which this kernel does not stage): use ap_resblock_fwd_u_save + ap_resblock_bwd_bf16_saved.
 * ap_resblock_bwd_bf16_available returns 1 where a bf16 backward serves (B, L) in this context: ap_resblock_bwd_bf16_saved, in both
 * bf16 modes -- in AP_PREC_BF16 also ap_resblock_bwd_bf16. */
int ap_resblock_bwd_bf16(ap_ctx *ctx, int layer, const float *h_in, const float *part_t_layer, const float *dh_out, const float *dskip,
                         void *dy_scratch, float *dh_in, int B, int L, void *stream);
int ap_resblock_bwd_bf16_available(ap_ctx *ctx, int B, int L);
/* The gradient pass can skip the recomputation: ap_resblock_fwd_gate_save is ap_resblock_fwd_gate (bit-identical h_out and g_image)
 * that also keeps the gate's two derivative factors sg (1 - th^2), th sg (1 - sg) as an fp16 pair per (channel, sample) in
 * gate_factors -- an opaque image of ap_gate_factor_bytes(B, L) bytes (128 KB per clip and 128-sample tile, in the block kernel's own
 * accumulator order) -- and ap_resblock_bwd_bf16_saved is ap_resblock_bwd_bf16 that reads them instead of h_in / part_t:
 *   dy = factors . ([W_res sqrt(1/2); W_skip]^T [dh_out; dskip]);   dh_in = sqrt(1/2) dh_out + DilConv^T(dy).
 * (|factor| <= 1 at 11 significant bits; dy is rounded to bf16 behind it either way.)  The reference's autograd keeps its
 * activations too (white_box_attack.py:392,437-439).  ap_resblock_fwd_gate_save: AP_PREC_BF16 only (AP_PREC_BF16_STORE keeps its factors
 * with ap_resblock_fwd_u_save).  ap_resblock_bwd_bf16_saved: AP_PREC_BF16 and AP_PREC_BF16_STORE, res = skip = 256 channels. */
size_t ap_gate_factor_bytes(int B, int L);
int ap_resblock_fwd_gate_save(ap_ctx *ctx, int layer, const float *h_in, const float *part_t_layer, float *h_out, void *g_image,
                              void *gate_factors, int B, int L, void *stream);
int ap_resblock_bwd_bf16_saved(ap_ctx *ctx, int layer, const void *gate_factors, const float *dh_out, const void *dskip,
                               int dskip_is_image, void *dy_scratch, float *dh_in, int B, int L, void *stream);
/* dskip is the same tensor for every layer of an evaluation (skip is their sum): with dskip_is_image != 0 it is handed over once as
 * the bf16 image [B][L][S] ap_bwd_bf16_rows_image makes of the fp32 rows [B][S][L] (C = 256) -- what the kernel's staging would round
 * it to anyway, at half the bytes per layer and without the convert. */
int ap_bwd_bf16_rows_image(const float *rows, void *image, int B, int C, int L, void *stream);

int ap_final_affine(ap_ctx *ctx, const float *skip, const float *x, float *eps_out, float *out,
                    float ca, float cb, float cs, const float *z, uint64_t seed, uint32_t draw,
                    uint64_t utt_offset, int B, int L, void *stream);

/* out = ca * x + cs * z  (q-sample, diffwave_ddpm.py:66-67; also fills z-only buffers with ca = 0). */
int ap_affine_noise(const float *x, float *out, float ca, float cs, const float *z, uint64_t seed,
                    uint32_t draw, uint64_t utt_offset, int B, int L, void *stream);

/* ---- whole network / whole purification -----------------------------------------------------
 * ap_eps_fwd: WaveNet_Speech_Commands.forward((x, step*ones)) (WaveNet.py:164-172;
 *   DiffWave.compute_eps_t, diffwave_ddpm.py:166-172).  x, eps_out: [B][1][L]. */
int ap_eps_fwd(ap_ctx *ctx, const float *x, float step, float *eps_out, int B, int L,
               void *workspace, size_t ws_bytes, void *stream);

/* ap_eps_affine: one eps-evaluation that also returns out = ca*x + cb*eps in the same launch sequence
 * (DiffWave.compute_coefficients -> (eps, mu, sigma), diffwave_ddpm.py:143-164).  eps_out or out may be NULL. */
int ap_eps_affine(ap_ctx *ctx, const float *x, float step, float ca, float cb, float *eps_out, float *out,
                  int B, int L, void *workspace, size_t ws_bytes, void *stream);

/* One link of a sampling chain: eps = net(x, step); x <- ca*x + cb*eps + cs*z_draw.
 * DDPM, the SDE Euler scheme, one-shot denoising and respaced samplers (DiffWave.fast_reverse,
 * diffwave_ddpm.py:106-141) are all chains of this link with different coefficient tables. */
typedef struct ap_step {
  float step;      /* value fed to the step embedding (float(t), diffwave_ddpm.py:157) */
  float ca, cb, cs;
  int32_t draw;    /* index into z_all / Philox draw id; ignored when cs == 0 */
} ap_step;

/* ap_purify_chain: optional q-sample (x <- qa*x0 + qs*z_0; skipped when qa == 1 and qs == 0) followed by
 * n_steps links.  z_all: NULL (Philox) or [n_draws][B][L] device tensors indexed by `draw`. */
int ap_purify_chain(ap_ctx *ctx, const float *x0, float qa, float qs, const ap_step *steps, int n_steps,
                    const float *z_all, uint64_t seed, uint64_t utt_offset, float *x_out, int B, int L,
                    void *workspace, size_t ws_bytes, void *stream);

/* ap_purify_ddpm: DiffWave.forward = _diffusion + _reverse (diffwave_ddpm.py:36-104,143-164):
 *   x <- sqrt(ab[t*-1]) x0 + sqrt(1-ab[t*-1]) z0; for t = t*-1..0: eps = net(x,t);
 *   mu = (x - (1-a_t)/sqrt(1-ab_t) eps)/sqrt(a_t); x <- mu + Sigma[t] z_t (t>0) | mu.
 * z_all: NULL (Philox) or t* device tensors [t*][B][L] (z_all[0] = q-sample draw).
 * do_diffuse = 0 skips the q-sample (DiffWave._reverse alone). */
int ap_purify_ddpm(ap_ctx *ctx, const float *x0, int t_star, int do_diffuse, const float *z_all,
                   uint64_t seed, uint64_t utt_offset, float *x_out, int B, int L,
                   void *workspace, size_t ws_bytes, void *stream);

/* ap_purify_sde: RevDiffWave.audio_editing_sample, sample_step = 1 (diffwave_sde.py:167-212) with
 * torchsde's fixed-step Euler-Maruyama restated: per k = t*-1..0
 *   x <- x (1 + b_k/2) - b_k eps(x,k)/sqrt(1-ac_k) + sqrt(b_k) sqrt((1-ac_{k-1})/(1-ac_k)) z  (0 at k=0)
 * with ac = cumprod(1-b) (diffwave_sde.py:58).  Exactly t* eps-evaluations. */
int ap_purify_sde(ap_ctx *ctx, const float *x0, int t_star, const float *z_all, uint64_t seed,
                  uint64_t utt_offset, float *x_out, int B, int L,
                  void *workspace, size_t ws_bytes, void *stream);

/* ap_one_shot_denoise: DiffWave.one_shot_denoise (diffwave_ddpm.py:174-205), t = t*-1. */
int ap_one_shot_denoise(ap_ctx *ctx, const float *x_t, int t_star, float *x0_hat, int B, int L,
                        void *workspace, size_t ws_bytes, void *stream);

/* ---- classifier front-end --------------------------------------------------------------------
 * ap_m5_*: M5.forward (audio_models/M5/M5Net.py:21-38), BatchNorm in eval mode folded at create.
 * `blob_dev`: fp32 concat in state-dict order per stage i=1..4:
 *   conv{i}.weight, conv{i}.bias, bn{i}.weight, bn{i}.bias, bn{i}.running_mean, bn{i}.running_var;
 *   then fc1.weight, fc1.bias.  x [B][1][L] -> log-probabilities [B][n_output]. */
int ap_m5_create(int n_output, int n_channel, int first_kernel, int stride, float bn_eps,
                 const float *blob_dev, size_t n_elems, void *stream, ap_m5 **out);
int ap_m5_destroy(ap_m5 *m);
size_t ap_m5_blob_elems(int n_output, int n_channel, int first_kernel);
int ap_m5_fwd(ap_m5 *m, const float *x, float *logprobs, int B, int L, void *stream);

/* ap_melspec_db: the eval scripts' torchaudio front-end (adaptive_attack_eval.py:83-85):
 * MelSpectrogram(n_fft=2048, hop=512, n_mels, norm='slaney', mel_scale='slaney', pad_mode='constant')
 * + AmplitudeToDB('power').  x [B][1][L] -> [B][1][n_mels][1 + L/512].
 * mode 0: absolute dB (torchaudio); mode 1: librosa power_to_db(ref=max, top_db=80) as
 * transforms/transforms_stft.py:101-114 (ToSTFT + ToMelSpectrogramFromSTFT). */
int ap_melspec_db(const float *x, float *out, int n_mels, int mode, int B, int L, void *stream);

/* ---- 2-D ConvNet classifiers on the mel front-end (audio_models/ConvNets_SpeechCommands/models/ : vgg.py, resnet.py,
 * wideresnet.py, resnext.py:67-142, dpn.py, densenet.py).  The host lowers an eval-mode network
 * to these NCHW fp32 primitives (audiopure_amd/convnet.py); BatchNorm is folded into the conv or applied as a
 * per-channel affine.  `*_cstride` / `*_coff`: the operand is channels [coff, coff+C) of a tensor with cstride channels
 * (torch.cat results and x[:, :d] slices are consumed in place).
 *
 * ap_conv2d_pack: w [Cout][Cin/g][kh][kw] (times scale[Cout] if non-NULL, the folded BatchNorm gamma/sqrt(var+eps))
 *   -> wT [groups][ (Cin/g) kh kw ][Cout/g], the A-operand image of the implicit GEMM, followed (layers with
 *   Cin/g % 16 == 0 and Cout/g >= 64) by the same weights as MFMA A fragments in tap-major K order, which the
 *   streamed-weight kernel reads straight from L2; allocate ap_conv2d_packed_elems(...) floats.
 * ap_conv2d_fwd: out = [relu]( conv2d(x, w, stride, pad, groups) + bias + res ), nn.Conv2d semantics (cross-correlation,
 *   zero padding); bias / res may be NULL; res has the shape of out.  conv-as-GEMM on v_mfma_f32_32x32x2_f32.
 *   `relu` is a flag word: bit 0 = fused ReLU, bit 8 (AP_CONV_SPLIT) = run eligible layers (Cin/g % 16 == 0,
 *   Cout/g >= 64) on the bf16 MFMA with exactly 3-way-split fp32 operands (AP_PREC_F32_SPLIT's arithmetic); bit 9
 *   (AP_CONV_1D) = padding and dilation apply to W only (nn.Conv1d over [B][C][1][L]); bit 10 (AP_CONV_SPLIT_F16) = the
 *   same layers with operands as two fp16 parts, three partial products on the fp16 MFMA (valid for |w|, |x| < 3750 and a
 *   narrow dynamic range only -- the normalised activations of the UNet; not an fp32-class mode); bits 16-31 = dilation (0 = 1).
 *   nn.Linear is the kh = kw = H = W = 1 case. */
size_t ap_conv2d_packed_elems(int Cout, int Cin_g, int kh, int kw, int groups);   /* floats ap_conv2d_pack writes */
int ap_conv2d_pack(const float *w, const float *scale, float *wT, int Cout, int Cin_g, int kh, int kw, int groups,
                   void *stream);
int ap_conv2d_fwd(const float *x, const float *wT, const float *bias, const float *res, float *out, int B, int Cin,
                  int H, int W, int Cout, int kh, int kw, int stride, int pad, int groups, int relu, int x_cstride,
                  int x_coff, void *stream);
/* ap_conv2d_fwd with `out` a channel slice [out_coff, out_coff + Cout) of a tensor of out_cstride channels -- the destination
 * of the torch.cat that follows the layer in improved_diffusion/unet.py:490-491 (h = th.cat([h, hs.pop()], dim=1)): the layer
 * that produces h writes it in place.  `res` keeps the shape of the convolution's own output.  Layers of the streamed-weight
 * fp32 kernel only (Cin/g % 16 == 0, Cout/g >= 64, no split-operand flag); -22 otherwise. */
int ap_conv2d_fwd_slice(const float *x, const float *wT, const float *bias, const float *res, float *out, int B, int Cin,
                        int H, int W, int Cout, int kh, int kw, int stride, int pad, int groups, int relu, int x_cstride,
                        int x_coff, int out_cstride, int out_coff, void *stream);
/* y[B][C][HW] = [relu](x * scale[c] + shift[c]); scale == NULL: plain (optionally ReLU'd) copy of the slice. */
int ap_affine_nchw(const float *x, const float *scale, const float *shift, float *y, int B, int C, int HW,
                   int x_cstride, int x_coff, int relu, void *stream);
/* y = [relu](a + b) on channel slices. */
int ap_add_nchw(const float *a, const float *b, float *y, int B, int C, int HW, int a_cstride, int a_coff,
                int b_cstride, int b_coff, int relu, void *stream);
/* dst[:, d_coff : d_coff + C] = src[:, s_coff : s_coff + C]  (torch.cat). */
int ap_copy_channels(const float *src, float *dst, int B, int C, int HW, int s_cstride, int s_coff, int d_cstride,
                     int d_coff, void *stream);
/* nn.MaxPool2d / F.avg_pool2d(k, stride, pad) on [BC][H][W]. */
int ap_pool2d(const float *x, float *y, int BC, int H, int W, int k, int stride, int pad, int is_max, void *stream);

/* ---- Improved-Diffusion UNet pieces (Improved_Diffusion_Unconditional/improved_diffusion/unet.py, nn.py; section 8 a15).
 * ap_groupnorm_nchw: GroupNorm32 (nn.py:17-19,95-102) on [B][C][HW], optionally followed by the scale-shift FiLM of
 *   use_scale_shift_norm, y = gn(x) * (1 + scale[b][c]) + shift[b][c] with scale_shift = [B][2C] (unet.py:184-190),
 *   and an activation (act: 0 none, 1 ReLU, 2 SiLU).
 * ap_timestep_embedding: [cos(t f_j), sin(t f_j)] (nn.py:103-121); freqs computed by the host like the reference.
 * ap_silu, ap_upsample_nearest2x (unet.py:60-72).
 * ap_attention_qkv: QKVAttention (unet.py:239-252) on qkv [B][heads][3*ch][T] -> [B][heads*ch][T], fp32 softmax. */
int ap_groupnorm_nchw(const float *x, const float *gamma, const float *beta, const float *scale_shift, float *y, int B,
                      int C, int HW, int groups, float eps, int act, void *stream);
int ap_timestep_embedding(const float *t_dev, const float *freqs_dev, float *out, int B, int dim, void *stream);
int ap_silu(const float *x, float *y, size_t n, void *stream);
int ap_upsample_nearest2x(const float *x, float *y, int BC, int H, int W, void *stream);
int ap_attention_qkv(const float *qkv, float *out, int B, int C, int T, int heads, void *stream);
/* Input gradients of the three above (white-box attack through the DiffSpec purifier, adaptive_attack_eval.py:102-104 +
 * white_box_attack.py:437-439; the convolutions' input gradients are ap_conv2d_fwd on flipped / transposed weights).
 * ap_groupnorm_bwd: x and the forward's parameters + dy -> dx.  ap_attention_qkv_bwd: qkv, the forward's `out`, dout ->
 * dqkv (same layout as qkv); `stats` holds B * heads * T * 3 floats.  ap_upsample_nearest2x_bwd: dy [BC][2H][2W] -> dx. */
int ap_groupnorm_bwd(const float *x, const float *gamma, const float *beta, const float *scale_shift, const float *dy,
                     float *dx, int B, int C, int HW, int groups, float eps, int act, void *stream);
int ap_attention_qkv_bwd(const float *qkv, const float *out, const float *dout, float *dqkv, float *stats, int B, int C,
                         int T, int heads, void *stream);
int ap_upsample_nearest2x_bwd(const float *dy, float *dx, int BC, int H, int W, void *stream);
/* out = a*x + b*y + c elementwise (y may be NULL): melspec_standardize / inv (sc09_spectrogram_dataset.py:65-81) and the
 * Euler links of the spectrogram SDE (improved_diffusion_sde.py:173-221). */
int ap_axpbyc(const float *x, const float *y, float *out, float a, float b, float c, size_t n, void *stream);
/* GaussianDiffusion.p_sample, epsilon prediction + fixed variance (gaussian_diffusion.py:232-387): pred_x0 =
 * clamp(r1 x - r2 eps, -1, 1) (clip != 0), mean = c1 pred_x0 + c2 x, out = mean + sigma z (z NULL at t = 0). */
int ap_psample_update(const float *x, const float *eps, const float *z, float *out, float r1, float r2, float c1, float c2,
                      float sigma, int clip, size_t n, void *stream);

/* Fill out[B][L] with the library's Philox N(0,1) stream (same values the fused paths use). */
int ap_philox_normal(float *out, uint64_t seed, uint32_t draw, uint64_t utt_offset, int B, int L,
                     void *stream);

/* ---- baseline defenses (`--defense AS | MS | AT | DS | LPF | BPF`, adaptive_attack_eval.py:36,106-125) ----
 * transforms/time_defense.py and transforms/frequency_defense.py on x[B][L], fp32, any L >= 1, 1 <= B <= 65535.  Each
 * forward has an input-gradient launch (its adjoint); nothing reads device data on the host.  Refusals return -22 with
 * ap_last_error set: a NULL tensor, B or L out of range, and the op-specific ones listed below. */
#define AP_MS_MAX_WINDOW 63     /* largest median window */
#define AP_IIR_MAX_COEF 16      /* largest len(b) == len(a) of ap_iir_*: order 15 */
#define AP_IIR_CHUNK 128        /* time chunk of the IIR scan: AC = A^128, H[128][order] */
#define AP_DS_DOWN_TAPS 28      /* torchaudio sinc_interpolation 16 k -> 8 k kernel (width 13, stride 2) */
#define AP_DS_UP_TAPS 15        /* ... 8 k -> 16 k kernel per output phase (width 7, 2 phases) */

/* AS (time_defense.py:117-124): y[n] = sum_{|j| <= r} w x[n + j], k = 2r + 1, w = float(1 / k), zero padding.
 * The operator is symmetric Toeplitz: its adjoint IS this launch (call it on the cotangent).  Refuses an even or
 * non-positive k. */
int ap_avg_smooth(const float *x, float *y, int k, int B, int L, void *stream);
/* MS (time_defense.py:146-156): y[n] = median of x[n - r .. n + r] (zero padding, odd k <= AP_MS_MAX_WINDOW); argoff[n]
 * (int8, in [-r, r]) is the offset of the element picked.  Tie rule: the element of rank r in the order (value, then
 * position), i.e. the middle one of a run of equal values in window order.  Refuses an even k or k > 63. */
int ap_median_smooth(const float *x, float *y, int8_t *argoff, int k, int B, int L, void *stream);
/* MS adjoint, a gather with no atomics: dx[m] = sum over n with n + argoff[n] == m of g[n] (n ascending). */
int ap_median_smooth_bwd(const float *g, const int8_t *argoff, float *dx, int k, int B, int L, void *stream);
/* AT (time_defense.py:93-100): P = sum_n x^2 / L per clip, y = x + z sqrt(P / snr), snr = 10^(param / 10); z [B][L] is
 * given (the Python layer fills it from ap_philox_normal unless the caller injects it).  A silent clip (P = 0) gives y = x.
 * Refuses snr <= 0. */
int ap_at_fwd(const float *x, const float *z, float *y, float snr, int B, int L, void *stream);
/* AT adjoint, with the term through P as autograd differentiates the reference: dx = g + (sum g z) x / (L snr sqrt(P / snr));
 * for a silent clip that term is dropped (dx = g; the reference's autograd gives NaN there). */
int ap_at_bwd(const float *x, const float *z, const float *g, float *dx, float snr, int B, int L, void *stream);
/* DS (frequency_defense.py:38-58): torchaudio 0.11 Resample(16 k -> 8 k) then Resample(8 k -> 16 k), sinc_interpolation,
 * lowpass_filter_width 6, rolloff 0.99.  kd[28] and ku[2][15] (HOST arrays, fp32) are the two kernels as torchaudio
 * builds them; d[m] = sum_j kd[j] x[2m + j - 13] for 0 <= m < M = ceil(L / 2), y[2n + p] = sum_j ku[p][j] d[n + j - 7];
 * y is [B][Lout] with Lout = L (same_size) or 2M.  Refuses any other Lout. */
int ap_ds_fwd(const float *x, float *y, const float *kd, const float *ku, int B, int L, int Lout, void *stream);
/* DS adjoint: g [B][Lout] -> dx [B][L], the transposed up- then down-sampling pair. */
int ap_ds_bwd(const float *g, float *dx, const float *kd, const float *ku, int B, int L, int Lout, void *stream);
/* LPF / BPF (frequency_defense.py:60-141): lfilter(b, a) per clip (direct form II transposed, zero initial state), then
 * clamp.  b, a: HOST arrays of ncoef (2 .. AP_IIR_MAX_COEF) fp32 coefficients, normalised here by a[0]; AC: HOST fp64
 * [N][N] (N = ncoef - 1) = A^AP_IIR_CHUNK of the state recurrence s' = A s + B u, A[i][0] = -a[i+1], A[i][i+1] = 1; H:
 * DEVICE fp64 [AP_IIR_CHUNK][N], H[k] = e_0' A^k (the zero-input output basis).  The state is carried in fp64 (poles near
 * the unit circle amplify fp32 state rounding); input and output are fp32.  scratch: ap_iir_scratch_elems floats.
 * Clamp rule over the whole batch, decided on the device (minmax: 2 DEVICE words this call writes): [-1, 1] if
 * 0.9 max(x) <= 1 and 0.9 min(x) >= -1, else [-2^(bits-1), 2^(bits-1) - 1].  ypre (may be NULL) receives the values
 * before the clamp.  Refuses ncoef outside 2 .. 16, a[0] == 0, bits outside 2 .. 31. */
size_t ap_iir_scratch_elems(int ncoef, int B, int L);
int ap_iir_fwd(const float *x, float *y, float *ypre, unsigned *minmax, const float *b, const float *a, int ncoef,
               const double *AC, const double *H, float *scratch, int bits, int B, int L, void *stream);
/* LPF / BPF adjoint: the same scan backwards in time on g * 1[lo <= ypre <= hi] (inclusive, as clamp's backward), with the
 * forward's ypre and minmax; ypre == NULL applies no mask (the adjoint of the filter alone). */
int ap_iir_bwd(const float *g, const float *ypre, const unsigned *minmax, float *dx, const float *b, const float *a,
               int ncoef, const double *AC, const double *H, float *scratch, int bits, int B, int L, void *stream);

/* ---- psychoacoustic masking threshold and hinge loss of the attack's second, imperceptible stage (Qin et al. 2019;
 * robustness_eval/white_box_attack.py:36-273 PsychoacousticMasker, :610-710 AudioAttack's loss, gradient and stabilised
 * thresholds).  Window 2048 (periodic Hann), hop `hop`, center=False: F = 1 + (L - 2048) / hop frames of 1025 bins.
 * `tables`: DEVICE fp64 [AP_PSY_TABLE_ELEMS] built on the host from the masker's sample rate: the analysis window
 * (scipy.signal.get_window("hann", 2048), :163-168) at 0, the bark scale of the 1025 bin frequencies at 2048 (:111-125),
 * the absolute threshold of hearing at 3073 (-inf outside 20 Hz .. 20 kHz; :127-149).  `scratch`: ap_psy_scratch_elems
 * floats, shared by both calls.  Window sizes other than 2048, hop outside [1, 2048] and L < 2048 are refused (-22). */
#define AP_PSY_TABLE_ELEMS (2048 + 2 * 1025)
size_t ap_psy_scratch_elems(int window, int hop, int B, int L);
/* PsychoacousticMasker.calculate_threshold_and_psd_maximum (:61-86) for x [B][L] plus the stabilisation of
 * AudioAttack._stabilized_threshold_and_psd_maximum (:692-715): thr_stab [B][1025][F] = 10^(0.1 threshold),
 * psd_max_stab [B] = 10^(0.1 psd_max).  thr_db [B][1025][F] (the fp32 threshold in dB) and psd_max_db [B] may be NULL.
 * On return `scratch` holds the first stage: the fp32 PSD in dB, un-normalised and floored at -200, [B][F][1025], followed by
 * its per-frame maxima [B][F] (B F 1026 floats in all; the rest of ap_psy_scratch_elems is not written).  The clip maximum
 * psd_max is the maximum of a clip's F frame maxima; the threshold is computed from the PSD shifted by 96 - psd_max. */
int ap_psy_threshold(const float *x, const double *tables, float *thr_stab, float *thr_db, float *psd_max_stab,
                     float *psd_max_db, float *scratch, int window, int hop, int B, int L, void *stream);
/* AudioAttack._loss_gradient_masking_threshold (:610-690) for the perturbation delta [B][L]: loss [B] = mean over bins and
 * frames of relu(10^9.6 / psd_max_stab |sqrt(8/3) STFT(delta) / 2048|^2 - thr_stab), grad [B][L] = dloss[b] / ddelta[b]
 * (0 past the last frame; 0 where the spectrum is exactly 0, where the reference's sqrt backward gives NaN). */
int ap_psy_loss_grad(const float *delta, const float *thr_stab, const float *psd_max_stab, float *grad, float *loss,
                     float *scratch, int window, int hop, int B, int L, void *stream);

/* ---- keyword-spotting route: clips of any length ----
 * ap_kws_*: KWSModel.forward (audio_models/RCNN_KWS/model.py:66-114): depthwise Conv1d(k=5, s=2) + grouped pointwise
 * Conv1d(s=8), 2-layer bidirectional GRU, additive attention, linear, log-softmax.  `blob_dev`: the state dict
 * concatenated in state-dict order.  mel [B][n_mels][T] -> log-probabilities [B][num_classes].
 * ap_melspec_db_htk: the front-end that script builds (kws_adaptive_attack_eval.py:65-67):
 * torchaudio MelSpectrogram(sample_rate=16000, n_mels) with default n_fft = 400, hop = 200, reflect padding, HTK scale,
 * + AmplitudeToDB('power').  x [B][1][L] -> [B][1][n_mels][1 + L/200]. */
typedef struct ap_kws ap_kws;
size_t ap_kws_blob_elems(int n_mels, int hidden, int num_classes);
int ap_kws_create(int n_mels, int hidden, int num_classes, const float *blob_dev, size_t n_elems, void *stream, ap_kws **out);
int ap_kws_destroy(ap_kws *k);
int ap_kws_fwd(ap_kws *k, const float *mel, float *logprobs, int B, int T, void *stream);
int ap_melspec_db_htk(const float *x, float *out, int n_mels, int B, int L, void *stream);
/* Input gradients of the two above (the script's default attack is PGD through front-end + classifier,
 * kws_adaptive_attack_eval.py:132-143).  ap_kws_bwd: dlogprobs [B][K] -> dmel [B][n_mels][T]; `scratch` holds
 * ap_kws_bwd_scratch_elems floats (the recomputed GRU gates).  ap_melspec_db_htk_bwd: dout [B][n_mels][1 + L/200] ->
 * dx [B][L]; `scratch` holds B * (1 + L/200) * 400 floats. */
size_t ap_kws_bwd_scratch_elems(const ap_kws *k, int B, int T);
int ap_kws_bwd(ap_kws *k, const float *mel, const float *dlogprobs, float *dmel, float *scratch, int B, int T, void *stream);
int ap_melspec_db_htk_bwd(const float *x, const float *dout, float *dx, float *scratch, int n_mels, int B, int L, void *stream);
/* Training step of KWSModel (audio_models/RCNN_KWS/train.py:84-121 the PGD inner loop in train(), :147-153 CrossEntropyLoss +
 * loss.backward() + Adam, :177 validation in train()).  The model has no BatchNorm and no dropout: the train-mode forward is
 * ap_kws_fwd.  ap_kws_train_bwd: dlogprobs [B][K] -> dparams, one gradient blob in the layout of `blob_dev` (state-dict order),
 * overwritten, and -- unless dmel is NULL -- dmel [B][n_mels][T] with the bits of ap_kws_bwd.  `workspace` holds
 * ap_kws_train_workspace_elems floats: the per-clip saves of the sweep and 16 partial blobs that are summed in a fixed order
 * (no atomics: two runs give the same bits).  Refused with -22 before any launch: a null handle or pointer (dmel excepted),
 * B < 1, T < 5, a workspace too small, hidden > 128, num_classes > 64.
 * ap_kws_set_weights: what the optimizer step (train.py:153) asks of the handle -- a stream-ordered copy of a new blob into the
 * existing one, with no allocation and no synchronisation; n_elems is checked as by ap_kws_create. */
size_t ap_kws_train_workspace_elems(const ap_kws *k, int B, int T);
int ap_kws_train_bwd(ap_kws *k, const float *mel, const float *dlogprobs, float *dmel, float *dparams, float *workspace,
                     size_t workspace_elems, int B, int T, void *stream);
int ap_kws_set_weights(ap_kws *k, const float *blob_dev, size_t n_elems, void *stream);

/* ---- input gradient of the eps-network (reference: the white-box attack back-propagates through
 * the defender, robustness_eval/white_box_attack.py:392,437-439; diffwave_sde.py:200-204 sdeint_adjoint).  The GEMM-shaped
 * terms run on ap_conv2d_fwd (AP_CONV_1D + dilation); these are the element-wise pieces between them. ---- */
/* WaveNet.py:90 backward: a = [a_t; a_s] [B][2C][L], dg [B][C][L] -> da [B][2C][L] */
int ap_gate_bwd(const float *a, const float *dg, float *da, int B, int C, int L, void *stream);
/* WaveNet.py:160-162 backward through the ReLU: dr[b][c][t] = r > 0 ? w2[c] deps[b][t] : 0 */
int ap_relu_outer_bwd(const float *r, const float *w2, const float *deps, float *dr, int B, int S, int L, void *stream);
/* NES queries of the black-box attack (robustness_eval/_NES.py:14-55) with counter-based noise: ap_nes_perturb writes,
 * per audio a, [lead unperturbed copy,] S/2 copies x + sigma z_p and S/2 copies x - sigma z_p (z_p = Philox(seed, draw,
 * a S/2 + p)) into out [A][S + lead][L]; ap_nes_grad forms grad[a] (+)= (1/S) sum_p (loss[a][p] - loss[a][p + S/2]) z_p
 * from the per-copy losses [A][S], regenerating z_p -- the reference's [A][S][L] noise tensor never exists. */
int ap_nes_perturb(const float *x, float *out, float sigma, uint64_t seed, uint32_t draw, int A, int S, int lead, int L,
                   void *stream);
int ap_nes_grad(const float *loss, float *grad, uint64_t seed, uint32_t draw, int A, int S, int L, int accumulate,
                void *stream);
/* counts[argmax_k scores[b][k]] += 1 for b < B (int64 device histogram of K + 1 slots; certified_robust.py:58-65).
 * Rows holding a NaN or an infinity are not votes: they are counted in slot K. */
int ap_argmax_hist(const float *scores, long long *counts, int B, int K, void *stream);
/* pieces of the input gradient of the lowered 2-D classifiers (audiopure_amd/convnet.py): slice accumulate, backward
 * through a fused ReLU, zero insertion for the transposed conv of a strided conv (the conv itself is ap_conv2d_fwd on
 * the flipped, transposed weights), pooling backward. */
int ap_acc_channels(const float *src, float *dst, int B, int C, int HW, int s_cstride, int s_coff, int d_cstride, int d_coff,
                    void *stream);
int ap_relu_mask(const float *dy, const float *y, float *out, size_t n, void *stream);
int ap_zero_insert2d(const float *dy, float *out, int BC, int Ho, int Wo, int Hz, int Wz, int stride, void *stream);
int ap_pool2d_bwd(const float *x, const float *dy, float *dx, int BC, int H, int W, int k, int stride, int pad, int is_max,
                  void *stream);
/* mode-0 ap_melspec_db backward with respect to the waveform: dout [B][n_mels][F] -> dx [B][1][L]; scratch: B F 2048 floats */
int ap_melspec_db_bwd(const float *x, const float *dout, float *dx, float *scratch, int n_mels, int B, int L, void *stream);
/* M5.forward (M5Net.py:20-38) backward with respect to the waveform: dlogprobs [B][n_output] -> dx [B][1][L] */
int ap_m5_bwd(ap_m5 *m, const float *x, const float *dlogprobs, float *dx, int B, int L, void *stream);
/* WaveNet.py:147,168 backward: dx[b][t] = sum_c [h0 > 0] w0[c] dh0[b][c][t] */
int ap_init_conv_bwd(const float *h0, const float *w0, const float *dh0, float *dx, int B, int C, int L, void *stream);

/* ---- parameter gradients of the eps-network (the reference trains it: DiffWave_Unconditional/util.py:161-185 `training_loss`,
 * loss.backward() and Adam in train.py / train_qkws.py).  The input-gradient sweep above forms every cotangent; these contract a
 * cotangent with an activation over (clip, time).  Every sum has a fixed order (no atomics): two runs give the same bits. ---- */
/* Weight gradient of a k = 1 or k = 3 dilated, zero-padded Conv1d (WaveNet.py:26-27 dilated conv :87, res_conv :93, skip_conv :95,
 * final_conv.0 :160), on the exact-fp32 matrix instruction:
 *   G[m][n][k] (+)= p_scale * sum_b sum_t P[b][m][t] * Q~[b][n][t + (k - taps/2) dil],   terms with the Q index outside [0, L) are 0.
 * P [B][M][L] is the cotangent of the conv's output, G [M][N][taps] has the layout of the conv's weight.  Q~ by `mode`:
 *   0  Q [B][N][L] as given;
 *   1  Q + film[n] inside [0, L) (the conv pads u = h + part_t with zeros, so padded samples stay 0; WaveNet.py:84,87);
 *   2  tanh(Q[n]) * sigmoid(Q[n + N]) from pre-gate rows Q [B][2N][L] (WaveNet.py:90).
 * M, N: multiples of 32; taps 1 or 3 (dil ignored for taps = 1); L >= 1.  A tap with |offset| >= L meets no sample: it is skipped and
 * contributes exact zeros.  K = B L is split over workgroups; the partial sums go to `workspace` (ap_wgrad_workspace_bytes(B, M, N, L,
 * taps) bytes, caller-owned: the launch allocates nothing) and a second kernel adds them in slice order; accumulate != 0 adds to G. */
size_t ap_wgrad_workspace_bytes(int B, int M, int N, int L, int taps);
int ap_wgrad_corr(const float *P, const float *Q, const float *film, float *G, void *workspace, size_t ws_bytes, int B, int M, int N,
                  int L, int taps, int dil, int mode, float p_scale, int accumulate, void *stream);
/* out[m] (+)= scale * sum_b sum_t A[b][m][t] * w, A [B][M][L]; w = W's element (W [B][M][L], or the broadcast row W [B][1][L] with
 * w_broadcast != 0; 1 if W is NULL), taken only where R[b][m][t] > 0 if R [B][M][L] is given.  Every conv bias (the sum of its output's
 * cotangent), the init conv's dw0 / db0 (mask h0 > 0, times x; WaveNet.py:147,168) and final_conv.2's weight (sum relu(r) d_eps;
 * WaveNet.py:161-162).  (The FiLM cotangents are the same plain sum, handed out as fp64: ap_rowsum_f64.) */
int ap_rowsum(const float *A, const float *W, const float *R, float *out, int B, int M, int L, int w_broadcast, float scale,
              int accumulate, void *stream);
/* The plain sum (w = 1, scale 1) handed out as fp64: the FiLM cotangents dpart_n = sum du_n (WaveNet.py:82-84), which ap_embed_bwd
 * takes through long cancelling sums.  (ap_rowsum itself sums in fp64 too and rounds once on the way out.) */
int ap_rowsum_f64(const float *A, double *out, int B, int M, int L, int accumulate, void *stream);
/* Backward of ap_embed (util.py:68-93; WaveNet.py:82-83,124-126) with the context's loaded weights: from dpart [num_res_layers][C] (fp64:
 * ap_rowsum_f64; everything between it and the results is summed in fp64, so sub-batches add up to what one batch gives) and the
 * embedding ap_embed left behind its FiLM vectors (emb [embed_dim_out]):  d fc_t_n.weight = dpart_n (x) emb [NL][C][Eout], d fc_t_n.bias
 * [NL][C], then through swish(fc_t2(swish(fc_t1(.)))) (recomputed from `step`) the gradients of fc_t2 and fc_t1, each (+)= into buffers
 * shaped like the parameter.  scratch: ap_embed_bwd_scratch_elems(ctx) floats, 8-byte aligned. */
size_t ap_embed_bwd_scratch_elems(const ap_ctx *ctx);
int ap_embed_bwd(ap_ctx *ctx, float step, const double *dpart, const float *emb, float *d_fct_w, float *d_fct_b, float *d_fc1_w,
                 float *d_fc1_b, float *d_fc2_w, float *d_fc2_b, float *scratch, int accumulate, void *stream);
/* Gradient of the weight-norm fold W[o] = g[o] v[o] / ||v[o]|| (WaveNet.py:23-34, nn.utils.weight_norm dim = 0): from dW [rows][cols],
 *   dg[o] = (dW[o] . v[o]) / ||v[o]||,   dv[o] = (g[o] / ||v[o]||) (dW[o] - v[o] (dW[o] . v[o]) / ||v[o]||^2).
 * cols = 1 (the init conv): dv is exactly 0. */
int ap_weight_norm_bwd(const float *dW, const float *v, const float *g, float *dg, float *dv, int rows, int cols, void *stream);

/* ---- M5 in train mode: batch-statistics BatchNorm, parameter gradients (the reference trains the classifier:
 * audio_models/M5/train.py:86-103 `model.train(); loss = F.nll_loss(model(data), target); loss.backward()`, M5Net.py:21-38 with
 * nn.BatchNorm1d in training mode).  Stage i = 1..4: z = conv_i(a_{i-1}) + b_i; per channel over all n = B P_i positions the mean and
 * the BIASED variance; y = gamma (z - mean) / sqrt(var + eps) + beta; a_i = maxpool4(relu(y)) -- max and argmax on y, after the
 * affine, so a negative gamma is served; then the mean over time, fc1, log_softmax.  The handle supplies geometry and eps only: `blob`
 * is the LIVE parameter blob in ap_m5_create's order, read at every call; the folded images of the handle are never read.
 * Activations live in the caller's workspace (ap_m5_train_workspace_bytes; a launch allocates nothing), so there is no LDS ceiling on
 * L as in ap_m5_fwd / ap_m5_bwd.  -22 before any launch: L too short for four stages, n <= 1 values per channel, workspace too small.
 * No floating-point atomics: every sum over the batch runs in a fixed number of slices (64, whatever the card), each summed in a fixed
 * order, and the slices are added in fp64 and rounded once -- two runs give the same bits. */
/* elements of the gradient blob: per stage conv.weight, conv.bias, bn.weight, bn.bias, then fc1.weight, fc1.bias */
size_t ap_m5_param_elems(const ap_m5 *m);
size_t ap_m5_train_workspace_bytes(const ap_m5 *m, int B, int L);   /* 0 (error text set) where the shape is refused */
/* x [B][1][L] -> logprobs [B][n_output]; new_running [2 sum(co)]: the four stages' new running means, then their new running variances
 * ((1 - momentum) old + momentum batch value, the variance UNBIASED, n / (n - 1); torch's momentum=None is the host's momentum =
 * 1 / num_batches_tracked).  keep != 0 leaves in the workspace what ap_m5_train_bwd reads; keep = 0 is the no_grad form. */
int ap_m5_train_fwd(ap_m5 *m, const float *blob, const float *x, float *logprobs, float *new_running, float momentum, void *workspace,
                    size_t ws_bytes, int keep, int B, int L, void *stream);
/* After ap_m5_train_fwd(keep != 0) on the same blob, x and workspace: dlogprobs [B][n_output] -> grads [ap_m5_param_elems] (written,
 * not accumulated) and, if dx is not NULL, dx [B][1][L]. */
int ap_m5_train_bwd(ap_m5 *m, const float *blob, const float *x, const float *dlogprobs, float *grads, float *dx, void *workspace,
                    size_t ws_bytes, int B, int L, void *stream);

/* ---- train-mode step of the 2-D ConvNet classifiers (ap_convnet_train.hip).  The reference trains them with
 * audio_models/ConvNets_SpeechCommands/train_speech_commands.py:122-153 (model.train(), criterion(model(x), y), loss.backward(),
 * optimizer.step(); adv_train_speech_commands.py:191-225 likewise); its autograd forms what these entry points form.  Conv forward and
 * conv dx stay ap_conv2d_fwd, the biases ap_rowsum.  No floating-point atomics: every sum has a fixed order and a slice count that is a
 * constant, two runs give equal bits.  A launch allocates nothing; every refusal is -22 with ap_last_error set before any launch. ---- */
/* nn.Conv2d / nn.Linear weight gradient (the autograd of F.conv2d in models/resnext.py:39-51, resnet.py:84-103, wideresnet.py:28-41,
 * dpn.py:35-45, densenet.py:36-44 and of the classifiers' nn.Linear):
 *   dW[Cout][Cin/g][k][k] (+)= sum_{b,oh,ow} dy[b][m][oh][ow] x[b][g Cin/g + n][oh s + i - pad][ow s + j - pad], terms outside the image 0;
 * x = channels [x_coff, x_coff + Cin) of a tensor of x_cstride channels, dy [B][Cout][OH][OW] with OH = (H + 2 pad - k) / s + 1.
 * Square k in {1, 3, 7}, stride 1 or 2, 0 <= pad <= k - 1, groups dividing both channel counts; Cin = 1 and H = W = 1 (nn.Linear) are
 * ordinary cases.  Implicit GEMM on v_mfma_f32_32x32x2_f32 (per group rows Cout/g, columns (Cin/g) k k, contraction B OH OW), the
 * contraction split over workgroups into `workspace` (ap_conv2d_wgrad_workspace_bytes, 0 where the shape is refused) and added in
 * slice order by a second kernel. */
size_t ap_conv2d_wgrad_workspace_bytes(int B, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int groups);
int ap_conv2d_wgrad(const float *dy, const float *x, float *dW, void *workspace, size_t ws_bytes, int B, int Cin, int H, int W, int Cout,
                    int kh, int kw, int stride, int pad, int groups, int x_cstride, int x_coff, int accumulate, void *stream);
/* The A-operand image ap_conv2d_fwd reads for the conv's input gradient (the transposed convolution autograd runs for the same
 * F.conv2d calls), from the LIVE weight w [Cout][Cin/g][k][k]: taps flipped, in / out swapped within each group, i.e. ap_conv2d_pack of
 * wt[g Cin/g + n][m][i][j] = w[g Cout/g + m][n][k-1-i][k-1-j].  wT: ap_conv2d_packed_elems(groups Cin/g, Cout/g, k, k, groups) floats;
 * scratch: Cout Cin/g k k floats (receives wt). */
int ap_conv2d_pack_bwd(const float *w, float *wT, float *scratch, int Cout, int Cin_g, int kh, int kw, int groups, void *stream);
/* nn.BatchNorm2d in training mode (F.batch_norm(training=True) of the same model files, e.g. models/resnext.py:40-50) on x = channels
 * [x_coff, x_coff + C) of [B][x_cstride][HW].  Forward: per channel the mean and the biased variance over n = B HW values from 64 fixed
 * slices summed in fp64; y [B][C][HW] = gamma xhat + beta, ReLU'd if relu != 0; stat [2][C] = mean, 1 / sqrt(var + eps);
 * running_mean / running_var updated in place as (1 - momentum) old + momentum batch, the variance unbiased (n / (n - 1)).
 * Backward (y: the forward's output, read only when relu != 0; stat: the forward's): dy' = dy where y > 0 (all of dy without the ReLU),
 *   dbeta = sum dy', dgamma = sum dy' xhat, dx [B][C][HW] = gamma rstd (dy' - mean(dy') - xhat mean(dy' xhat));
 * dx, dgamma, dbeta may each be NULL.  gamma of either sign or 0 is served; n <= 1 is refused (torch raises there too).
 * workspace: ap_bn2d_train_workspace_bytes(C) bytes, 8-byte aligned. */
size_t ap_bn2d_train_workspace_bytes(int C);
int ap_bn2d_train_fwd(const float *x, const float *gamma, const float *beta, float *running_mean, float *running_var, float *y,
                      float *stat, void *workspace, size_t ws_bytes, int B, int C, int HW, int x_cstride, int x_coff, float eps,
                      float momentum, int relu, void *stream);
int ap_bn2d_train_bwd(const float *x, const float *y, const float *dy, const float *gamma, const float *stat, float *dx, float *dgamma,
                      float *dbeta, void *workspace, size_t ws_bytes, int B, int C, int HW, int x_cstride, int x_coff, int relu,
                      void *stream);

/* ---- train-mode step of the Improved-Diffusion UNet (ap_unet_train.hip).  The reference trains it with
 * improved_diffusion/train_util.py:191-229 (losses = diffusion.training_losses(ddp_model, micro, t); loss.backward()) at --dropout 0.3
 * (spect_train_mpi_run.sh:1-8); its autograd forms what these entry points form.  Conv / Linear dW are ap_conv2d_wgrad, their biases
 * ap_rowsum, the input-gradient sweep is ap_groupnorm_bwd's family.  Plain fp32; no floating-point atomics: every sum has a fixed
 * order, sums over the batch run in fp64 and round once, two runs give equal bits.  A launch allocates nothing; every refusal is -22
 * with ap_last_error set before any launch. ---- */
/* GroupNorm32 + scale-shift + activation backward with every cotangent (the autograd of nn.py:17-19 normalization, unet.py:186-190
 * `out_norm(h) * (1 + scale) + shift` and the SiLU behind it; unet.py:229 for the attention's norm, act 0).  Notation of
 * ap_groupnorm_bwd: xh = (x - mean) rstd over the (sample, group) slab, y0 = gamma xh + beta, y1 = y0 (1 + sc) + sh, y = act(y1)
 * (act 0 identity, 1 ReLU, 2 SiLU), e = dy act'(y1).  x, dy, dx [B][C][HW]; scale_shift and dss [B][2C] (scale first);
 *   dss[b][c] = sum_hw e y0,  dss[b][C + c] = sum_hw e,
 *   dbeta[c] = sum_b (1 + sc[b][c]) sum_hw e,  dgamma[c] = sum_b (1 + sc[b][c]) sum_hw e xh,  dx as ap_groupnorm_bwd forms it.
 * Each of dx, dgamma, dbeta, dss may be NULL (not all); scale_shift == NULL: sc = sh = 0 and dss must be NULL.  gamma of either sign
 * or 0 is served.  workspace: ap_groupnorm_train_workspace_bytes(B, C) bytes, 4-byte aligned, needed for dgamma / dbeta only. */
size_t ap_groupnorm_train_workspace_bytes(int B, int C);
int ap_groupnorm_train_bwd(const float *x, const float *gamma, const float *beta, const float *scale_shift, const float *dy, float *dx,
                           float *dgamma, float *dbeta, float *dss, void *workspace, size_t ws_bytes, int B, int C, int HW, int groups,
                           float eps, int act, void *stream);
/* nn.Dropout(p) in training mode (unet.py:150-160, the ResBlock's out_layers) on a counter-based mask that is never stored: element e
 * of sample b (n elements per sample) draws Philox4x32-10 with counter (e / 4, draw, low and high word of sample_offset + b), key =
 * the two words of seed, and takes word e % 4: u = (r >> 8) 2^-24; kept iff u >= p (fp32), y = x s with s = fp32(1 / (1 - p)), else 0.
 * The backward is the same call on dy; y may be x.  p = 0 copies bits; p outside [0, 1) is refused. */
int ap_dropout(const float *x, float *y, int B, int n, float p, uint64_t seed, uint32_t draw, uint64_t sample_offset, void *stream);
/* Backward of nn.py:12-14 SiLU (time_embed and emb_layers, unet.py:333-337,139-145): dx = dy s (1 + x (1 - s)), s = sigmoid(x). */
int ap_silu_bwd(const float *x, const float *dy, float *dx, size_t n, void *stream);
/* q_sample with one step per sample (gaussian_diffusion.py:188-206 with _extract_into_tensor's per-sample coefficients):
 * out[b] = a[b] x0[b] + b[b] z[b]; x0, z, out [B][n], a and b device rows [B]. */
int ap_qsample_rows(const float *x0, const float *z, const float *a, const float *b, float *out, int B, int n, void *stream);

/* ---- optimizer step (ap_optim.hip).  The reference's trainers end every iteration in torch.optim: Adam with coupled weight decay
 * (DiffWave_Unconditional/train.py:79, M5/train.py:51, RCNN_KWS/train.py:80, train_speech_commands.py:99), SGD(momentum 0.9,
 * weight_decay) (train_speech_commands.py:97) and AdamW (improved_diffusion/train_util.py:82); the UNet loop also walks every
 * parameter for the gradient norm (train_util.py:254-258, one host read per tensor) and for each EMA rate (nn.py:55-65).  These
 * entry points run all of it over a table of tensors: ceil(n_tensors / ap_optim_slab()) launches per call, the table in the kernel
 * arguments, no copy, no allocation, no synchronise.  fp32; the formulas are torch.optim's default single-tensor path, element by
 * element, with the scalars rounded to fp32 once and the roundings of torch's default path on the device (a rounding after each of
 * its operators, one fma inside add(alpha), lerp, addcmul and addcdiv, correctly rounded sqrt and divide): the results are
 * torch.optim's bit for bit; no atomics, two runs give equal bits.  Every refusal is -22 with ap_last_error set
 * before any launch. ---- */
#define AP_OPTIM_MAX_EMA 4
enum {
  AP_OPTIM_ADAM = 0,     /* g += wd p;  m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g g;
                            p -= step_size m / (sqrt(v) / sqrt_bc2 + eps) */
  AP_OPTIM_ADAMW = 1,    /* p *= 1 - lr wd first, then AP_OPTIM_ADAM's step with the bare gradient */
  AP_OPTIM_SGD = 2,      /* g += wd p;  momentum != 0: state1 = momentum state1 + g, g = state1;  p -= lr g   (dampening 0, no Nesterov;
                            state1 holds zeros before the first step) */
  AP_OPTIM_EMA_ONLY = 3  /* the EMA copies only: update_ema (nn.py:55-65) on its own; param is read, never written */
};
/* One tensor of the table; every pointer a device pointer to n contiguous fp32 elements at any 4-byte offset (16-byte loads and
 * stores where all of a tensor's pointers are 16-byte aligned, per element otherwise).  grad NULL: the parameter did not take part
 * in the backward; its state stays and only its EMA copies move (update_ema walks every parameter).  state1 / state2: exp_avg /
 * exp_avg_sq (Adam, AdamW), momentum_buffer / unused (SGD with momentum != 0; unused without).  ema[k], k < n_ema, after the update
 * and in the same pass: ema[k] = rate[k] ema[k] + (1 - rate[k]) p_new.  step_size = lr / (1 - beta1^t) and sqrt_bc2 =
 * sqrt(1 - beta2^t), formed by the caller in double and rounded: per tensor, because a parameter without a grad does not advance
 * its step count t.  Both unused by AP_OPTIM_SGD and AP_OPTIM_EMA_ONLY. */
typedef struct ap_optim_tensor {
  float *param;
  const float *grad;
  float *state1, *state2;
  float *ema[AP_OPTIM_MAX_EMA];
  uint64_t n;
  float step_size, sqrt_bc2;
} ap_optim_tensor;
/* The launch's hyper-parameters, in double as Python holds them; the library rounds each to fp32 once (1 - beta_i, 1 - lr wd and
 * 1 - rate formed in double first, as torch's scalar arguments are).  Refused: kind not one of AP_OPTIM_*, n_ema outside
 * [0, AP_OPTIM_MAX_EMA] (AP_OPTIM_EMA_ONLY: n_ema >= 1), a beta outside [0, 1), a negative lr, eps, weight_decay or momentum, an
 * ema_rate outside [0, 1], a null param, a null state tensor the kind needs, a null ema[k < n_ema]. */
typedef struct ap_optim_hyper {
  int32_t kind;                       /* AP_OPTIM_* */
  int32_t n_ema;
  double lr, beta1, beta2, eps, weight_decay, momentum;
  double ema_rate[AP_OPTIM_MAX_EMA];
} ap_optim_hyper;
/* Tensors per launch and elements per workgroup (a tensor of n elements is ceil(n / chunk) workgroups): where the kernel branches. */
int ap_optim_slab(void);
int ap_optim_chunk(void);
/* One step over `tensors` (a host array of n_tensors descriptors; n_tensors = 0 is a no-op). */
int ap_optim_step(const ap_optim_tensor *tensors, int n_tensors, const ap_optim_hyper *hp, void *stream);
/* out[0] = sum over the table of g^2 as one device double (the square of train_util.py:254-258's norm): each chunk sums its squares
 * in fp64 (an fp32 square is exact there) into `workspace`, one last workgroup adds the partials in a fixed order.  grads and n are
 * host arrays of n_tensors device pointers / element counts; workspace: ap_optim_sqnorm_workspace_bytes(n, n_tensors) bytes, 8-byte
 * aligned like out.  No host read: the caller reads the double when it needs it. */
size_t ap_optim_sqnorm_workspace_bytes(const uint64_t *n, int n_tensors);
int ap_optim_sqnorm(const float *const *grads, const uint64_t *n, int n_tensors, void *workspace, size_t ws_bytes, double *out,
                    void *stream);

/* ---- loss head: what train_speech_commands.py:131-163 runs between model(inputs) and optimizer.step().  Plain fp32 (expf / logf,
 * correctly rounded divide), no atomics, nothing allocated; every refusal is -22 with ap_last_error set before any launch. ---- */
/* Loss of B rows of K scores, the seed of loss.backward(), the predictions and the count of correct ones, in two launches (one wave
 * per row; one workgroup that adds the B row losses in fp64 in index order and counts: two runs give equal bits).
 *   mode 0  nn.CrossEntropyLoss():  row = logsumexp(in) - in[y] (row maximum subtracted first), loss = mean, din = (softmax - onehot) / B
 *   mode 1  mixup_cross_entropy_loss(in, soft) (mixup.py:17-29): p = softmax(in), row = -sum_i soft_i log(clamp(p_i, 1e-5, 1)),
 *           loss = sum / B, din_j = (-soft_j m_j + p_j sum_i soft_i m_i) / B with m_i = [1e-5 <= p_i <= 1], autograd's clamp
 *   mode 2  F.nll_loss on log-probabilities:  row = -in[y], din = -1 / B at y and 0 elsewhere
 * labels int64 [B] (modes 0, 2; in mode 1 optional, for n_correct only), soft [B][K] (mode 1).  loss_rows [B] and loss [1] are
 * written always; din [B][K], pred int64 [B] (the LOWEST index of the row maximum of `in`) and n_correct int64 [1] (#{pred ==
 * labels}; needs labels and pred) may each be NULL.  A label outside [0, K) makes its row's loss and din row NaN; nothing is read out
 * of bounds.  1 <= K <= 4096, 1 <= B <= 65535; din must not overlap in or soft.  No ignore_index, class weights or label smoothing. */
int ap_class_loss(const float *in, const int64_t *labels, const float *soft, int mode, float *loss_rows, float *loss, float *din,
                  int64_t *pred, int64_t *n_correct, int B, int K, void *stream);
/* mixup (mixup.py:40-52) on device tensors, with torch's fp32 rounding sequence -- omw = fl(1 - w), fl(fl(w a) + fl(omw c)), never an
 * fma -- so the bits are those of `weight * x1 + (1 - weight) * x2`:
 *   ap_mixup_rows     out[b] = w[b] x[b] + (1 - w[b]) x[index[b]], rows of n elements; out overlapping x is refused; an index outside
 *                     [0, B) writes NaN to that row
 *   ap_mixup_targets  out[b] = w[b] onehot(labels[b]) + (1 - w[b]) onehot(labels[index[b]]), [B][K]; an index or label out of range
 *                     writes NaN to that row */
int ap_mixup_rows(const float *x, const int64_t *index, const float *weight, float *out, int B, int n, void *stream);
int ap_mixup_targets(const int64_t *labels, const int64_t *index, const float *weight, float *out, int B, int K, void *stream);
/* out[i] = x[i] * fl(g[0] * factor) with g a DEVICE scalar (g NULL: x[i] * factor): din times the upstream cotangent of the scalar
 * loss without a host read.  out may be x. */
int ap_scale_by_scalar(const float *x, const float *g, float factor, float *out, size_t n, void *stream);

/* ---- train-time augmentation and mel features of the speech-commands classifiers (train_speech_commands.py:60-68), batched on the
 * device.  A lane is one clip or one background clip; every random number is drawn on the host and arrives as a per-lane DEVICE array
 * (int32 / float / double as typed).  fp32 data, complex values as (re, im) float pairs, STFTs laid out [lane][frame][1025 bins].
 * Nothing allocated, no synchronise, no atomics: two runs give equal bits.  A per-lane value out of range cannot be refused without
 * a host read; every index derived from one is clamped, so nothing is read or written out of bounds. ---- */
/* ChangeAmplitude, ChangeSpeedAndPitchAudio, FixAudioLength (transforms/transforms_wav.py:50-78,34-48) in one pass: x [N][L_max] with
 * len[N] valid samples each -> out [N][L_out],  out[j] = amp * np.interp(j * speed_fac, arange(len), x)  for j < n_interp (the host's
 * len(np.arange(0, len, speed_fac))), the position formed in fp64, positions in (len-1, len) taking x[len-1]; zeros from n_interp to
 * L_out, cut at L_out.  speed_applied[lane] == 0: out[j] = amp * x[j] for j < len, one fp32 rounding (speed_fac, n_interp unread). */
int ap_aug_wave(const float *x, const int32_t *len, const float *amp, const double *speed_fac, const int32_t *n_interp,
                const int32_t *speed_applied, float *out, int N, int L_max, int L_out, void *stream);
/* ToSTFT (transforms/transforms_stft.py:14-28): librosa.stft(x, n_fft=2048, hop_length=512) -- periodic Hann, center=True, F = 1 + L / 512
 * frames, complex64 -- of x [N][L] into out [N][F][1025][2].  pad_mode AP_PAD_CONSTANT (librosa >= 0.10; what ap_melspec_db assumes) or
 * AP_PAD_REFLECT (older librosa; needs L > 1024). */
#define AP_PAD_CONSTANT 0
#define AP_PAD_REFLECT 1
int ap_stft(const float *x, float *out, int pad_mode, int N, int L, void *stream);
/* StretchAudioOnSTFT, TimeshiftAudioOnSTFT, FixSTFTDimension (transforms/transforms_stft.py:30-68,86-99) fused: D [N][F][1025][2] ->
 * out, same shape.  stretch_applied[lane] != 0: S = librosa.core.phase_vocoder(D, rate, hop_length=512) with n_out =
 * len(np.arange(0, F, rate)) columns from the host, the step positions t * rate formed in fp64, the phase accumulator kept wrapped to
 * [-pi, pi] and the expected advance pi k / 2 applied as k mod 4 quarter turns; == 0: S = D (rate, n_out unread), copied bit for bit.
 * out[:, c] = S[:, c + shift] where c and c + shift are both columns of S, zeros elsewhere.  F <= 4096; out must not alias D. */
int ap_phase_vocoder_shift(const float *D, float *out, const double *rate, const int32_t *n_out, const int32_t *stretch_applied,
                           const int32_t *shift, int N, int F, void *stream);
/* AddBackgroundNoiseOnSTFT, ToMelSpectrogramFromSTFT (transforms/transforms_stft.py:70-84,101-114): for clip b < B of the N lanes of
 * D [N][F][1025][2]:  D[b] (1 - p[b]) + D[noise_lane[b]] p[b]  (noise_lane[b] outside [0, N): D[b] as it is), |.|^2, librosa.filters.mel
 * (sr=16000, n_fft=2048, n_mels) as ap_melspec_db builds it, librosa.power_to_db(ref=np.max) -> out [B][n_mels][F]. */
int ap_mel_from_stft(const float *D, const int32_t *noise_lane, const float *p, float *out, int n_mels, int B, int N, int F, void *stream);

/* ---- PGD attack loop (ap_attack.hip): what the reference's adversarial-training scripts run between two model calls of `pgd`
 * (audio_models/RCNN_KWS/train.py:84-121, audio_models/ConvNets_SpeechCommands/adv_train_speech_commands.py:139-183) and what stage 1
 * of the white-box attack runs (robustness_eval/white_box_attack.py:362-471).  The loop has no early exit, so with these it is enqueued
 * without a host read.  Rows are [B][n] fp32 ([B,1,L] waveforms); x, u, g, delta, x_pert and x_adv share the layout and a row may
 * start at any 4-byte offset (16-byte accesses where every row base allows).  Streaming kernels, one chunk of ap_pgd_chunk() elements
 * of a row per workgroup.  torch's fp32 rounding sequence, one rounding per operator and never an fma: the bits of the scripts' loops.
 * Nothing allocated, no synchronise, no atomics: two runs give equal bits.  Every refusal is -22 with ap_last_error set before any
 * launch.  1 <= B <= 65535, n >= 1; no output may overlap another tensor of the call. ---- */
int ap_pgd_chunk(void);
/* The random start (adv_train_speech_commands.py:146-148, RCNN_KWS/train.py:91-93), u the uniform draws of torch.rand_like:
 *   d = fl(eps fl(fl(2u) - 1)),  delta = fl(clamp(fl(x + d), -1, 1) - x),  x_pert = fl(x + delta)
 * u == NULL: stage 1's zero start (white_box_attack.py:378,384): delta = 0, x_pert = fl(x + 0).  One launch. */
int ap_pgd_init(const float *x, const float *u, float *delta, float *x_pert, float eps, int B, int n, void *stream);
/* One iteration's bookkeeping and linf update in ONE launch (adv_train_speech_commands.py:158-169, RCNN_KWS/train.py:103-113,
 * white_box_attack.py:399-407,442-453).  g is the gradient of the loss at x_pert.  The row's prediction is pred[b] (int64), or, with
 * pred NULL, the argmax of scores[b][0..K) taken by the kernel: the LOWEST index of the row maximum, a NaN counting as the maximum (as
 * Tensor.max does); exactly one of pred and scores is given, 1 <= K <= 4096.  For row b:
 *   hit = targeted ? pred == y[b] : pred != y[b];   hit: x_adv[b] = x_pert[b] (the iterate BEFORE the update) and found[b] = 1 --
 *         a later hit overwrites an earlier one, as the scripts' loops do
 *   last != 0: rows with found[b] == 0 get x_adv[b] = x_pert[b] (the fallback of :177-179 / :461-465); nothing else is written and g
 *         may be NULL
 *   otherwise: d = clamp(fl(delta + step sgn(g)), -eps_b, eps_b),  delta = fl(clamp(fl(x + d), -1, 1) - x),  x_pert = fl(x + delta)
 * step is signed: +alpha untargeted, -lr targeted.  sgn is torch.sign -- (0 < g) - (g < 0): +-0 and NaN give 0; clamp passes a NaN
 * on.  eps_b = eps_rows[b] (stage 1 keeps a bound per sample), or eps with eps_rows NULL.  found is uint8 [B], zeroed by the caller
 * before the first iteration. */
int ap_pgd_step_linf(const float *x, const float *g, float *delta, float *x_pert, float *x_adv, uint8_t *found, const int64_t *pred,
                     const float *scores, int K, const int64_t *y, float step, const float *eps_rows, float eps, int targeted, int last,
                     int B, int n, void *stream);
/* The same iteration with the l2 rule of adv_train_speech_commands.py:171 (project_to_norm_ball, :112-123), norms per row:
 *   g^ = g min(1, 1 / |g|_b),  v = delta + step g^,  d = v min(1, eps_b / |v|_b),  then the box step as above
 * THREE launches (one with last != 0): the squares of g summed per chunk, the squares of v per chunk (it adds the first launch's
 * partials of its row), the update (it adds both).  The partials are fp64 and are added in index order, the norm is rounded to fp32 as
 * torch.norm's is; the result is held to the float64 expression (measured: the same error as float32 torch's), not to torch's bits.  A row of zeros
 * behaves as torch's: 1 / 0 = inf, min(1, inf) = 1, no NaN appears.  workspace: ap_pgd_l2_workspace_bytes(B, n) bytes, 8-byte
 * aligned (unread with last != 0). */
size_t ap_pgd_l2_workspace_bytes(int B, int n);
int ap_pgd_step_l2(const float *x, const float *g, float *delta, float *x_pert, float *x_adv, uint8_t *found, const int64_t *pred,
                   const float *scores, int K, const int64_t *y, float step, const float *eps_rows, float eps, int targeted, int last,
                   void *workspace, size_t ws_bytes, int B, int n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AUDIOPURE_H */
