// ap_conv2d_fwd's dispatch as a pure function: which kernel serves a layer, on which tile, with which grid.  Host-only (no HIP header,
// plain g++ -std=c++17 compiles it), so the rule that carries the conv throughput is pinned on the CPU: tests/test_conv_plan_cpu.py
// against tests/golden/conv_dispatch_v1.json.  ap_convnet.hip builds a ConvGeom, asks conv_plan and launches what the plan says.
#pragma once
#include <stddef.h>

namespace ap {
// thresholds (swept: profiles/, tools/sweep_conv_*.py) and switches: constexpr in the product, written by ap_debug_conv_* in the -DAP_TOOLS build
struct ConvTune {
  int no_frag = 0;                  // ap_debug_conv_path(1): timing A/B against the LDS-staged 128 x 128 kernel
  long long frag_min_tiles = 512;   // below two 128 x 128 tiles per CU the 128 x 64 variant wins (swept)
  int wide_1x1 = 0;                 // ap_debug_conv_path(2): pointwise layers on 128 x 128 tiles again (A/B)
  int force = 0;                    // ap_debug_conv_path(4..7): every streamed-weight layer on 128x128 / 128x64 / 64x64 / 64x128 tiles; 8: off
  int w3 = 1;                       // ap_debug_conv_w3(on, min_pairs): the F(2,3) kernel for the layers it serves / the direct kernels
  long long w3_min_pairs = 0;       //   (w3 == 2: every served layer, worth it or not)
  int w3_split = 1;                 // ap_debug_conv_w3(on + 4 * nosplit, ..): K slices for the low-resolution maps on / off
  int p1 = 0;                       // ap_debug_conv_p1(1): try the LDS-free pointwise kernel of tools/csrc/ap_conv_p1.hip first (A/B: slower)
  long long splitk_t2 = 384;        // ap_debug_conv_splitk: split-K is taken below this many half-tiles (2 x 128 x 128 tiles)
  int splitk_cap = 768;             // ... and slices are doubled while tiles x slices stays below this
};

// ---- ap_conv_w3.hip: 3 x 3 / stride 1 / pad 1 / ungrouped layers in F(2,3) form along W ----
inline bool conv_w3_serves(int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int groups) {
  return kh == 3 && kw == 3 && stride == 1 && pad == 1 && groups == 1 && Cin % 32 == 0 && Cout % 128 == 0 && (W & 1) == 0 && W >= 2 && H >= 1;
}
inline size_t conv_w3_elems(int Cout, int Cin) { return (size_t)4 * Cout * Cin * 3; }
// rows per workgroup: 256 (RT = 2 row tiles per wave) where Cout allows it, else 128 (RT = 1, four column tiles per wave)
inline int conv_w3_rt(int Cout) { return Cout % 256 == 0 ? 2 : 1; }
// persistent one-workgroup-per-CU kernel: worth it from two tiles per CU on (measured at B = 256: the UNet's 32 x 32 and 16 x 16 maps
// 1.15-1.36 x faster than the direct kernels, its 8 x 8 / 4 x 4 maps -- 128 / 32 tiles -- 1.15-3 x slower: those keep the direct kernels)
inline long long conv_w3_tiles(int B, int H, int W, int Cout) {
  const int rt = conv_w3_rt(Cout), ncol = rt == 2 ? 64 : 128;
  return (long long)(Cout / (128 * rt)) * (((long long)B * H * (W / 2) + ncol - 1) / ncol);
}
inline bool conv_w3_worth(int B, int H, int W, int Cout) { return conv_w3_tiles(B, H, W, Cout) >= 512; }
// K slices for a layer with too few tiles (the UNet's 8 x 8 and 4 x 4 maps: 128 / 32 tiles): each slice sums its share of the
// (ky, channel-block) chunks and writes its TRANSFORMED partial outputs (the output transform is linear) to the caller's
// workspace; the conv launcher's reduce kernel adds the slices in order (deterministic), then bias / residual / ReLU.
// 0: not worth it (under 32 tiles, or fewer than 3 chunks per slice)
inline int conv_w3_splits(int B, int Cin, int H, int W, int Cout, size_t ws_bytes) {
  const long long t = conv_w3_tiles(B, H, W, Cout), nch = 3 * (Cin / 32);
  if (t >= 512 || t < 32) return 0;
  int S = 2;
  while (S < 8 && t * S < 512) S *= 2;
  while (S > 1 && (nch / S < 3 || (size_t)S * B * Cout * H * W * sizeof(float) > ws_bytes)) S /= 2;
  return S > 1 ? S : 0;
}

// ---- the packed weight buffer: [transposed image][A fragments][3 x bf16 fragments][2 x fp16 fragments][F(2,3) image], each image
// 16-byte aligned; offsets in floats.  ap_conv2d_packed_elems, ap_conv2d_pack and the launcher all read them here.
struct ConvImages {
  bool has_frag, has_w3;            // layers the streamed-weight kernel serves carry the three fragment images, F(2,3) layers the last one
  size_t frag_elems;                // floats of the fp32 fragment image (rows padded to 32)
  size_t frag, split, splith, w3, total;   // offsets (valid where the image exists)
};
inline ConvImages conv_images(int Cout, int Cin_g, int kh, int kw, int groups) {
  const auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
  ConvImages im{};
  im.has_frag = Cin_g % 16 == 0 && Cout / groups >= 64;
  im.has_w3 = conv_w3_serves(Cin_g, 4, 4, Cout, kh, kw, 1, 1, groups);   // the weight-side conditions (3 x 3, ungrouped, Cin % 32, Cout % 128)
  im.frag_elems = (size_t)groups * ((Cout / groups + 31) / 32) * 32 * Cin_g * kh * kw;
  im.total = (size_t)Cout * Cin_g * kh * kw;
  if (im.has_frag) {
    im.frag = up4(im.total);
    im.split = im.frag + im.frag_elems;
    im.splith = im.split + up4(im.frag_elems * 3 / 2);                  // 3 x bf16 per weight = 1.5 floats, whole float4s
    im.total = im.splith + up4(im.frag_elems);                          // 2 x fp16 per weight = 1 float
  }
  if (im.has_w3) { im.w3 = up4(im.total); im.total = im.w3 + conv_w3_elems(Cout, Cin_g); }
  return im;
}

// ---- one layer's geometry; the ONLY decoder of ap_conv2d_fwd's flag word: bit 0 ReLU, bit 8 AP_CONV_SPLIT, bit 10 AP_CONV_SPLIT_F16,
// bit 9 AP_CONV_1D (padding and dilation apply to W only: Conv1d over [B][C][1][L]), bits 16-31 dilation (0 = 1)
struct ConvGeom {
  int B, Cin, H, W, Cout, kh, kw, stride, pad, groups, x_cstride;
  int relu, dil_w, dil_h, pad_h, Ho, Wo, Mg, o_cstride, o_coff;    // o_cstride / o_coff: the output slice (Cout / 0: the whole tensor)
  bool split, splith, one_d, sliced;
  long long N;                                                     // output pixels B Ho Wo
};
inline ConvGeom conv_geom(int B, int Cin, int H, int W, int Cout, int kh, int kw, int stride, int pad, int groups, int flags, int x_cstride,
                          int o_cstride, int o_coff) {
  ConvGeom g{};
  g.B = B; g.Cin = Cin; g.H = H; g.W = W; g.Cout = Cout; g.kh = kh; g.kw = kw; g.stride = stride; g.pad = pad; g.groups = groups; g.x_cstride = x_cstride;
  g.relu = flags & 1; g.split = (flags >> 8) & 1; g.one_d = (flags >> 9) & 1; g.splith = (flags >> 10) & 1;
  g.dil_w = (flags >> 16) ? (flags >> 16) : 1;
  g.dil_h = g.one_d ? 1 : g.dil_w; g.pad_h = g.one_d ? 0 : pad;
  g.Ho = (H + 2 * g.pad_h - g.dil_h * (kh - 1) - 1) / stride + 1;
  g.Wo = (W + 2 * pad - g.dil_w * (kw - 1) - 1) / stride + 1;
  g.N = (long long)B * g.Ho * g.Wo; g.Mg = Cout / groups;
  g.o_cstride = o_cstride ? o_cstride : Cout; g.o_coff = o_cstride ? o_coff : 0;
  g.sliced = g.o_cstride != Cout || g.o_coff != 0;
  return g;
}

enum ConvFamily {
  CONV_GENERIC,   // conv2d_f32_kernel, 64 x 64 LDS-staged: everything nothing else serves
  CONV_FEW,       // conv2d_few_kernel<Cout, 3 x 3 undilated>: one thread per pixel, Cout <= 4, weights in dynamic LDS
  CONV_BIG,       // conv2d_f32_big_kernel, LDS-staged 128 x 128 (no fragment image)
  CONV_BIG2,      // conv2d_f32_big2_kernel<BM, BN, buf, p1>: the streamed-weight fp32 kernel
  CONV_SPLIT,     // conv2d_split_kernel<BM, 128>: three bf16 parts per operand (AP_CONV_SPLIT)
  CONV_SPLITH,    // conv2d_split_kernel<BM, 128, true>: two fp16 parts (AP_CONV_SPLIT_F16)
  CONV_W3,        // ap_conv_w3.hip conv2d_w3_kernel<BM / 128, nb>: F(2,3), persistent
  CONV_P1         // tools/csrc/ap_conv_p1.hip (-DAP_TOOLS, ap_debug_conv_p1): never planned, tried first where ConvPlan::try_p1
};
// ap_conv_profile_read's class of a launch -- the one table: 0 streamed-weight 128 x 128; 1 streamed-weight 64 x 128; 2 streamed-weight
// 128 x 64 and 64 x 64, which includes every split-K launch (and, tools, every forced tile); 3 bf16- / fp16-split; 4 LDS-staged
// 128 x 128; 5 generic and few-output; 6 F(2,3), K-sliced or not; 7 the tools build's pointwise kernel
inline int conv_class(int family, int BM, int BN) {
  if (family == CONV_BIG2) return BN == 64 ? 2 : BM == 128 ? 0 : 1;
  return family == CONV_SPLIT || family == CONV_SPLITH ? 3 : family == CONV_BIG ? 4 : family == CONV_W3 ? 6 : family == CONV_P1 ? 7 : 5;
}
struct ConvPlan {
  int family, BM, BN;               // kernel and workgroup tile, rows x pixel columns (CONV_FEW: BM = Cout; CONV_W3: 128 RT x pair columns)
  bool buf, p1;                     // CONV_BIG2: buffer-load form (x slab and fragment image below 2 GB each); 16-byte pointwise staging
  bool k3_nb;                       // CONV_FEW: the 3 x 3 undilated instantiation; CONV_W3: the neighbour staging form
  bool try_p1;                      // tools: launch_conv_p1 first, this plan if it declines
  int splits;                       // K slices (1: none); > 1: raw partial sums [splits][B][Cout][Ho][Wo] go to the workspace ...
  bool reduce;                      // ... and conv_splitk_reduce_kernel follows (bias / residual / ReLU move there)
  unsigned grid[3];                 // CONV_W3: grid[0] = tiles; the launch takes min(tiles, CUs of the device)
  size_t lds, xbytes, abytes;       // dynamic LDS bytes; CONV_BIG2: bytes of the x slab and of the fragment image
  int cls;
  const char *err;                  // the refusal's text where conv_plan returns non-zero
};

// The whole decision.  ws_bytes: the split-K workspace registered for the launching device (0: none -- such a layer runs un-split).
inline int conv_plan(const ConvGeom &g, const ConvImages &im, const ConvTune &t, size_t ws_bytes, ConvPlan *p) {
  *p = ConvPlan{}; p->splits = 1;
  if (g.Ho < 1 || g.Wo < 1) { p->err = "ap_conv2d_fwd: empty output"; return -22; }
  const bool splitop = g.split || g.splith, frag = im.has_frag && !t.no_frag;
  if (g.sliced && !(frag && !splitop)) {
    p->err = "ap_conv2d_fwd_slice: this layer is not served by the streamed-weight fp32 kernel (Cin/g % 16, Cout/g >= 64, no split-operand flag)";
    return -22;
  }
  const long long N = g.N, G = g.groups, Mg = g.Mg, kchunks = (long long)g.kh * g.kw * (g.Cin / 16);
  const size_t GB2 = (size_t)1 << 31, hw4 = (size_t)g.H * g.W * sizeof(float), obytes = (size_t)g.B * g.Cout * g.Ho * g.Wo * sizeof(float);
  const auto tiles = [&](int bm, int bn) { return ((N + bn - 1) / bn) * ((Mg + bm - 1) / bm); };
  const auto take = [&](int family, int bm, int bn, long long z) {
    p->family = family; p->BM = bm; p->BN = bn; p->cls = conv_class(family, bm, bn);
    p->grid[0] = (unsigned)((N + bn - 1) / bn); p->grid[1] = (unsigned)((Mg + bm - 1) / bm); p->grid[2] = (unsigned)z;
    return 0;
  };
  if (t.w3 && !splitop && !g.one_d && g.dil_w == 1 && conv_w3_serves(g.Cin, g.H, g.W, g.Cout, g.kh, g.kw, g.stride, g.pad, g.groups) &&
      (size_t)g.B * g.x_cstride * hw4 < GB2 && (size_t)g.B * g.o_cstride * hw4 < GB2 && (long long)g.B * g.H * (g.W / 2) >= t.w3_min_pairs) {
    // too few tiles for one workgroup per CU (the UNet's 8 x 8 and 4 x 4 maps): K slices into the caller's workspace, summed in
    // order by the reduce kernel -- deterministic; neither worth it nor sliceable (S = 0): the direct kernels below
    const bool whole = t.w3 == 2 || conv_w3_worth(g.B, g.H, g.W, g.Cout);
    const int S = whole ? 1 : (t.w3_split && ws_bytes) ? conv_w3_splits(g.B, g.Cin, g.H, g.W, g.Cout, ws_bytes) : 0;
    if (S >= 1) {
      const int rt = conv_w3_rt(g.Cout), w2 = g.W / 2;
      take(CONV_W3, 128 * rt, rt == 2 ? 64 : 128, 1);
      p->grid[0] = (unsigned)(conv_w3_tiles(g.B, g.H, g.W, g.Cout) * S); p->grid[1] = 1;
      p->k3_nb = w2 <= 64 && (w2 & (w2 - 1)) == 0;       // whole image rows per 64 staging lanes
      p->splits = S; p->reduce = S > 1;
      return 0;
    }
  }
  if (frag) {
    // buffer-load form of the fp32 kernel: the activations' slab and the fragment image each below 2 GB (32-bit offsets,
    // bit 31 marks the padding taps); larger tensors keep the pointer form
    p->xbytes = (size_t)g.B * g.x_cstride * hw4;
    p->abytes = im.frag_elems * sizeof(float);
    const bool buf = p->buf = p->xbytes < GB2 && p->abytes < GB2, pointwise = g.kh == 1 && g.kw == 1;
    const bool p1 = pointwise && g.stride == 1 && g.pad == 0 && !g.one_d && (g.H * g.W) % 4 == 0;   // pointwise: 16-byte staging
    p->try_p1 = t.p1 && p1 && buf && !splitop;
    if (splitop) return take(g.splith ? CONV_SPLITH : CONV_SPLIT, Mg < 128 ? 64 : 128, 128, G);
    if (t.force && buf && G == 1) {                      // tools: one tile shape for every layer (sweeps), all of them class 2
      take(CONV_BIG2, t.force == 4 || t.force == 5 ? 128 : 64, t.force == 4 || t.force == 7 ? 128 : 64, 1);
      p->p1 = p1; p->cls = 2;
      return 0;
    }
    if (Mg < 128) return take(CONV_BIG2, 64, 128, G);    // 64 <= Cout/g < 128
    p->p1 = buf && p1;                                   // (not on the split-K tiles)
    // the 128 x 128 tile needs enough workgroups to fill 256 CUs (pointwise layers: 128 x 64 below)
    if (tiles(128, 128) * G >= t.frag_min_tiles && !(pointwise && !t.wide_1x1)) return take(CONV_BIG2, 128, 128, G);
    if (buf && G == 1 && tiles(128, 128) * 2 < t.splitk_t2 && kchunks >= 32 && 2 * obytes <= ws_bytes) {
      // too few output tiles for 256 CUs and a long K (the 4 x 4 and 8 x 8 maps of the UNet: K = 2 304 .. 4 608): split-K over
      // blockIdx.z, partial sums to the caller's workspace, slices summed in order by a second small kernel (deterministic)
      const bool small = tiles(128, 64) < 192;
      const long long nt = small ? tiles(64, 64) : tiles(128, 64);
      int S = 2;
      while (S < 8 && nt * S < t.splitk_cap && kchunks / (2 * S) >= 16 && (size_t)(2 * S) * obytes <= ws_bytes) S *= 2;
      p->splits = S; p->reduce = true; p->p1 = false;
      return take(CONV_BIG2, small ? 64 : 128, 64, S);
    }
    if (tiles(128, 64) * G >= 192) return take(CONV_BIG2, 128, 64, G);   // few tiles (low-resolution layers): 128 x 64
    p->p1 = false;
    return take(CONV_BIG2, 64, 64, G);                   // fewer still (4 x 4 maps, the embedding's linear layers): twice the workgroups
  }
  const size_t wbytes = (size_t)g.Cin * g.kh * g.kw * g.Cout * sizeof(float);
  if (G == 1 && g.Cout <= 4 && wbytes <= 48 * 1024) {
    p->lds = wbytes; p->k3_nb = g.kh == 3 && g.kw == 3 && g.dil_h == 1 && g.dil_w == 1;
    return take(CONV_FEW, g.Cout, 256, 1);
  }
  if (Mg >= 128 && g.kh <= 3 && g.kw <= 3 && tiles(128, 128) * G >= 512) return take(CONV_BIG, 128, 128, G);
  return take(CONV_GENERIC, 64, 64, G);
}

}  // namespace ap
