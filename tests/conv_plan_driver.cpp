// The conv dispatch plan (audiopure_amd/csrc/ap_conv_plan.h) behind a C ABI, for tests/test_conv_plan_cpu.py and
// tools/conv_dispatch_cases.py: host compiler only, nothing of the GPU library.  With -DDRIVER_MAIN a stand-alone program that plans
// every shape of a text file (one shape per line: the 14 ints of ap_plan + ws_bytes) and checks the sweep invariants -- the form
// that runs under -fsanitize=address,undefined.
#include <stdio.h>

#include "../audiopure_amd/csrc/ap_conv_plan.h"

using namespace ap;

// in: B Cin H W Cout kh kw stride pad groups flags x_cstride o_cstride o_coff.  out: rc family BM BN buf p1 k3_nb splits reduce
// grid[3] lds cls Ho Wo (16 values)
extern "C" int ap_plan(const int *in, long long ws_bytes, long long *out) {
  const ConvGeom g = conv_geom(in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], in[10], in[11], in[12], in[13]);
  const ConvImages im = conv_images(in[4], in[1] / in[9], in[5], in[6], in[9]);
  ConvPlan p;
  const int rc = conv_plan(g, im, ConvTune{}, (size_t)ws_bytes, &p);
  const long long v[16] = {rc, p.family, p.BM, p.BN, p.buf, p.p1, p.k3_nb, p.splits, p.reduce, p.grid[0], p.grid[1], p.grid[2],
                           (long long)p.lds, p.cls, g.Ho, g.Wo};
  for (int i = 0; i < 16; i++) out[i] = v[i];
  return rc;
}

// out: has_frag has_w3 frag_elems frag split splith w3 total
extern "C" void ap_plan_images(int Cout, int Cin_g, int kh, int kw, int groups, long long *out) {
  const ConvImages im = conv_images(Cout, Cin_g, kh, kw, groups);
  const long long v[8] = {im.has_frag, im.has_w3, (long long)im.frag_elems, (long long)im.frag, (long long)im.split, (long long)im.splith,
                          (long long)im.w3, (long long)im.total};
  for (int i = 0; i < 8; i++) out[i] = v[i];
}

#ifdef DRIVER_MAIN
int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: %s <sweep file>\n", argv[0]); return 2; }
  int in[14], n = 0, bad = 0;
  long long ws, o[16];
  while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld", in, in + 1, in + 2, in + 3, in + 4, in + 5, in + 6, in + 7, in + 8, in + 9,
                in + 10, in + 11, in + 12, in + 13, &ws) == 15) {
    n++;
    if (ap_plan(in, ws, o)) continue;
    const long long part = o[7] > 1 ? o[7] * in[0] * (long long)in[4] * o[14] * o[15] * 4 : 0;
    const bool sliced = in[12] && (in[12] != in[4] || in[13]);
    bad += part > ws || (o[7] > 1 && in[9] > 1) || (sliced && o[1] != CONV_BIG2 && o[1] != CONV_W3) || !o[9] || !o[10] || !o[11];
  }
  fclose(f);
  printf("%d shapes planned, %d invariant violations\n", n, bad);
  return bad ? 1 : 0;
}
#endif
