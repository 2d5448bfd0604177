// The residual block's dispatch plan (audiopure_amd/csrc/ap_block_plan.h) behind a C ABI, for tests/test_block_plan_cpu.py and
// tools/block_dispatch_cases.py: host compiler only, nothing of the GPU library.  With -DDRIVER_MAIN a stand-alone program that plans
// every ask of a text file (one per line: the 20 values of ap_block) and checks the sweep invariants -- the form that runs under
// -fsanitize=address,undefined.
#include <stdio.h>

#include "../audiopure_amd/csrc/ap_block_plan.h"

using namespace ap;

// in: precision C S NL cycle f32_form w1w w1w_s w2p_bf wf1p_bf layer B L n_cu hout skip aout gout fout u
static BlockAsk ask_of(const long long *in) {
  return BlockAsk{(int)in[0], (int)in[1], (int)in[2], (int)in[3], (int)in[4], (int)in[5], in[6] != 0, in[7] != 0, in[8] != 0, in[9] != 0,
                  (int)in[10], (int)in[11], (int)in[12], (int)in[13], in[14] != 0, in[15] != 0, in[16] != 0, in[17] != 0, in[18] != 0, in[19] != 0};
}

// out: rc family tile save noh q16 dcls diet ws rag ds savef e4 d logd np ntiles ntiles2 nblk nblk2 grid grid2 wg (23 values);
// err: the refusal's text as set_error would format it ("" where rc == 0)
extern "C" int ap_block(const long long *in, long long *out, char *err, int err_len) {
  BlockPlan p;
  const int rc = block_plan(ask_of(in), BlockTune{}, &p);
  const long long v[23] = {rc, p.family, p.tile, p.save, p.noh, p.q16, p.dcls, p.diet, p.ws, p.rag, p.ds, p.savef, p.e4, p.d, p.logd, p.np,
                           p.ntiles, p.ntiles2, p.nblk, p.nblk2, p.grid, p.grid2, p.wg};
  for (int i = 0; i < 23; i++) out[i] = v[i];
  if (err && err_len > 0) {
    err[0] = 0;
    if (rc && p.err) snprintf(err, (size_t)err_len, p.err, p.err_arg[0], p.err_arg[1], p.err_arg[2]);
  }
  return rc;
}

extern "C" int ap_block_drops_last_h(const long long *in) { return block_drops_last_h(ask_of(in), BlockTune{}); }

// out: rc rag ntiles nblk grid wg; err as above (null: not wanted)
extern "C" int ap_skipgemm(const long long *in, int layer0, int nl, long long *out, char *err, int err_len) {
  BlockPlan p;
  const int rc = skipgemm_plan(ask_of(in), layer0, nl, &p);
  if (err && err_len > 0) err[0] = 0;
  if (err && err_len > 0 && rc) snprintf(err, (size_t)err_len, p.err, p.err_arg[0], p.err_arg[1], p.err_arg[2], p.err_arg[3]);
  const long long v[6] = {rc, p.rag, p.ntiles, p.nblk, p.grid, p.wg};
  for (int i = 0; i < 6; i++) out[i] = v[i];
  return rc;
}

// out: rc bf16 S tile ntiles grid wg; err as above
extern "C" int ap_final(const long long *in, long long *out, char *err, int err_len) {
  BlockPlan p;
  const int rc = final_plan(ask_of(in), &p);
  if (err && err_len > 0) err[0] = 0;
  if (err && err_len > 0 && rc) snprintf(err, (size_t)err_len, p.err, p.err_arg[0]);
  const long long v[7] = {rc, p.family == BLOCK_FINAL_BF16, in[2], p.tile, p.ntiles, p.grid, p.wg};
  for (int i = 0; i < 7; i++) out[i] = v[i];
  return rc;
}

#ifdef DRIVER_MAIN
int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!f) { fprintf(stderr, "usage: %s <sweep file>\n", argv[0]); return 2; }
  long long in[20], o[23], s[6];
  char err[512];
  int n = 0, bad = 0, refused = 0;
  for (;;) {
    int got = 0;
    while (got < 20 && fscanf(f, "%lld", in + got) == 1) got++;
    if (got < 20) break;
    n++;
    const BlockAsk a = ask_of(in);
    if (const int rc = ap_block(in, o, err, (int)sizeof err)) {
      refused++;
      bad += rc != -22 || !err[0];
      continue;
    }
    const int fam = (int)o[1];
    const long long cap = o[18] < a.n_cu ? o[18] : a.n_cu;
    bad += !o[20] || !o[22] || (fam == BLOCK_SPLIT_F23 && !o[21]);                                          // no zero grid dimension
    bad += (fam == BLOCK_F32_F23 || fam == BLOCK_BF16_P || fam == BLOCK_BF16U_P) && o[20] > cap;   // never above min(nblk, CUs)
    bad += (fam == BLOCK_BF16_S || fam == BLOCK_BF16U_S) && (long long)a.B * ((a.L + 127) / 128) > 256;       // small-tile rule
    bad += o[4] && a.hout;                                                                                   // NOH only without h'
    bad += (o[3] && !a.aout) || (o[11] && !a.fout);                                                          // SAVE / SAVEF only with the buffer
    bad += (fam == BLOCK_F32_F23 || fam == BLOCK_SPLIT_F23) &&
           !(a.C == 256 && a.S == 256 && a.f32_form == 1 && (fam == BLOCK_F32_F23 ? a.w1w : a.w1w_s));     // F(2,3) only where built
    if (a.gout && !ap_skipgemm(in, 0, 1, s, nullptr, 0)) bad += !s[4] || s[4] > (s[3] < a.n_cu ? s[3] : a.n_cu);
  }
  fclose(f);
  printf("%d asks planned, %d refused, %d invariant violations\n", n, refused, bad);
  return bad ? 1 : 0;
}
#endif
