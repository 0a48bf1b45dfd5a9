// TEST-ONLY harness for tests/test_hostsim_shares.py: compiles the threshold-recovery headers (agora-blsful_amd/csrc/fr.cuh,
// shares.cuh) as plain host C++ with the bound tracker on, so that the `-m "not gpu"` suite checks the scalar-field arithmetic,
// the per-share Lagrange function and the per-share ladder without a GPU.  Never linked into libblsgpu.so.
#include <string.h>
#include "../../agora-blsful_amd/csrc/verify.cuh"
#include "../../agora-blsful_amd/csrc/msm2.cuh"
#include "../../agora-blsful_amd/csrc/shares.cuh"

static void ld_fr(fr& a, const uint32_t* w) { for (int j = 0; j < 8; j++) a.w[j] = w[j]; }
static void st_fr(uint32_t* w, const fr& a) { for (int j = 0; j < 8; j++) w[j] = a.w[j]; }

extern "C" {
// raw Montgomery product a b / 2^256 mod r (a < 2^256, b < r)
void hs_fr_mont_mul(const uint32_t* a, const uint32_t* b, uint32_t* out) {
  fr x, y, r;
  ld_fr(x, a); ld_fr(y, b); fr_mul(r, x, y); st_fr(out, r);
}
// on canonical values (through the Montgomery form): op 0: a b, 1: a - b, 2: a^-1, 3: a mod r (to and from the form)
void hs_fr_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  fr x, y, r;
  fr_to_mont(x, a);
  fr_to_mont(y, b);
  if (op == 0) fr_mul(r, x, y);
  else if (op == 1) fr_sub(r, x, y);
  else if (op == 2) fr_inv(r, x);
  else r = x;
  fr_from_mont(out, r);
}
int hs_fr_canonical(const uint32_t* a) { return fr_words_canonical(a) ? 1 : 0; }
// lambda_i of share i of a set of t identifiers (any 256-bit values); returns the share's VSSS flag
uint32_t hs_lagrange(const uint32_t* ids, int t, int i, uint32_t* lam) {
  fr xi, xj;
  fr_to_mont(xi, ids + 8 * i);
  share_lagrange L;
  share_lagrange_init(L);
  for (int j = 0; j < t; j++) {
    if (j == i) continue;
    fr_to_mont(xj, ids + 8 * j);
    share_lagrange_acc(L, xi, xj);
  }
  return share_lagrange_fin(lam, L, xi);
}
void hs_naf(const uint64_t* k, int words, uint64_t* pos, uint64_t* neg) { share_naf(pos, neg, k, words); }
// lambda P (P raw Jacobian, may be the identity) by the joint ladder -> compressed
void hs_share_ladder(int group, const uint32_t* p, const uint32_t* lam, uint8_t* out) {
  if (group == 1) {
    g1_jac a, r; g1_aff f;
    fp_from_raw(a.x, p); fp_from_raw(a.y, p + 12); fp_from_raw(a.z, p + 24);
    jac_to_aff(f, a);
    share_ladder<1>(r, f, lam);
    jac_to_aff(f, r);
    g1_compress(out, f, false);
  } else {
    g2_jac a, r; g2_aff f;
    fp_from_raw(a.x.c0, p); fp_from_raw(a.x.c1, p + 12); fp_from_raw(a.y.c0, p + 24); fp_from_raw(a.y.c1, p + 36);
    fp_from_raw(a.z.c0, p + 48); fp_from_raw(a.z.c1, p + 60);
    jac_to_aff(f, a);
    share_ladder<2>(r, f, lam);
    jac_to_aff(f, r);
    g2_compress(out, f, false);
  }
}
}
