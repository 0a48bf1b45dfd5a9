// TEST-ONLY harness for tests/test_hostsim_elgamal.py: compiles the ElGamal device functions (agora-blsful_amd/csrc/elgamal.cuh,
// fr.cuh) as plain host C++ with the bound tracker on, so that the `-m "not gpu"` suite checks STROBE / Merlin, the 512-bit
// reduction, the shared-inversion affine conversion and the multi-term joint ladder without a GPU.  Never linked into libblsgpu.so.
#include <string.h>
#include "../../agora-blsful_amd/csrc/verify.cuh"
#include "../../agora-blsful_amd/csrc/msm2.cuh"
#include "../../agora-blsful_amd/csrc/elgamal.cuh"

static void ld_jac(g1_jac& a, const uint32_t* p) {
  fp_from_raw(a.x, p); fp_from_raw(a.y, p + 12); fp_from_raw(a.z, p + 24);
}
static void ld_jac(g2_jac& a, const uint32_t* p) {
  fp_from_raw(a.x.c0, p); fp_from_raw(a.x.c1, p + 12); fp_from_raw(a.y.c0, p + 24); fp_from_raw(a.y.c1, p + 36);
  fp_from_raw(a.z.c0, p + 48); fp_from_raw(a.z.c1, p + 60);
}
static void compress(uint8_t* out, const g1_aff& a) { g1_compress(out, a, false); }
static void compress(uint8_t* out, const g2_aff& a) { g2_compress(out, a, false); }

// sum_t k_t P_t by the joint ladder; P_t raw Jacobian, none the identity -> compressed
template <int G, class J>
static void ladder(int terms, const uint32_t* pts, const uint32_t* ks, uint8_t* out) {
  typedef typename elgamal_terms<G>::F F;
  J p[ELGAMAL_MAX_TERMS], r;
  aff<F> a[ELGAMAL_MAX_TERMS], ra;
  for (int t = 0; t < ELGAMAL_MAX_TERMS; t++) ld_jac(p[t], pts + (t < terms ? t : 0) * 36 * G);
  elgamal_to_aff<ELGAMAL_MAX_TERMS>(a, p);
  elgamal_terms<G> S;
  S.terms = terms;
  for (int t = 0; t < terms; t++) {
    elgamal_term_point<G>(S, t, a[t]);
    elgamal_term_scalar<G>(S, t, ks + 8 * t);
  }
  elgamal_ladder<G>(r, S);
  jac_to_aff(ra, r);
  compress(out, ra);
}

extern "C" {
uint64_t hs_keccak_f0(void) {
  keccak_state st;
  for (int k = 0; k < 25; k++) st.s[k] = 0;
  keccak_f1600(st);
  return st.s[0];
}
// Transcript::new(label), n append_message calls (labels and messages flat, lens[2 k], lens[2 k + 1] their lengths), then
// challenge_bytes(clabel, out_len)
void hs_merlin(const uint8_t* label, size_t ll, int n, const uint8_t* flat, const uint64_t* lens, const uint8_t* clabel, size_t cl, uint8_t* out,
               size_t out_len) {
  strobe128 s;
  merlin_init(s, label, ll);
  for (int k = 0; k < n; k++) {
    merlin_append(s, flat, lens[2 * k], flat + lens[2 * k], lens[2 * k + 1]);
    flat += lens[2 * k] + lens[2 * k + 1];
  }
  merlin_challenge(s, clabel, cl, out, out_len);
}
// the proof's transcript through the prefix state: gbytes the compressed generator, pts = pk, generator, c1, c2, rs = r1, r2
void hs_elgamal_transcript(const uint8_t* gbytes, const uint8_t* pts, const uint8_t* rs, size_t K, uint8_t* out) {
  strobe128 s;
  elgamal_transcript_prefix(s, gbytes, K);
  elgamal_transcript(out, s, pts, rs, K);
}
// 64 little-endian bytes (as sixteen words) mod r, canonical
void hs_fr_from_wide(const uint32_t* v, uint32_t* out) {
  fr a;
  fr_from_wide(a, v);
  fr_from_mont(out, a);
}
// the signed window digits of a sub-scalar of `words` 64-bit words; returns the window count
int hs_elgamal_recode(int group, const uint64_t* k, int8_t* dig) {
  if (group == 1) {
    elgamal_recode(dig, k, share_ladder_t<1>::WORDS, elgamal_terms<1>::NW);
    return elgamal_terms<1>::NW;
  }
  elgamal_recode(dig, k, share_ladder_t<2>::WORDS, elgamal_terms<2>::NW);
  return elgamal_terms<2>::NW;
}
void hs_fr_neg(const uint32_t* c, uint32_t* out) { elgamal_neg_scalar(out, c); }
void hs_elgamal_ladder(int group, int terms, const uint32_t* pts, const uint32_t* ks, uint8_t* out) {
  if (group == 1) ladder<1, g1_jac>(terms, pts, ks, out);
  else ladder<2, g2_jac>(terms, pts, ks, out);
}
}
