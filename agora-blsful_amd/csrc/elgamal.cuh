// ElGamal over the public-key group, the public-data side (reference src/traits/elgamal.rs:177-226 verify_proof,
// src/elgamal_decryption_share.rs:76-90 from_shares / decrypt) for many proofs / ciphertexts at once:
// blsgpu_elgamal_proof_verify_batch and blsgpu_elgamal_open_batch.  The per-item functions, shared by the kernels
// (tu_elgamal.inc) and the host harness (tests/hostsim_elgamal):
//   * strobe128 / merlin_*: STROBE-128 as Merlin uses it (rate 166, protocol "Merlin v1.0"), a byte-wise duplex over the
//     Keccak-f[1600] of keccak.cuh, and the three Transcript calls of the proof (new, append_message, challenge_bytes);
//   * elgamal_transcript: the proof's transcript from the state after its fixed prefix to the 64 challenge bytes;
//   * elgamal_terms / elgamal_ladder: sum_t k_t P_t for up to three (point, scalar) terms as ONE joint ladder over the
//     endomorphism split (msm2.cuh, shares.cuh): every image of every term shares the 68 (G2) / 132 (G1) doublings.
//     The bases are chosen by whoever made the proof and can be related (c1 = G, c1 = -G, a proof with r = 0), so the
//     accumulator does meet P + P, P - P and the identity: jac_madd (msm2.cuh) handles all three, jac_dbl is not given the
//     identity.
#pragma once
#include "keccak.cuh"
#include "shares.cuh"

#define BLS_ERR_ELGAMAL_IDENTITY 16     // InvalidInputs("Parameters or ciphertext values are identity point") (include/blsgpu.h)
#define BLS_ERR_ELGAMAL_ZERO_PROOF 17   // InvalidInputs("Proof values are zero")
#define BLS_ERR_CHALLENGE_MISMATCH 18   // InvalidInputs("Challenge values do not match")

// ---- STROBE-128 (v1.0.2), the operations Merlin uses: AD, meta-AD and PRF
#define STROBE_R 166
#define STROBE_FLAG_I 1u
#define STROBE_FLAG_A 2u
#define STROBE_FLAG_C 4u
#define STROBE_FLAG_M 16u
#define STROBE_FLAG_K 32u

struct strobe128 {
  keccak_state st;
  uint32_t pos, pos_begin;
};
KECCAK_FN void strobe_xor_byte(strobe128& s, uint32_t at, uint8_t b) { s.st.s[at >> 3] ^= (uint64_t)b << (8 * (at & 7)); }
KECCAK_FN void strobe_run_f(strobe128& s) {
  strobe_xor_byte(s, s.pos, (uint8_t)s.pos_begin);
  strobe_xor_byte(s, s.pos + 1, 0x04);
  strobe_xor_byte(s, STROBE_R + 1, 0x80);
  keccak_f1600(s.st);
  s.pos = 0;
  s.pos_begin = 0;
}
KECCAK_FN void strobe_absorb(strobe128& s, const uint8_t* d, size_t n) {
  for (size_t k = 0; k < n; k++) {
    strobe_xor_byte(s, s.pos, d[k]);
    if (++s.pos == STROBE_R) strobe_run_f(s);
  }
}
KECCAK_FN void strobe_squeeze(strobe128& s, uint8_t* out, size_t n) {
  for (size_t k = 0; k < n; k++) {
    const uint32_t sh = 8 * (s.pos & 7);
    out[k] = (uint8_t)(s.st.s[s.pos >> 3] >> sh);
    s.st.s[s.pos >> 3] &= ~((uint64_t)0xff << sh);
    if (++s.pos == STROBE_R) strobe_run_f(s);
  }
}
// the start of an operation that is not a continuation (Merlin continues only meta-AD, which needs no call here)
KECCAK_FN void strobe_begin_op(strobe128& s, uint32_t flags) {
  const uint8_t hdr[2] = {(uint8_t)s.pos_begin, (uint8_t)flags};
  s.pos_begin = s.pos + 1;
  strobe_absorb(s, hdr, 2);
  if ((flags & (STROBE_FLAG_C | STROBE_FLAG_K)) && s.pos != 0) strobe_run_f(s);
}
KECCAK_FN void strobe_meta_ad(strobe128& s, const uint8_t* d, size_t n, bool more) {
  if (!more) strobe_begin_op(s, STROBE_FLAG_M | STROBE_FLAG_A);
  strobe_absorb(s, d, n);
}
KECCAK_FN void strobe_ad(strobe128& s, const uint8_t* d, size_t n) {
  strobe_begin_op(s, STROBE_FLAG_A);
  strobe_absorb(s, d, n);
}
KECCAK_FN void strobe_prf(strobe128& s, uint8_t* out, size_t n) {
  strobe_begin_op(s, STROBE_FLAG_I | STROBE_FLAG_A | STROBE_FLAG_C);
  strobe_squeeze(s, out, n);
}
KECCAK_FN void strobe_init(strobe128& s, const uint8_t* label, size_t n) {
  const uint8_t head[18] = {1, STROBE_R + 2, 1, 0, 1, 96, 'S', 'T', 'R', 'O', 'B', 'E', 'v', '1', '.', '0', '.', '2'};
  for (int k = 0; k < 25; k++) s.st.s[k] = 0;
  s.pos = 0;
  s.pos_begin = 0;
  for (int k = 0; k < 18; k++) strobe_xor_byte(s, (uint32_t)k, head[k]);
  keccak_f1600(s.st);
  strobe_meta_ad(s, label, n, false);
}

// ---- Merlin: Transcript::new, append_message, challenge_bytes
KECCAK_FN void merlin_len(uint8_t b[4], size_t n) {
  for (int k = 0; k < 4; k++) b[k] = (uint8_t)(n >> (8 * k));
}
KECCAK_FN void merlin_append(strobe128& s, const uint8_t* label, size_t ll, const uint8_t* msg, size_t ml) {
  uint8_t len[4];
  merlin_len(len, ml);
  strobe_meta_ad(s, label, ll, false);
  strobe_meta_ad(s, len, 4, true);
  strobe_ad(s, msg, ml);
}
KECCAK_FN void merlin_init(strobe128& s, const uint8_t* label, size_t ll) {
  const uint8_t proto[11] = {'M', 'e', 'r', 'l', 'i', 'n', ' ', 'v', '1', '.', '0'}, dom[7] = {'d', 'o', 'm', '-', 's', 'e', 'p'};
  strobe_init(s, proto, 11);
  merlin_append(s, dom, 7, label, ll);
}
KECCAK_FN void merlin_challenge(strobe128& s, const uint8_t* label, size_t ll, uint8_t* out, size_t n) {
  uint8_t len[4];
  merlin_len(len, n);
  strobe_meta_ad(s, label, ll, false);
  strobe_meta_ad(s, len, 4, true);
  strobe_prf(s, out, n);
}

// ---- the proof's transcript (elgamal.rs:203-216).  The prefix is the same for every proof of a group: Transcript::new(b"ElGamalProof"),
// "dst" and "base point" (gbytes: the compressed generator, K = 48 / 96 bytes).
KECCAK_FN void elgamal_transcript_prefix(strobe128& s, const uint8_t* gbytes, size_t K) {
  const uint8_t proof[12] = {'E', 'l', 'G', 'a', 'm', 'a', 'l', 'P', 'r', 'o', 'o', 'f'}, dst[3] = {'d', 's', 't'},
                base[10] = {'b', 'a', 's', 'e', ' ', 'p', 'o', 'i', 'n', 't'};
  const char* salt = "ELGAMAL_BLS12381_XOF:HKDF-SHA2-256_";
  merlin_init(s, proof, 12);
  merlin_append(s, dst, 3, (const uint8_t*)salt, 35);
  merlin_append(s, base, 10, gbytes, K);
}
// from the prefix state: pk, generator, c1, c2 (pts: 4 K bytes in that order), r1, r2 (rs: 2 K bytes), then the 64 challenge bytes
KECCAK_FN void elgamal_transcript(uint8_t out[64], const strobe128& prefix, const uint8_t* pts, const uint8_t* rs, size_t K) {
  const uint8_t l_pk[2] = {'p', 'k'}, l_gen[9] = {'g', 'e', 'n', 'e', 'r', 'a', 't', 'o', 'r'}, l_c1[2] = {'c', '1'}, l_c2[2] = {'c', '2'},
                l_r1[2] = {'r', '1'}, l_r2[2] = {'r', '2'}, l_ch[9] = {'c', 'h', 'a', 'l', 'l', 'e', 'n', 'g', 'e'};
  strobe128 s = prefix;
  merlin_append(s, l_pk, 2, pts, K);
  merlin_append(s, l_gen, 9, pts + K, K);
  merlin_append(s, l_c1, 2, pts + 2 * K, K);
  merlin_append(s, l_c2, 2, pts + 3 * K, K);
  merlin_append(s, l_r1, 2, rs, K);
  merlin_append(s, l_r2, 2, rs + K, K);
  merlin_challenge(s, l_ch, 9, out, 64);
}

// ---- affine forms of K Jacobian points with ONE inversion (prefix products of the Z coordinates; an identity is skipped)
template <int K, class F>
BLS_FN void elgamal_to_aff(aff<F>* a, const jac<F>* p) {
  F pre[K], acc, inv;
  fe_one(acc);
  for (int k = 0; k < K; k++) {
    pre[k] = acc;
    if (!jac_is_inf(p[k])) fe_mul(acc, acc, p[k].z);
  }
  fe_inv(inv, acc);
  for (int k = K - 1; k >= 0; k--) {
    a[k].inf = jac_is_inf(p[k]);
    if (a[k].inf) {
      fe_zero(a[k].x);
      fe_zero(a[k].y);
      continue;
    }
    F zi, zi2;
    fe_mul(zi, inv, pre[k]);
    fe_mul(inv, inv, p[k].z);
    fe_sqr(zi2, zi);
    fe_mul(a[k].x, p[k].x, zi2);
    fe_mul(zi2, zi2, zi);
    fe_mul(a[k].y, p[k].y, zi2);
  }
}

// ---- the joint ladder: sum_t k_t P_t over the endomorphism split with ONE accumulator.
// Every sub-scalar (E per term, msm2.cuh) is cut into signed windows of ELGAMAL_W bits, digits in [-2^(W-1), 2^(W-1)], and every
// term brings the affine multiples 1 .. 2^(W-1) of its point; the image of a multiple is taken when it is added.  The schedule --
// W doublings, then one mixed addition per (term, image) -- is the same in every lane whatever the scalars are, which is what a
// wave needs: with per-lane NAF digits 64 independent lanes want an addition at nearly every (bit, image) slot and the
// sparsity of the form is lost to divergence (DESIGN.md section 4 "ElGamal").
#define ELGAMAL_MAX_TERMS 3
#define ELGAMAL_W 4
#define ELGAMAL_TAB 8            // 2^(W-1) multiples per term
template <int G>
struct elgamal_terms {
  typedef share_ladder_t<G> T;
  typedef typename T::F F;
  enum { E = T::E, NW = T::TOP / ELGAMAL_W + 1 };     // a sub-scalar is below 2^TOP; the last window holds the carry alone
  aff<F> tab[ELGAMAL_MAX_TERMS][ELGAMAL_TAB];          // tab[t][m - 1] = m P_t
  int8_t dig[ELGAMAL_MAX_TERMS * T::E][NW];
  int terms;
};
// signed digits of k (`words` 64-bit words, k < 2^(64 words)): k = sum_w dig[w] 2^(W w); W divides 64, so no window straddles a word
BLS_FN void elgamal_recode(int8_t* dig, const uint64_t* k, int words, int nw) {
  int carry = 0;
  for (int w = 0; w < nw; w++) {
    const int bit = ELGAMAL_W * w;
    int d = carry + (bit < 64 * words ? (int)((k[bit >> 6] >> (bit & 63)) & ((1u << ELGAMAL_W) - 1)) : 0);
    carry = d > (1 << (ELGAMAL_W - 1)) ? 1 : 0;
    dig[w] = (int8_t)(d - (carry << ELGAMAL_W));
  }
}
// term t's scalar: canonical little-endian words
template <int G>
BLS_FN void elgamal_term_scalar(elgamal_terms<G>& S, int t, const uint32_t k[8]) {
  typedef share_ladder_t<G> T;
  uint64_t a[4];
  T::decompose(a, k);
  for (int j = 0; j < T::E; j++) elgamal_recode(S.dig[t * T::E + j], a + j * T::WORDS, T::WORDS, elgamal_terms<G>::NW);
}
// the multiples 1 .. ELGAMAL_TAB of an affine point (not the identity), affine, with ONE inversion
template <class F>
BLS_FN void elgamal_multiples(aff<F>* tab, const aff<F>& p) {
  jac<F> m[ELGAMAL_TAB];
  F x, y;
  fe_reduce(x, p.x);
  fe_reduce(y, p.y);
  m[0].x = x;
  m[0].y = y;
  fe_one(m[0].z);
  jac_dbl(m[1], m[0]);
  for (int k = 2; k < ELGAMAL_TAB; k++) jac_madd(m[k], m[k - 1], x, y);
  elgamal_to_aff<ELGAMAL_TAB>(tab, m);
}
template <int G, class F>
BLS_FN void elgamal_term_point(elgamal_terms<G>& S, int t, const aff<F>& p) {
  elgamal_multiples(S.tab[t], p);
}
// image j of an affine point with the sign of the decomposition folded in (msm2.cuh): G1: P, -phi P; G2: P, -psi P, psi^2 P, -psi^3 P
BLS_FN void elgamal_image(fp& x, fp& y, const g1_aff& p, int j) {
  if (j == 0) {
    fp_reduce(x, p.x);
    fp_reduce(y, p.y);
    return;
  }
  fp beta;
  fp_load(beta, G1_BETA);
  fp_mul(x, p.x, beta);
  fp_neg(y, p.y);
  fp_reduce(y, y);
}
BLS_FN void elgamal_image(fp2& x, fp2& y, const g2_aff& p, int j) {
  if (j == 0) {
    fp2_reduce(x, p.x);
    fp2_reduce(y, p.y);
    return;
  }
  fp2 sx = p.x, sy = p.y, t;
  if (j >= 2) {                            // psi^2
    fp cx2, cy2;
    fp_load(cx2, PSI2_CX);
    fp_load(cy2, PSI2_CY);
    fp2_mul_fp(sx, p.x, cx2);
    fp2_mul_fp(sy, p.y, cy2);
    if (j == 2) {
      x = sx;
      y = sy;
      return;
    }
  }
  fp2_conj(t, sx);                         // -psi of what is there
  fp2_mul_const(x, t, PSI_CX);
  fp2_conj(t, sy);
  fp2_mul_const(t, t, PSI_CY);
  fp2_neg(t, t);
  fp2_reduce(y, t);
}
template <int G, class F>
BLS_FN void elgamal_ladder(jac<F>& acc, const elgamal_terms<G>& S) {
  typedef elgamal_terms<G> TS;
  jac_set_inf(acc);
  for (int w = TS::NW - 1; w >= 0; w--) {
    if (!jac_is_inf(acc))
      for (int k = 0; k < ELGAMAL_W; k++) jac_dbl(acc, acc);
    for (int t = 0; t < S.terms; t++) {
      for (int j = 0; j < TS::E; j++) {
        const int d = S.dig[t * TS::E + j][w];
        if (d == 0) continue;
        const aff<F>& e = S.tab[t][(d < 0 ? -d : d) - 1];
        if (e.inf) continue;               // only a point outside the prime-order subgroup has the identity among its multiples
        F x, y;
        elgamal_image(x, y, e, j);
        if (d < 0) {
          fe_neg(y, y);
          fe_reduce(y, y);
        }
        jac_madd(acc, acc, x, y);
      }
    }
  }
}
// -c mod r on canonical words (c < r)
BLS_FN void elgamal_neg_scalar(uint32_t o[8], const uint32_t c[8]) {
  fr z, v, d;
  for (int j = 0; j < 8; j++) {
    z.w[j] = 0;
    v.w[j] = c[j];
  }
  fr_sub(d, z, v);
  for (int j = 0; j < 8; j++) o[j] = d.w[j];
}

#if defined(__HIPCC__)
// ---- kernels (tu_elgamal1.hip: G = 1, tu_elgamal2.hip: G = 2; G is the KEY group of the proofs), described in tu_elgamal.inc
// fixed[((p ELGAMAL_TAB + m - 1) 2 + (0: x, 1: y)) FW ..): the multiple m of p = 0: the group generator, 1: the message generator h,
// raw affine coordinates
template <int G>
__global__ void k_elgamal_fixed(const uint8_t* h, uint32_t* fixed);
// aff[4 i + k], comp[(4 i + k) K ..): pk, generator, c1, c2 of proof i as Z = 1 RAW_PROJ records and compressed; dec / dec_pk: the
// decode verdicts of wire-format input (per proof; of the one shared key) or null
template <int G>
__global__ void k_elgamal_prep(size_t n, const uint8_t* pks, size_t n_pks, const uint8_t* gens, const uint8_t* h, const uint8_t* c1s, const uint8_t* c2s, int fmt,
                               const uint8_t* mps, const uint8_t* bps, const uint8_t* cs, const int32_t* dec, const int32_t* dec_pk, uint8_t* aff_out,
                               uint8_t* comp, int32_t* status);
// 2 n lanes: lane i < n computes r1 of proof i, lane n + i its r2 (waves stay uniform in their term count) -> rj[lane], RAW_PROJ
template <int G>
__global__ void k_elgamal_ladder(size_t n, int own_gens, const uint8_t* aff_in, const uint32_t* fixed, const uint8_t* mps, const uint8_t* bps,
                                 const uint8_t* cs, const int32_t* status, uint8_t* rj);
template <int G>
__global__ void k_elgamal_transcript(size_t n, strobe128 prefix, const uint8_t* comp, const uint8_t* rj, const uint8_t* cs, int32_t* status);
// out[s] = c2[s] - key[s] (all-zero bytes for the identity or when cst[s] is not OK); status[s] = cst[s] (OK when cst is null)
template <int G>
__global__ void k_elgamal_sub(size_t n, const uint8_t* c2s, int fmt, const uint8_t* keys, int key_fmt, const int32_t* cst, uint8_t* out, int32_t* status);
#endif
