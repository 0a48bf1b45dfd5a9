// Per-item pieces of the reference's core_verify (src/traits/sig_core.rs:120-146), shared by every kernel:
//   prepare  : identity checks (signature first, then public key), to-affine, optional Aug prefix, hash-to-curve
//   pairs    : (H(m), pk), (sig, -g)   with the G1 member first, as src/helpers.rs:41-63 arranges them
// SIG_GROUP = 1: Bls12381G1Impl (sig in G1, pk in G2, src/impls/g1.rs);  = 2: Bls12381G2Impl (src/impls/g2.rs).
#pragma once
#include "h2c.cuh"
#include "pairing.cuh"

// status codes of the C ABI (include/blsgpu.h)
#define BLS_OK 0
#define BLS_ERR_INVALID_SIGNATURE 1
#define BLS_ERR_SIG_IDENTITY 2
#define BLS_ERR_PK_IDENTITY 3
#define BLS_ERR_DUPLICATE_MESSAGE 4
#define BLS_ERR_INVALID_COEFFICIENT 5
#define BLS_ERR_BAD_LENGTH 6
#define BLS_ERR_BAD_ENCODING 7
#define BLS_ERR_LEGACY_FORMAT 8
#define BLS_ERR_COMMITMENT_IDENTITY 9
#define BLS_ERR_PROOF_IDENTITY 10
#define BLS_ERR_ZERO_CHALLENGE 11

// 1/a, 1/b, 1/c with one inversion (all three non-zero)
BLS_FN void fp_inv3(fp& a, fp& b, fp& c) {
  fp ab, abc, t;
  fp_mul(ab, a, b);
  fp_mul(abc, ab, c);
  fp_inv(abc, abc);
  fp_mul(t, abc, ab);   // 1/c
  fp_mul(abc, abc, c);  // 1/(ab)
  c = t;
  fp_mul(t, abc, b);    // 1/a
  fp_mul(b, abc, a);    // 1/b
  a = t;
}
BLS_FN void fp_inv2(fp& a, fp& b) {
  fp ab, t;
  fp_mul(ab, a, b);
  fp_inv(ab, ab);
  fp_mul(t, ab, b);
  fp_mul(b, ab, a);
  a = t;
}
BLS_FN void g1_apply_zinv(g1_aff& r, const g1_jac& p, const fp& zi) {
  fp zi2;
  fp_sqr(zi2, zi);
  fp_mul(r.x, p.x, zi2);
  fp_mul(zi2, zi2, zi);
  fp_mul(r.y, p.y, zi2);
  r.inf = false;
}
// 1/z for z in Fp2 given 1/norm(z)
BLS_FN void g2_apply_ninv(g2_aff& r, const g2_jac& p, const fp& ni) {
  fp2 zi, zi2;
  fp_mul(zi.c0, p.z.c0, ni);
  fp_mul(zi.c1, p.z.c1, ni);
  fp_neg(zi.c1, zi.c1);
  fp2_sqr(zi2, zi);
  fp2_mul(r.x, p.x, zi2);
  fp2_mul(zi2, zi2, zi);
  fp2_mul(r.y, p.y, zi2);
  r.inf = false;
}
BLS_FN void fp2_norm_sq(fp& n, const fp2& a) {
  fp t;
  fp_sqr(n, a.c0);
  fp_sqr(t, a.c1);
  fp_add(n, n, t);
}

// both of (pk, sig) to affine with one inversion; neither is infinity
BLS_FN void g1g2_to_aff(g1_aff& a1, g2_aff& a2, const g1_jac& p1, const g2_jac& p2) {
  fp z1 = p1.z, n2;
  fp2_norm_sq(n2, p2.z);
  fp_inv2(z1, n2);
  g1_apply_zinv(a1, p1, z1);
  g2_apply_ninv(a2, p2, n2);
}

BLS_FN void g1_neg_gen(g1_aff& r) {
  fp_load(r.x, G1_GEN_X);
  fp y;
  fp_load(y, G1_GEN_Y);
  fp_neg(r.y, y);
  r.inf = false;
}
// -[c] g2, c = h_eff^-1 mod r: the second pair's G2 member when the message point of a Bls12381G1Impl verification is not
// cofactor-cleared (csrc/g2neg_lines.cuh, tools/gen_g2_lines.py: e(h P', pk) e(sig, -g2) = 1  <=>  e(P', pk) e(sig, -[c] g2) = 1)
BLS_FN void g2_negc_gen(g2_aff& r) {
  fp2_load(r.x, G2_NEGC_X);
  fp2_load(r.y, G2_NEGC_Y);
  r.inf = false;
}
BLS_FN void g2_neg_gen(g2_aff& r) {
  fp2_load(r.x, G2_GEN_X);
  fp2 y;
  fp2_load(y, G2_GEN_Y);
  fp2_neg(r.y, y);
  r.inf = false;
}

// Bls12381G1Impl: builds P[0] = H(m), Q[0] = pk, P[1] = sig, Q[1] = -g2.
// Without message augmentation the three Jacobian -> affine conversions (sig, pk, H(m)) share ONE field inversion;
// with augmentation the key must be affine (compressed) before hashing, so that path keeps two.
// mode: 0 = message as given, 1 = MessageAugmentation (key bytes || message, reference src/traits/sig_aug.rs:20-24),
//       2 = proof of possession (the message IS the key bytes, reference src/traits/sig_pop.rs:67-70)
// no_clear: P[0] is the message point BEFORE its cofactor clearing and Q[1] = -[c] g2 instead of -g2 (same verdict, a third
// of the hash saved; see g2_negc_gen)
// the part after the hash (no augmentation): sig, H(m) and pk to affine with ONE shared inversion
BLS_FN void prepare_g1impl_tail(g1_aff* P, g2_aff* Q, const g2_jac& pk, const g1_jac& sig, const g1_jac& h) {
  if (jac_is_inf(h)) {              // cannot happen for a hash output in practice; keep the generic path correct
    g1g2_to_aff(P[1], Q[0], sig, pk);
    jac_to_aff(P[0], h);
  } else {
    fp zs = sig.z, zh = h.z, n;
    fp2_norm_sq(n, pk.z);
    fp_inv3(zs, zh, n);
    g1_apply_zinv(P[1], sig, zs);
    g1_apply_zinv(P[0], h, zh);
    g2_apply_ninv(Q[0], pk, n);
  }
}
BLS_FN int prepare_g1impl(g1_aff* P, g2_aff* Q, const g2_jac& pk, const g1_jac& sig, int mode, const uint8_t* msg,
                          uint32_t msg_len, const uint8_t* dst, uint32_t dst_len, int lane2 = -1, bool no_clear = false) {
  if (jac_is_inf(sig)) return BLS_ERR_SIG_IDENTITY;
  if (jac_is_inf(pk)) return BLS_ERR_PK_IDENTITY;
  g1_jac h;
  if (mode) {
    g1g2_to_aff(P[1], Q[0], sig, pk);
    uint8_t pre[96];
    g2_compress(pre, Q[0], false);
    if (mode == 1) hash_to_g1(h, pre, 96, msg, msg_len, dst, dst_len, lane2, no_clear);
    else hash_to_g1(h, nullptr, 0, pre, 96, dst, dst_len, lane2, no_clear);
    jac_to_aff(P[0], h);
  } else {
    hash_to_g1(h, nullptr, 0, msg, msg_len, dst, dst_len, lane2, no_clear);
    prepare_g1impl_tail(P, Q, pk, sig, h);
  }
  if (no_clear) g2_negc_gen(Q[1]);
  else g2_neg_gen(Q[1]);
  return BLS_OK;
}

// Bls12381G2Impl: P[0] = pk, Q[0] = H(m), P[1] = -g1, Q[1] = sig
BLS_FN int prepare_g2impl(g1_aff* P, g2_aff* Q, const g1_jac& pk, const g2_jac& sig, int mode, const uint8_t* msg,
                          uint32_t msg_len, const uint8_t* dst, uint32_t dst_len, int lane2 = -1) {
  if (jac_is_inf(sig)) return BLS_ERR_SIG_IDENTITY;
  if (jac_is_inf(pk)) return BLS_ERR_PK_IDENTITY;
  g2_jac h;
  if (mode) {
    g1g2_to_aff(P[0], Q[1], pk, sig);
    uint8_t pre[48];
    g1_compress(pre, P[0], false);
    if (mode == 1) hash_to_g2(h, pre, 48, msg, msg_len, dst, dst_len, lane2);
    else hash_to_g2(h, nullptr, 0, pre, 48, dst, dst_len, lane2);
    jac_to_aff(Q[0], h);
  } else {
    hash_to_g2(h, nullptr, 0, msg, msg_len, dst, dst_len, lane2);
    if (jac_is_inf(h)) {
      g1g2_to_aff(P[0], Q[1], pk, sig);
      jac_to_aff(Q[0], h);
    } else {
      fp zp = pk.z, ns, nh;
      fp2_norm_sq(ns, sig.z);
      fp2_norm_sq(nh, h.z);
      fp_inv3(zp, ns, nh);
      g1_apply_zinv(P[0], pk, zp);
      g2_apply_ninv(Q[1], sig, ns);
      g2_apply_ninv(Q[0], h, nh);
    }
  }
  g1_neg_gen(P[1]);
  return BLS_OK;
}

template <class F2>
BLS_FN int pairing_verdict(const fp12_t<F2>& f) {
  return final_exp_is_one(f) ? BLS_OK : BLS_ERR_INVALID_SIGNATURE;
}

// ---- per-item bodies of the stage-1 variants that feed the two-pair pairing stages (k_prepare_hashed, k_prepare_proof):
// one item in, its two pairs and its status out.  A status other than BLS_OK leaves the pairs unset: the
// kernels then write no pair slots and every later stage skips the item on its status.  tests/hostsim_pairing_doors compiles
// the same functions for the host with the bound tracker on.

// core_verify's stage 1 with H(msg) given: the identity checks (signature first, then key: reference
// src/traits/sig_core.rs:126-135) and the shared-inversion conversion to affine pairs.  SG = 1: P[0] = H, Q[0] = pk, P[1] = sig,
// Q[1] = -g2; SG = 2: P[0] = pk, Q[0] = H, P[1] = -g1, Q[1] = sig.
BLS_FN int prepare_hashed_item(g1_aff* P, g2_aff* Q, const g2_jac& pk, const g1_jac& sig, const g1_jac& h) {
  int st = BLS_OK;
  if (jac_is_inf(sig)) st = BLS_ERR_SIG_IDENTITY;
  else if (jac_is_inf(pk)) st = BLS_ERR_PK_IDENTITY;
  else if (jac_is_inf(h)) {
    g1g2_to_aff(P[1], Q[0], sig, pk);
    jac_to_aff(P[0], h);
  } else {
    fp zs = sig.z, zh = h.z, nn;
    fp2_norm_sq(nn, pk.z);
    fp_inv3(zs, zh, nn);
    g1_apply_zinv(P[1], sig, zs);
    g1_apply_zinv(P[0], h, zh);
    g2_apply_ninv(Q[0], pk, nn);
  }
  g2_neg_gen(Q[1]);
  return st;
}
BLS_FN int prepare_hashed_item(g1_aff* P, g2_aff* Q, const g1_jac& pk, const g2_jac& sig, const g2_jac& h) {
  int st = BLS_OK;
  if (jac_is_inf(sig)) st = BLS_ERR_SIG_IDENTITY;
  else if (jac_is_inf(pk)) st = BLS_ERR_PK_IDENTITY;
  else if (jac_is_inf(h)) {
    g1g2_to_aff(P[0], Q[1], pk, sig);
    jac_to_aff(Q[0], h);
  } else {
    fp zp = pk.z, ns, nh;
    fp2_norm_sq(ns, sig.z);
    fp2_norm_sq(nh, h.z);
    fp_inv3(zp, ns, nh);
    g1_apply_zinv(P[0], pk, zp);
    g2_apply_ninv(Q[1], sig, ns);
    g2_apply_ninv(Q[0], h, nh);
  }
  g1_neg_gen(P[1]);
  return st;
}

BLS_FN bool scalar_words_zero(const uint32_t* y) {
  uint32_t o = 0;
  for (int k = 0; k < 8; k++) o |= y[k];
  return o == 0;
}
// BlsSignatureProof::verify (reference src/traits/sig_proof.rs:102-142): the checks in the reference's order (commitment, proof,
// pk identity; y zero), T = commitment + y * H(msg), and the pairs of e(T, pk) * e(-proof, -g) == 1 in core_verify's layout with
// H(m) := T and sig := -proof.  u: the commitment, v: the proof (negated in place), y: 8 little-endian words.
BLS_FN int prepare_proof_item(g1_aff* P, g2_aff* Q, const g1_jac& u, g1_jac& v, const g2_jac& pk, const uint32_t* y, const uint8_t* m,
                              uint32_t mlen, const uint8_t* dst, uint32_t dst_len) {
  int st = BLS_OK;
  if (jac_is_inf(u)) st = BLS_ERR_COMMITMENT_IDENTITY;
  else if (jac_is_inf(v)) st = BLS_ERR_PROOF_IDENTITY;
  else if (jac_is_inf(pk)) st = BLS_ERR_PK_IDENTITY;
  else if (scalar_words_zero(y)) st = BLS_ERR_ZERO_CHALLENGE;
  if (st == BLS_OK) {
    g1_jac a;
    hash_to_g1(a, nullptr, 0, m, mlen, dst, dst_len);
    jac_mul_scalar(a, a, y);
    jac_add(a, a, u);
    if (jac_is_inf(a)) {          // e(T, pk) = 1: the product is e(proof, g) with proof != identity, never one
      st = BLS_ERR_INVALID_SIGNATURE;
    } else {
      jac_neg(v, v);
      g1g2_to_aff(P[1], Q[0], v, pk);
      jac_to_aff(P[0], a);
      g2_neg_gen(Q[1]);
    }
  }
  return st;
}
BLS_FN int prepare_proof_item(g1_aff* P, g2_aff* Q, const g2_jac& u, g2_jac& v, const g1_jac& pk, const uint32_t* y, const uint8_t* m,
                              uint32_t mlen, const uint8_t* dst, uint32_t dst_len) {
  int st = BLS_OK;
  if (jac_is_inf(u)) st = BLS_ERR_COMMITMENT_IDENTITY;
  else if (jac_is_inf(v)) st = BLS_ERR_PROOF_IDENTITY;
  else if (jac_is_inf(pk)) st = BLS_ERR_PK_IDENTITY;
  else if (scalar_words_zero(y)) st = BLS_ERR_ZERO_CHALLENGE;
  if (st == BLS_OK) {
    g2_jac a;
    hash_to_g2(a, nullptr, 0, m, mlen, dst, dst_len);
    jac_mul_scalar(a, a, y);
    jac_add(a, a, u);
    if (jac_is_inf(a)) {
      st = BLS_ERR_INVALID_SIGNATURE;
    } else {
      jac_neg(v, v);
      g1g2_to_aff(P[0], Q[1], pk, v);
      jac_to_aff(Q[0], a);
      g1_neg_gen(P[1]);
    }
  }
  return st;
}
