// Threshold recovery: Signature::from_shares / PublicKey::from_shares (reference src/signature.rs:151-165,
// src/public_key.rs:128-134 -> core_combine_*_shares, src/traits/sig_core.rs:92-105) for many independent sets at once.
// The dependency interpolates at zero:  lambda_i = prod_{j != i} x_j / (x_j - x_i),  result = sum_i lambda_i P_i.
// The per-item functions of the recovery, shared by the kernels (tu_shares.inc) and the host harness (tests/hostsim_shares):
//   * share_lagrange_acc / share_lagrange_fin: one share's coefficient from the identifiers of its set, streamed in any order
//     (the kernel streams them through LDS in tiles): t - 1 products for the numerator, t - 1 for the denominator, ONE
//     inversion.  A zero difference is the duplicate check.
//   * share_naf / share_ladder: lambda_i P_i as ONE joint ladder over the endomorphism split of lambda_i (msm2.cuh):
//     64 (G2) / 128 (G1) doublings, and a mixed addition from an affine image for every non-zero NAF digit of every
//     sub-scalar (about a third of the digits).
#pragma once
#include "verify.cuh"
#include "msm2.cuh"
#include "fr.cuh"

// per-set flags (atomicOr by the share lanes) -> one status, in the order of the reference: deserialisation first (an
// identifier >= r cannot be a Scalar), then the scheme check of from_shares, then the dependency's combine
#define SHARE_F_ENCODING 1u
#define SHARE_F_SCHEME 2u
#define SHARE_F_VSSS 4u
#define SHARE_F_MSM 8u        // set by the host: the set is summed by the bucket MSM, not by the per-share ladders
#define BLS_ERR_INVALID_SCHEME 12   // BlsError::InvalidSignatureScheme (include/blsgpu.h)
#define BLS_ERR_VSSS 13             // BlsError::VsssError

struct share_lagrange {
  fr num, den;         // prod_{j != i} x_j, prod_{j != i} (x_j - x_i), Montgomery form
  bool dup;            // some x_j == x_i with j != i
};
BLS_FN void share_lagrange_init(share_lagrange& L) {
  fr_one(L.num);
  fr_one(L.den);
  L.dup = false;
}
// one other share j (j != i) of the set
BLS_FN void share_lagrange_acc(share_lagrange& L, const fr& xi, const fr& xj) {
  fr d;
  fr_sub(d, xj, xi);
  if (fr_is_zero(d)) L.dup = true;
  fr_mul(L.num, L.num, xj);
  fr_mul(L.den, L.den, d);
}
// lambda_i as canonical little-endian words; returns the share's VSSS flag (zero identifier or duplicate)
BLS_FN uint32_t share_lagrange_fin(uint32_t lam[8], const share_lagrange& L, const fr& xi) {
  fr inv, l;
  fr_inv(inv, L.den);
  fr_mul(l, L.num, inv);
  fr_from_mont(lam, l);
  return (L.dup || fr_is_zero(xi)) ? SHARE_F_VSSS : 0u;
}

// non-adjacent form of a multiword scalar k (words 64-bit words, k < 2^(64 words - 1) or any value when words = 1 with an extra
// word of headroom below): digit i = +1 where pos bit i is set, -1 where neg bit i is set.  With h = 3 k: digit i = h_{i+1} - k_{i+1}.
BLS_FN void share_naf(uint64_t pos[3], uint64_t neg[3], const uint64_t* k, int words) {
  uint64_t kk[3] = {0, 0, 0}, h[3];
  for (int j = 0; j < words; j++) kk[j] = k[j];
  uint64_t c = 0;
  for (int j = 0; j < 3; j++) {       // h = k + 2 k
    const uint64_t s = (kk[j] << 1) | (j ? kk[j - 1] >> 63 : 0);
    const uint64_t a = kk[j] + s;
    const uint64_t c1 = a < kk[j] ? 1 : 0;
    h[j] = a + c;
    c = c1 + (h[j] < a ? 1 : 0);
  }
  for (int j = 0; j < 3; j++) {       // bits 1.. of h and k, shifted down by one
    const uint64_t hs = (h[j] >> 1) | (j < 2 ? h[j + 1] << 63 : 0);
    const uint64_t ks = (kk[j] >> 1) | (j < 2 ? kk[j + 1] << 63 : 0);
    pos[j] = hs & ~ks;
    neg[j] = ~hs & ks;
  }
}

// lambda P for an affine point P (not the identity) and canonical lambda words: the joint NAF ladder over the E images of P
// (G1: P, -phi P with 128-bit sub-scalars; G2: P, -psi P, psi^2 P, -psi^3 P with 64-bit ones)
template <int G>
struct share_ladder_t;
template <>
struct share_ladder_t<1> {
  typedef fp F;
  enum { E = 2, WORDS = 2, TOP = 128 };
  BLS_MFN static void images(F qx[2], F qy[2], const g1_aff& p) { msm2_images_g1(qx, qy, p); }
  BLS_MFN static void decompose(uint64_t a[4], const uint32_t* lam) { msm2_decompose_g1(a, lam); }
};
template <>
struct share_ladder_t<2> {
  typedef fp2 F;
  enum { E = 4, WORDS = 1, TOP = 64 };
  BLS_MFN static void images(F qx[4], F qy[4], const g2_aff& p) { msm2_images_g2(qx, qy, p); }
  BLS_MFN static void decompose(uint64_t a[4], const uint32_t* lam) { msm2_decompose_g2(a, lam); }
};
template <int G, class F>
BLS_FN void share_ladder(jac<F>& acc, const aff<F>& p, const uint32_t lam[8]) {
  typedef share_ladder_t<G> T;
  jac_set_inf(acc);
  if (p.inf) return;
  uint64_t a[4], pos[T::E][3], neg[T::E][3];
  T::decompose(a, lam);
  for (int j = 0; j < T::E; j++) share_naf(pos[j], neg[j], a + j * T::WORDS, T::WORDS);
  F qx[T::E], qy[T::E];
  T::images(qx, qy, p);
  for (int b = T::TOP; b >= 0; b--) {
    if (!jac_is_inf(acc)) jac_dbl(acc, acc);
    for (int j = 0; j < T::E; j++) {
      const bool ps = (pos[j][b >> 6] >> (b & 63)) & 1, ng = (neg[j][b >> 6] >> (b & 63)) & 1;
      if (ps || ng) {
        F y = qy[j];
        if (ng) {
          fe_neg(y, y);
          fe_reduce(y, y);
        }
        jac_madd(acc, acc, qx[j], y);
      }
    }
  }
}

// level `step` (1, 2, 4, ...) of the segmented pairwise tree over the records [lo, hi) of one set: does record i add in record
// i + step?  (k_share_fold; the strips of the batched multi verify, multi_batch.cuh, fold through it too)
BLS_FN bool share_fold_adds(uint64_t i, uint64_t step, uint64_t lo, uint64_t hi) {
  return ((i - lo) & (2 * step - 1)) == 0 && i + step < hi;
}

#if defined(__HIPCC__)
// ---- kernels (tu_shares1.hip: the coefficients and G1, tu_shares2.hip: G2); one lane per share unless said otherwise
// status flags of set s: flags[s]; the share -> set map: sid[i]; the per-share products lambda_i P_i: part (RAW_PROJ records)
__global__ void k_share_lagrange(size_t n, const uint64_t* offs, size_t n_sets, const uint8_t* ids, uint32_t* flags, uint32_t* nd, uint32_t* sid);
__global__ void k_share_lagrange_fin(size_t n, int S, const uint64_t* offs, const uint8_t* ids, const uint8_t* schemes, const uint32_t* nd,
                                     const uint32_t* sid, uint32_t* flags, uint8_t* lam);
template <int G>
__global__ void k_share_ladder(size_t n, const uint8_t* pts, int fmt, const uint8_t* lam, const uint32_t* sid, const uint32_t* flags,
                               uint8_t* part);
template <int G>
__global__ void k_share_fold(size_t n, uint64_t step, const uint64_t* offs, const uint32_t* sid, uint8_t* part);
template <int G>
__global__ void k_share_out(size_t n_sets, const uint64_t* offs, const uint32_t* flags, const uint8_t* part, uint8_t* out, int32_t* status);
#endif
