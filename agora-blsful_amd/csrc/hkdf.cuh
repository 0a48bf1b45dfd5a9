// HashToScalar of the reference (src/impls/g1.rs:25-27, g2.rs:23-25 -> scalar_from_hkdf_bytes, src/helpers.rs:9-26): HKDF-SHA-256
// extract with the salt as key over ikm || 0x00, expand with info = 00 30 to 48 bytes, the 48 bytes read as one big-endian integer
// and reduced modulo r (Scalar::from_okm).  The reference repeats the expand while the scalar is zero; expand returns the same
// bytes every time, so a zero stays a zero and is written as zero here (the proof check then reports BLSGPU_ZERO_CHALLENGE).
//   hkdf_scalar              any input and salt, on the byte-streaming sha256_ctx (h2c.cuh): SecretKey::from_hash,
//                            ProofCommitmentChallenge::from_hash, the oracle of the fixed shapes below
//   pok_challenge_words      BlsSignatureProof::compute_y (src/traits/sig_proof.rs:38-46): the hash input has one shape per orientation
//                            -- the compressed commitment, LE64(t), the extract's 0x00: 57 bytes (G1) or 105 (G2) -- and the salt is a
//                            constant, so its two key-block states are constants and every block is written in sixteen registers:
//                            9 compressions (2 inner + 1 outer extract, 2 PRK key blocks, 2 + 2 for T1 and T2) against the 13 of
//                            the streaming form, and no array that a run-time index addresses
// Public inputs only: nothing here is constant time.  Also compiles as plain C++ (tests/hostsim_pok).
#pragma once
#include "h2c.cuh"
#include "fr.cuh"

// ------------------------------------------------------------------ the general form
// out = HMAC-SHA-256(key, a || b).  A key longer than a block is hashed first (RFC 2104); an empty key is the all-zero block.
BLS_FN void hmac_sha256_2(uint8_t* out, const uint8_t* key, uint32_t key_len, const uint8_t* a, uint32_t a_len, const uint8_t* b,
                          uint32_t b_len) {
  uint8_t kb[64], d[32];
  sha256_ctx c;
  for (int i = 0; i < 64; i++) kb[i] = 0;
  if (key_len > 64) {
    sha256_init(c);
    sha256_update(c, key, key_len);
    sha256_final(c, kb);
  } else {
    for (uint32_t i = 0; i < key_len; i++) kb[i] = key[i];
  }
  sha256_init(c);
  for (int i = 0; i < 64; i++) sha256_byte(c, kb[i] ^ 0x36);
  sha256_update(c, a, a_len);
  sha256_update(c, b, b_len);
  sha256_final(c, d);
  sha256_init(c);
  for (int i = 0; i < 64; i++) sha256_byte(c, kb[i] ^ 0x5c);
  sha256_update(c, d, 32);
  sha256_final(c, out);
}
// twelve big-endian words of output keying material (most significant first) -> the canonical scalar, eight little-endian words
BLS_FN void okm_words_to_scalar(uint32_t y[8], const uint32_t okm[12]) {
  uint32_t v[16];
#pragma unroll
  for (int j = 0; j < 12; j++) v[j] = okm[11 - j];
#pragma unroll
  for (int j = 12; j < 16; j++) v[j] = 0;
  fr s;
  fr_from_wide(s, v);
  fr_from_mont(y, s);
}
// out: 32 bytes, little-endian, canonical (the form k_prepare_proof reads its challenges in)
BLS_FN void hkdf_scalar(uint8_t* out, const uint8_t* ikm, uint32_t ikm_len, const uint8_t* salt, uint32_t salt_len) {
  const uint8_t zero = 0, i1[3] = {0, 48, 1}, i2[3] = {0, 48, 2};
  uint8_t prk[32], t1[32], t2[32];
  hmac_sha256_2(prk, salt, salt_len, ikm, ikm_len, &zero, 1);
  hmac_sha256_2(t1, prk, 32, nullptr, 0, i1, 3);
  hmac_sha256_2(t2, prk, 32, t1, 32, i2, 3);
  uint32_t okm[12], y[8];
  for (int j = 0; j < 8; j++) okm[j] = be32_at(t1 + 4 * j);
  for (int j = 0; j < 4; j++) okm[8 + j] = be32_at(t2 + 4 * j);
  okm_words_to_scalar(y, okm);
  for (int j = 0; j < 8; j++) {
    out[4 * j] = (uint8_t)y[j];
    out[4 * j + 1] = (uint8_t)(y[j] >> 8);
    out[4 * j + 2] = (uint8_t)(y[j] >> 16);
    out[4 * j + 3] = (uint8_t)(y[j] >> 24);
  }
}

// ------------------------------------------------------------------ the two fixed shapes of compute_y
#define POK_SALT "BLS_POK__BLS12381_XOF:HKDF-SHA2-256_"   // src/traits/sig_proof.rs:5
#define POK_SALT_LEN 36
// SHA-256 states after the one key block of the extract: (salt || 0 ...) ^ 0x36 .. and ^ 0x5c .. (tests/test_hostsim_pok_timestamp.py
// recomputes them from the salt)
BLS_CONST uint32_t POK_IPAD_MID[8] = {0x015b55f2u, 0xde13ca20u, 0xf99a16cbu, 0x07ba9f4du, 0x2c39d2cbu, 0x04df6a00u, 0xcbaa6a82u, 0x94238950u};
BLS_CONST uint32_t POK_OPAD_MID[8] = {0x98ad0ba7u, 0xffe86374u, 0x7aa5910fu, 0xed02a85au, 0x5f1e4a29u, 0x685f9f5cu, 0x968e2c32u, 0xc1b0a632u};

// a hash state and a message block held by value: vector registers on the device (sha256_compress_v), plain structs on the host
#if defined(__HIPCC__)
typedef u32x8_t hk_h;
typedef u32x16_t hk_w;
BLS_FN hk_h hk_compress(hk_h h, hk_w w) { return sha256_compress_v(h, w); }
#else
struct hk_h {
  uint32_t v[8];
  uint32_t& operator[](int i) { return v[i]; }
  uint32_t operator[](int i) const { return v[i]; }
};
struct hk_w {
  uint32_t v[16];
  uint32_t& operator[](int i) { return v[i]; }
  uint32_t operator[](int i) const { return v[i]; }
};
BLS_FN hk_h hk_compress(hk_h h, const hk_w& w) {
  sha256_rounds(h.v, w.v);
  return h;
}
#endif
BLS_FN hk_h hk_state(const uint32_t* s) {
  hk_h h;
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = s[i];
  return h;
}
BLS_FN hk_h hk_iv() {
  hk_h h;
  h[0] = 0x6a09e667; h[1] = 0xbb67ae85; h[2] = 0x3c6ef372; h[3] = 0xa54ff53a;
  h[4] = 0x510e527f; h[5] = 0x9b05688c; h[6] = 0x1f83d9ab; h[7] = 0x5be0cd19;
  return h;
}
// words [from, 15) of a block zero, word 15 the bit length of a message of `bytes` bytes behind one key block
BLS_FN void hk_tail(hk_w& w, int from, uint32_t bytes) {
#pragma unroll
  for (int j = 0; j < 15; j++)
    if (j >= from) w[j] = 0;
  w[15] = (64 + bytes) * 8;
}
// the outer hash of an HMAC: `outer` is the state after the key ^ opad block, d the inner digest
BLS_FN hk_h hk_outer(hk_h outer, hk_h d) {
  hk_w w;
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = d[j];
  w[8] = 0x80000000u;
  hk_tail(w, 9, 32);
  return hk_compress(outer, w);
}
// the state after the one key block of an HMAC under a 32-byte key: (key || 0 ...) ^ pad
BLS_FN hk_h hk_key_state(hk_h key, uint32_t pad) {
  hk_w w;
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = key[j] ^ pad;
#pragma unroll
  for (int j = 8; j < 16; j++) w[j] = pad;
  return hk_compress(hk_iv(), w);
}
// y = compute_y(u, t): xw the NW = 12 (G1) or 24 (G2) big-endian words of u's modern compressed encoding.
//   G1, 57 bytes behind the key block:   block 1  x[0..12) t_lo t_hi 00800000 0          (byte 56 the extract's 0x00, byte 57 the pad)
//                                        block 2  0 ... 0 len
//   G2, 105 bytes:                       block 1  x[0..16)
//                                        block 2  x[16..24) t_lo t_hi 00800000 0 0 0 0 len   (byte 104 the 0x00, byte 105 the pad)
// with t_lo, t_hi the byte-swapped halves of t (LE64(t) read as big-endian words).
template <int NW>
BLS_FN void pok_challenge_words(uint32_t y[8], const uint32_t (&xw)[NW], uint64_t t) {
  static_assert(NW == 12 || NW == 24, "one compressed G1 or G2 point");
  const uint32_t t_lo = __builtin_bswap32((uint32_t)t), t_hi = __builtin_bswap32((uint32_t)(t >> 32));
  hk_h h = hk_state(POK_IPAD_MID);
  hk_w w;
  if constexpr (NW == 12) {
#pragma unroll
    for (int j = 0; j < 12; j++) w[j] = xw[j];
    w[12] = t_lo;
    w[13] = t_hi;
    w[14] = 0x00800000u;
    w[15] = 0;
    h = hk_compress(h, w);
    hk_tail(w, 0, 57);
    h = hk_compress(h, w);
  } else {
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = xw[j];
    h = hk_compress(h, w);
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = xw[NW - 8 + j];
    w[8] = t_lo;
    w[9] = t_hi;
    w[10] = 0x00800000u;
    hk_tail(w, 11, 105);
    h = hk_compress(h, w);
  }
  const hk_h prk = hk_outer(hk_state(POK_OPAD_MID), h);
  const hk_h ki = hk_key_state(prk, 0x36363636u), ko = hk_key_state(prk, 0x5c5c5c5cu);
  w[0] = 0x00300180u;                      // info = 00 30, counter 01, pad
  hk_tail(w, 1, 3);
  const hk_h t1 = hk_outer(ko, hk_compress(ki, w));
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = t1[j];
  w[8] = 0x00300280u;                      // T1 || 00 30 || 02, pad
  hk_tail(w, 9, 35);
  const hk_h t2 = hk_outer(ko, hk_compress(ki, w));
  uint32_t okm[12];
#pragma unroll
  for (int j = 0; j < 8; j++) okm[j] = t1[j];
#pragma unroll
  for (int j = 0; j < 4; j++) okm[8 + j] = t2[j];
  okm_words_to_scalar(y, okm);
}
// the big-endian words of a point's modern compressed encoding, straight from the canonical coordinate (no byte buffer)
BLS_FN void fp_be_words(uint32_t* w, const fp& a_mont) {
  fp t;
  uint32_t ww[12];
  fp_from_mont(t, a_mont);
  fp_get_words(ww, t);
#pragma unroll
  for (int j = 0; j < 12; j++) w[j] = ww[11 - j];
}
BLS_FN void pok_point_words(uint32_t (&w)[12], const g1_aff& a) {
  if (a.inf) {
#pragma unroll
    for (int j = 0; j < 12; j++) w[j] = 0;
    w[0] = 0xc0000000u;
    return;
  }
  fp_be_words(w, a.x);
  w[0] |= 0x80000000u | (fp_lex_largest(a.y) ? 0x20000000u : 0u);
}
BLS_FN void pok_point_words(uint32_t (&w)[24], const g2_aff& a) {
  if (a.inf) {
#pragma unroll
    for (int j = 0; j < 24; j++) w[j] = 0;
    w[0] = 0xc0000000u;
    return;
  }
  fp_be_words(w, a.x.c1);
  fp_be_words(w + 12, a.x.c0);
  w[0] |= 0x80000000u | (fp2_lex_largest(a.y) ? 0x20000000u : 0u);
}
// compute_y of a point in any projective scaling: the one inversion of the affine conversion, then the fixed shape
template <class F>
BLS_FN void pok_challenge_point(uint32_t y[8], const jac<F>& u, uint64_t t) {
  aff<F> a;
  a.inf = jac_is_inf(u);
  if (!a.inf) {               // jac_to_aff's body in place: only the inversion's two operands travel by reference
    F zi, zi2;
    fe_inv(zi, u.z);
    fe_sqr(zi2, zi);
    fe_mul(a.x, u.x, zi2);
    fe_mul(zi2, zi2, zi);
    fe_mul(a.y, u.y, zi2);
  }
  uint32_t w[sizeof(F) == sizeof(fp) ? 12 : 24];
  pok_point_words(w, a);
  pok_challenge_words(y, w, t);
}
// the timeout rule of verify_timestamp_proof (sig_proof.rs:154-161), tested before anything else: 0 leaves the item's status alone.
// The host calls it too (a batch whose every item trips the rule launches nothing else).
#if defined(__HIPCC__)
__host__ __device__ __forceinline__
#else
static inline
#endif
int pok_timeout_status(uint64_t t, uint64_t now_ms, int64_t timeout_ms) {
  if (timeout_ms < 0) return 0;
  if (t > now_ms) return -3;                              // BLSGPU_E_ARG: the reference panics (duration_since(..).unwrap())
  return now_ms - t > (uint64_t)timeout_ms ? 1 : 0;      // BLSGPU_INVALID_SIGNATURE = InvalidProof; elapsed == timeout passes
}

#if defined(__HIPCC__)
// ---- kernels (tu_pok.hip), one lane per item
__global__ void k_hash_to_scalar(size_t n, const uint8_t* msgs, const uint64_t* offs, const uint8_t* salt, uint32_t salt_len, uint8_t* out);
// bad: the decode statuses of wire-format commitments (null for the raw formats); an item that did not decode gets y = 0
template <int SG>
__global__ void k_proof_challenge(size_t n, const uint8_t* commitments, int fmt, const uint64_t* timestamps, const int32_t* bad, uint8_t* out_ys);
// after k_prepare_proof, before the pairing: the timeout rule first, then a decode failure (dec, null for the raw formats)
__global__ void k_proof_timeout(size_t n, const uint64_t* timestamps, uint64_t now_ms, int64_t timeout_ms, const int32_t* dec, int32_t* status);
#endif
