// TEST-ONLY harness for tests/test_hostsim_pok_timestamp.py: compiles agora-blsful_amd/csrc/hkdf.cuh as plain host C++ with the
// bound tracker on, so that the `-m "not gpu"` suite checks HashToScalar's general form, the 48-byte reduction, the two fixed-shape
// register paths of compute_y and the precomputed key-block states without a GPU.  With -DPOK_HOSTSIM_MAIN it is a program of its
// own (the sanitizer leg): the same functions on inputs it makes itself, checked against each other.  Never linked into libblsgpu.so.
#include <stdio.h>
#include <string.h>
#include "../../agora-blsful_amd/csrc/verify.cuh"
#include "../../agora-blsful_amd/csrc/hkdf.cuh"

static void st_le(uint8_t* out, const uint32_t* y) {
  for (int j = 0; j < 8; j++)
    for (int k = 0; k < 4; k++) out[4 * j + k] = (uint8_t)(y[j] >> (8 * k));
}

extern "C" {
// the general form: out = 32 bytes little-endian
void hs_hkdf_scalar(const uint8_t* ikm, uint32_t ikm_len, const uint8_t* salt, uint32_t salt_len, uint8_t* out) {
  hkdf_scalar(out, ikm, ikm_len, salt, salt_len);
}
// 48 bytes big-endian -> the scalar
void hs_okm_to_scalar(const uint8_t* okm, uint8_t* out) {
  uint32_t w[12], y[8];
  for (int j = 0; j < 12; j++) w[j] = be32_at(okm + 4 * j);
  okm_words_to_scalar(y, w);
  st_le(out, y);
}
// the fixed shape on the bytes of a compressed point (48: G1, 96: G2)
void hs_challenge_bytes(int sg, const uint8_t* comp, uint64_t t, uint8_t* out) {
  uint32_t y[8];
  if (sg == 1) {
    uint32_t w[12];
    for (int j = 0; j < 12; j++) w[j] = be32_at(comp + 4 * j);
    pok_challenge_words(y, w, t);
  } else {
    uint32_t w[24];
    for (int j = 0; j < 24; j++) w[j] = be32_at(comp + 4 * j);
    pok_challenge_words(y, w, t);
  }
  st_le(out, y);
}
// what a lane of k_proof_challenge does: a RAW_PROJ point (blst words, any Z; Z = 0 the identity) -> affine -> words -> fixed shape.
// comp receives the words as bytes: the modern compressed encoding
void hs_challenge_point(int sg, const uint32_t* p, uint64_t t, uint8_t* out, uint8_t* comp) {
  uint32_t y[8];
  if (sg == 1) {
    g1_jac a;
    g1_aff f;
    uint32_t w[12];
    fp_from_raw(a.x, p); fp_from_raw(a.y, p + 12); fp_from_raw(a.z, p + 24);
    jac_to_aff(f, a);
    pok_point_words(w, f);
    for (int j = 0; j < 12; j++)
      for (int k = 0; k < 4; k++) comp[4 * j + k] = (uint8_t)(w[j] >> (24 - 8 * k));
    pok_challenge_point(y, a, t);
  } else {
    g2_jac a;
    g2_aff f;
    uint32_t w[24];
    fp_from_raw(a.x.c0, p); fp_from_raw(a.x.c1, p + 12); fp_from_raw(a.y.c0, p + 24); fp_from_raw(a.y.c1, p + 36);
    fp_from_raw(a.z.c0, p + 48); fp_from_raw(a.z.c1, p + 60);
    jac_to_aff(f, a);
    pok_point_words(w, f);
    for (int j = 0; j < 24; j++)
      for (int k = 0; k < 4; k++) comp[4 * j + k] = (uint8_t)(w[j] >> (24 - 8 * k));
    pok_challenge_point(y, a, t);
  }
  st_le(out, y);
}
// the two constant key-block states (out: 16 words, ipad then opad) and the same computed from the salt (out + 16)
void hs_midstates(uint32_t* out) {
  for (int j = 0; j < 8; j++) {
    out[j] = POK_IPAD_MID[j];
    out[8 + j] = POK_OPAD_MID[j];
  }
  for (int k = 0; k < 2; k++) {
    uint32_t w[16], h[8];
    uint8_t kb[64];
    memset(kb, 0, 64);
    memcpy(kb, POK_SALT, POK_SALT_LEN);
    for (int j = 0; j < 16; j++) w[j] = be32_at(kb + 4 * j) ^ (k ? 0x5c5c5c5cu : 0x36363636u);
    const hk_h iv = hk_iv();
    for (int j = 0; j < 8; j++) h[j] = iv[j];
    sha256_rounds(h, w);
    for (int j = 0; j < 8; j++) out[16 + 8 * k + j] = h[j];
  }
}
int hs_timeout_status(uint64_t t, uint64_t now_ms, int64_t timeout_ms) { return pok_timeout_status(t, now_ms, timeout_ms); }
}

#if defined(POK_HOSTSIM_MAIN)
static uint64_t g_s = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  g_s ^= g_s << 13;
  g_s ^= g_s >> 7;
  g_s ^= g_s << 17;
  return g_s;
}
int main() {
  int checks = 0, bad = 0;
  // the constant states are the salt's
  uint32_t mid[32];
  hs_midstates(mid);
  checks++;
  if (memcmp(mid, mid + 16, 64) != 0) bad++;
  // the general form at every length across the block and padding edges, every salt rule: canonical output, and deterministic
  static const uint32_t salt_lens[7] = {0, 1, 36, 63, 64, 65, 130};
  uint8_t msg[200], salt[130], a[32], b[32];
  for (int i = 0; i < 200; i++) msg[i] = (uint8_t)rnd();
  for (int i = 0; i < 130; i++) salt[i] = (uint8_t)rnd();
  for (uint32_t len = 0; len <= 200; len++)
    for (uint32_t sl : salt_lens) {
      hs_hkdf_scalar(msg, len, salt, sl, a);
      hs_hkdf_scalar(msg, len, salt, sl, b);
      uint32_t w[8];
      for (int j = 0; j < 8; j++) w[j] = a[4 * j] | a[4 * j + 1] << 8 | a[4 * j + 2] << 16 | (uint32_t)a[4 * j + 3] << 24;
      checks++;
      if (memcmp(a, b, 32) != 0 || !fr_words_canonical(w)) bad++;
    }
  // the reduction: 0, r and 3 r give zero (written, not looped on), 1 and r + 1 give one
  uint8_t okm[48], one[32] = {1}, zero[32] = {0};
  const uint8_t* want[5] = {zero, one, zero, one, zero};
  for (int k = 0; k < 5; k++) {
    uint32_t v[13] = {0};
    const int mul = k < 2 ? 0 : k < 4 ? 1 : 3, add = k & 1 && k < 4;
    uint64_t c = add;
    for (int j = 0; j < 12; j++) {
      c += (uint64_t)mul * (j < 8 ? FR_MOD[j] : 0);
      v[j] = (uint32_t)c;
      c >>= 32;
    }
    for (int j = 0; j < 12; j++)
      for (int q = 0; q < 4; q++) okm[4 * j + q] = (uint8_t)(v[11 - j] >> (24 - 8 * q));
    hs_okm_to_scalar(okm, a);
    checks++;
    if (memcmp(a, want[k], 32) != 0) bad++;
  }
  // the fixed shapes against the general form under the proof salt
  static const uint64_t ts[4] = {0, 1, 1ull << 32, ~0ull};
  for (int sg = 1; sg <= 2; sg++)
    for (int it = 0; it < 60; it++) {
      uint8_t in[96 + 8];
      const int nb = 48 * sg;
      for (int i = 0; i < nb; i++) in[i] = (uint8_t)rnd();
      if (it == 0) {
        memset(in, 0, nb);
        in[0] = 0xc0;
      }
      if (it == 1) memset(in + 1, 0, 3);
      const uint64_t t = it < 4 ? ts[it] : rnd();
      for (int k = 0; k < 8; k++) in[nb + k] = (uint8_t)(t >> (8 * k));
      hs_hkdf_scalar(in, nb + 8, (const uint8_t*)POK_SALT, POK_SALT_LEN, a);
      hs_challenge_bytes(sg, in, t, b);
      checks++;
      if (memcmp(a, b, 32) != 0) bad++;
    }
  // a point through the lane's path: the generator of G1 in blst words is not at hand here, so the identity (Z = 0) only
  uint32_t p[72] = {0};
  uint8_t comp[96];
  for (int sg = 1; sg <= 2; sg++) {
    uint8_t in[96 + 8] = {0xc0};
    for (int k = 0; k < 8; k++) in[48 * sg + k] = (uint8_t)((uint64_t)5 >> (8 * k));
    hs_hkdf_scalar(in, 48 * sg + 8, (const uint8_t*)POK_SALT, POK_SALT_LEN, a);
    hs_challenge_point(sg, p, 5, b, comp);
    checks++;
    if (memcmp(a, b, 32) != 0 || memcmp(comp, in, 48 * sg) != 0) bad++;
  }
  checks += 3;
  if (hs_timeout_status(10, 20, 10) != 0 || hs_timeout_status(9, 20, 10) != 1 || hs_timeout_status(21, 20, 10) != -3) bad++;
  printf("%d checks, %d bad\n", checks, bad);
  return bad ? 1 : 0;
}
#endif
