// TEST-ONLY harness (see tests/hostsim/hostsim.cpp): the G1 map of csrc/h2c.cuh with the affine isogeny, compiled as host C++ with
// the bound tracker on -- sswu_g1 with the inverse of xd out of its square-root chain, iso_map_g1 at x = xn / xd, and the whole of
// hash_to_g1_map -- on caller-chosen uniform bytes.  Never linked into libblsgpu.so.
#include <string.h>
#include "../../agora-blsful_amd/csrc/h2c.cuh"

extern "C" {
// one 64-byte block -> u; out: xn, y, xinv of sswu_g1_inv with xd of sswu_g1 in between -- xn, xd, y, xinv, 4 x 12 caller-format
// words -- then x = xn xinv, then the Jacobian X, Y, Z of iso_map_g1(x, y) (8 x 12 words in all)
void hs_affine_map(const uint8_t* block, uint32_t* out) {
  uint32_t w[16];
  for (int i = 0; i < 16; i++) w[i] = be32_at(block + 4 * i);
  fp u, xn, xd, y, xinv, x;
  fp_from_be64_words(u, w);
  sswu_g1(xn, xd, y, u);
  sswu_g1_inv(xn, xinv, y, u);
  fp_mul(x, xn, xinv);
  g1_jac r;
  iso_map_g1(r, x, y);
  fp_to_raw(out, xn); fp_to_raw(out + 12, xd); fp_to_raw(out + 24, y); fp_to_raw(out + 36, xinv); fp_to_raw(out + 48, x);
  fp_to_raw(out + 60, r.x); fp_to_raw(out + 72, r.y); fp_to_raw(out + 84, r.z);
}
// the form without the inverse (what the row-wide engine's callers use, here on fp): xn, xd, y
void hs_sswu_plain(const uint8_t* block, uint32_t* out) {
  uint32_t w[16];
  for (int i = 0; i < 16; i++) w[i] = be32_at(block + 4 * i);
  fp u, xn, xd, y;
  fp_from_be64_words(u, w);
  sswu_g1(xn, xd, y, u);
  fp_to_raw(out, xn); fp_to_raw(out + 12, xd); fp_to_raw(out + 24, y);
}
// hash_to_g1_map, the one-lane form, on 128 uniform bytes: RAW_PROJ words (36; Jacobian, Z = 0 for the identity)
void hs_affine_hash_map(const uint8_t* uniform, int no_clear, uint32_t* out) {
  uint32_t w[32];
  for (int i = 0; i < 32; i++) w[i] = be32_at(uniform + 4 * i);
  g1_jac h;
  hash_to_g1_map(h, w, -1, no_clear != 0);
  fp_to_raw(out, h.x); fp_to_raw(out + 12, h.y); fp_to_raw(out + 24, h.z);
}
}
