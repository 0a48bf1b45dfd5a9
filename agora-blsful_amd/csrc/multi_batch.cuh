// Batched multi verify: MultiSignature::verify (reference src/multi_signature.rs:127-135 over MultiPublicKey::from_public_keys,
// src/multi_public_key.rs:79-83 -> src/traits/pk_multi.rs:7-13) for many independent (keys, signature, message) sets in one call.
// Per set: the plain sum of its keys, then core_verify (src/traits/sig_core.rs:120-146) with that key.  The hot path is the
// SEGMENTED point sum over ragged sets (tu_multi_batch.inc):
//   * a STRIP is one accumulator lane's (G2 keys: lane pair's) share of one set.  With a strip length of L keys, set s of t_s keys
//     gets q_s = ceil(t_s / L) strips (an empty set none), numbered strip_offs[s] .. strip_offs[s + 1]; strip_sid[g] is strip
//     g's set.  Strip j of set s sums keys key_offs[s] + j, + q_s, + 2 q_s, ... -- interleaved like k_accumulate (kernels.cuh), so
//     that adjacent lanes read adjacent points -- into part[strip_offs[s] + j];
//   * the strips of a set are then folded by the segmented pairwise tree of the threshold recovery (k_share_fold, shares.cuh, over
//     strip_offs / strip_sid): ceil(log2 max q_s) launches, after which part[strip_offs[s]] is set s's key.
// The plan (multi_strip_len, multi_strip_plan) and the strip's key range (multi_strip_of) below are shared by the library and
// the host harness (tests/hostsim_multi_batch).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "shares.cuh"

// strip length for N keys in all: one strip per lane of a single sum over N points (`lanes`: accumulate_lanes(N) of blsgpu.hip,
// a quarter of the points, capped), never shorter than 4 keys; forced >= 1 (BLSGPU_MULTI_STRIP) overrides
static inline uint64_t multi_strip_len(uint64_t N, uint64_t lanes, uint64_t forced) {
  if (forced) return forced;
  const uint64_t l = lanes ? (N + lanes - 1) / lanes : N;
  return l < 4 ? 4 : l;
}
// strip_offs (n_sets + 1 prefix sums of q_s) and strip_sid (one set index per strip) from the key offsets (n_sets + 1 entries,
// non-decreasing); returns the largest q_s
static inline uint64_t multi_strip_plan(const uint64_t* key_offs, size_t n_sets, uint64_t L, std::vector<uint64_t>& strip_offs,
                                        std::vector<uint32_t>& strip_sid) {
  strip_offs.assign(n_sets + 1, 0);
  strip_sid.clear();
  uint64_t qmax = 0;
  for (size_t s = 0; s < n_sets; s++) {
    const uint64_t t = key_offs[s + 1] - key_offs[s], q = t / L + (t % L ? 1 : 0);
    strip_offs[s + 1] = strip_offs[s] + q;
    strip_sid.insert(strip_sid.end(), (size_t)q, (uint32_t)s);
    if (q > qmax) qmax = q;
  }
  return qmax;
}
// the keys of strip g: first, first + stride, ... below end
struct multi_strip {
  uint64_t first, stride, end;
};
BLS_FN multi_strip multi_strip_of(uint64_t g, const uint64_t* key_offs, const uint64_t* strip_offs, const uint32_t* strip_sid) {
  const uint32_t s = strip_sid[g];
  multi_strip st;
  st.first = key_offs[s] + (g - strip_offs[s]);
  st.stride = strip_offs[s + 1] - strip_offs[s];
  st.end = key_offs[s + 1];
  return st;
}

#if defined(__HIPCC__)
#include "kernels.cuh"
// G: the keys' group.  G = 1: one lane per strip; G = 2: one lane pair per strip (jac<hfp2>, as k_accumulate_g2s)
template <int G>
__global__ void k_multi_accumulate_seg(size_t n_strips, const uint8_t* pts, int fmt, const uint64_t* key_offs, const uint64_t* strip_offs,
                                       const uint32_t* strip_sid, uint8_t* part);
template <>
__global__ void k_multi_accumulate_seg<1>(size_t, const uint8_t*, int, const uint64_t*, const uint64_t*, const uint32_t*, uint8_t*);
template <>
__global__ void k_multi_accumulate_seg<2>(size_t, const uint8_t*, int, const uint64_t*, const uint64_t*, const uint32_t*, uint8_t*);
#endif
