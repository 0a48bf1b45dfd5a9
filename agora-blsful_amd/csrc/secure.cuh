// Batched verify_secure: Signature::verify_secure / verify_secure_with_mode (reference src/signature.rs:177-197,256-276 ->
// src/secure_aggregation.rs:182-205,236-246) for many independent (keys, signature, message) sets in one call.
// Per set: the keys' bytes in stable byte-lexicographic order (:41-42), H = SHA-256 of that stream (:45-49), t_p =
// SHA-256(BE32(p) || H) mod r for sorted position p (:61-100), the key sum_p t_p pk_sorted[p] (:201-204) and core_verify.
// The kernels (tu_secure.inc) take the sets below BLSGPU_SECURE_BATCH_MAX keys; larger sets reuse the single call's machinery.
// Batched secure aggregation (blsgpu_aggregate_secure_batch; aggregate_secure[_with_mode], reference
// src/secure_aggregation.rs:110-169,338-352) runs the same rank / gather / digest / coefficient kernels over the keys, then sums
// t_p sig[first_p] per set in the SIGNATURE group, where first_p is the first input position of the set whose key bytes equal
// those of the key at sorted position p (the reference's `position` search, :138-147): secure_first_tile below.
#pragma once
#include "verify.cuh"

// per-set flags: SECURE_F_ZERO by the coefficient lanes (atomicOr), the others by the host / k_set_out
#define SECURE_F_ZERO 1u        // some t_p is zero: BlsError::InvalidCoefficient (reference :97-100)
#define SECURE_F_LARGE 2u       // set by the host: the set runs through the one-set-at-a-time path, not these kernels
#define SECURE_F_IDSIG 4u       // the set's signature is the identity (what an empty set's verdict depends on, :189-195)

// ---- first occurrence of a key inside its set, shared by k_secure_first (tu_secure.inc) and the host harness
// (tests/hostsim_aggregate_batch).  Keys are WPK 32-bit words each (12 or 24), compared as they lie in memory.
template <int WPK>
BLS_FN bool secure_key_eq(const uint32_t* a, const uint32_t* b) {
  uint32_t d = 0;
  for (int k = 0; k < WPK; k++) d |= a[k] ^ b[k];
  return d == 0;
}
// One tile of key i's walk over its set [lo, ...): `tile` holds the keys t0 .. t0 + tile_keys - 1 of the flat array.  Returns the
// smallest j in the tile with lo <= j < best and key j == key i (`me`), else `best`.  A walk that starts from best = i and takes
// the tiles of i's set in any order ends at the first occurrence: i itself when no earlier key of the set equals it.  Keys of
// other sets that lie in the same tile (j < lo) are never compared.
template <int WPK>
BLS_FN uint32_t secure_first_tile(uint32_t best, const uint32_t* tile, size_t t0, size_t tile_keys, size_t lo, const uint32_t* me) {
  const size_t a = t0 > lo ? t0 : lo, e = t0 + tile_keys < (size_t)best ? t0 + tile_keys : (size_t)best;
  for (size_t j = a; j < e; j++)
    if (secure_key_eq<WPK>(tile + (j - t0) * WPK, me)) return (uint32_t)j;     // ascending: the first hit is the tile's smallest
  return best;
}

#if defined(__HIPCC__)
// one lane per key (the rank kernel: n-body tiles over the set, split over gridDim.y); WPK = 32-bit words per key (12 or 24)
template <int WPK>
__global__ void k_secure_rank(size_t n, const uint64_t* offs, size_t n_sets, const uint8_t* kb, const uint32_t* flags, uint32_t* rank,
                              uint32_t* sid);
__global__ void k_secure_gather(size_t n, size_t width, const uint64_t* offs, const uint8_t* kb, const uint32_t* rank, const uint32_t* sid,
                                const uint32_t* flags, uint8_t* sorted);
// one wave per set
__global__ void k_secure_digest(size_t n_sets, size_t width, const uint64_t* offs, const uint8_t* sorted, const uint32_t* flags, uint8_t* H);
__global__ void k_secure_coeff(size_t n, const uint32_t* rank, const uint32_t* sid, const uint8_t* H, uint32_t* flags, uint8_t* scal);
// one lane per set: the signature as RAW_PROJ, the set's summed key part[part_offs[s]] (the identity for an empty set), its status
// before the verification tail (flags may be null: BLS_OK, the batched multi verify); after the tail, the verdict of the empty sets
template <int SG>
__global__ void k_set_out(size_t n_sets, const uint64_t* key_offs, const uint64_t* part_offs, uint32_t* flags, const uint8_t* part,
                          const uint8_t* sigs, int fmt, uint8_t* sig_proj, uint8_t* apk, int32_t* status);
__global__ void k_secure_fin(size_t n_sets, const uint64_t* offs, const uint32_t* flags, int32_t* status);
// ---- batched aggregation (blsgpu_aggregate_secure_batch, blsgpu_sum_batch)
// one lane per key, after k_secure_rank (which fills sid): first[i] = the flat index of the first key of i's set with i's bytes;
// first is preset to ~0 by the caller, the gridDim.y slices of a set meet in it by atomicMin
template <int WPK>
__global__ void k_secure_first(size_t n, const uint64_t* offs, const uint8_t* kb, const uint32_t* sid, const uint32_t* flags, uint32_t* first);
// one lane per key: part[i] = scal[i] * sigs[first[i]] in group G (the joint NAF ladder of shares.cuh); the identity for a flagged set
template <int G>
__global__ void k_secure_ladder(size_t n, const uint8_t* sigs, int fmt, const uint8_t* scal, const uint32_t* first, const uint32_t* sid,
                                const uint32_t* flags, uint8_t* part);
// one lane per set: out[s] = part[part_offs[s]] (RAW_PROJ of group G), all-zero -- the identity -- for an empty set or a set with
// SECURE_F_ZERO; status[s] = OK or INVALID_COEFFICIENT.  flags and status may be null (blsgpu_sum_batch: no verdicts)
template <int G>
__global__ void k_set_sum_out(size_t n_sets, const uint64_t* key_offs, const uint64_t* part_offs, const uint32_t* flags, const uint8_t* part,
                              uint8_t* out, int32_t* status);
#endif
