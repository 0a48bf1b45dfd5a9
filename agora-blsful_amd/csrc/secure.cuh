// Batched verify_secure: Signature::verify_secure / verify_secure_with_mode (reference src/signature.rs:177-197,256-276 ->
// src/secure_aggregation.rs:182-205,236-246) for many independent (keys, signature, message) sets in one call.
// Per set: the keys' bytes in stable byte-lexicographic order (:41-42), H = SHA-256 of that stream (:45-49), t_p =
// SHA-256(BE32(p) || H) mod r for sorted position p (:61-100), the key sum_p t_p pk_sorted[p] (:201-204) and core_verify.
// The kernels (tu_secure.inc) take the sets below BLSGPU_SECURE_BATCH_MAX keys; larger sets reuse the single call's machinery.
#pragma once
#include "verify.cuh"

// per-set flags: SECURE_F_ZERO by the coefficient lanes (atomicOr), the others by the host / k_set_out
#define SECURE_F_ZERO 1u        // some t_p is zero: BlsError::InvalidCoefficient (reference :97-100)
#define SECURE_F_LARGE 2u       // set by the host: the set runs through the one-set-at-a-time path, not these kernels
#define SECURE_F_IDSIG 4u       // the set's signature is the identity (what an empty set's verdict depends on, :189-195)

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
#endif
