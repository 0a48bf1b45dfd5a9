// Registered message sets (blsgpu_msgset_*, blsgpu_verify_msgset_batch, blsgpu_verify_msgset_indexed_batch): a long-lived table of
// HASHED messages on the device, and groups of (key, signature) items named by a position in it.  Per entry the table keeps what a
// shared-message call (verify_shared.cuh) computes per group before its items start: the hash-to-curve point of the message under
// the set's scheme as a RAW_AFFINE record -- Bls12381G1Impl: the point before the cofactor clearing (its verifications pair the
// signature with -[c] g2), Bls12381G2Impl: the cleared point -- all-zero for the identity.  With BLSGPU_MSGSET_LINES a Bls12381G2Impl
// set also keeps the 68 normalised Miller rows of every entry (group_lines_build: the *_LINES_N layout, entry k's row e at word
// (k 68 + e) 4 FP_NL, what a key set keeps per G2 key), so that a verification under a registered message walks the signature alone.
// Shared by the kernels (tu_msgset.inc, tu_coop_rows.hip) and the library:
//   * MSGSET_SKIP / msgset_entry_of: a group's sanitised entry;
//   * the kernels' declarations.
#pragma once
#include "keyset.cuh"

#define MSGSET_SKIP 0xffffffffu           // a group whose index k_msgset_check did not accept: nothing is read for it
#define MSGSET_E_ARG (-3)                 // BLSGPU_E_ARG (include/blsgpu.h), in a status slot: the item's group names no entry
#define MSGSET_ENTRY_LINE_BYTES KEYSET_LINES_KEY_BYTES

// the entry a group names, or MSGSET_SKIP
BLS_FN uint32_t msgset_entry_of(uint32_t msg_idx, uint64_t n_msgs) { return (uint64_t)msg_idx < n_msgs ? msg_idx : MSGSET_SKIP; }

#if defined(__HIPCC__)
#include "kernels.cuh"
// ---- kernels (tu_msgset1.hip: the group-independent ones and Bls12381G1Impl, tu_msgset2.hip: Bls12381G2Impl; tu_coop_rows.hip)
// create / update / append: hash output l (RAW_PROJ, group SG) -> the RAW_AFFINE record of entry pos[l] (pos == nullptr: first + l),
// all-zero for the identity; one inversion per entry
template <int SG>
__global__ void k_msgset_seal(size_t cnt, const uint8_t* hashes, const uint32_t* pos, size_t first, uint8_t* recs);
// per group: cmsg[g] = msg_idx[g], or MSGSET_SKIP outside the set.  nolines != nullptr (a set with rows, a call that may read them):
// *walk |= 1 when a group names an entry without usable rows (the caller clears the word before the launch)
__global__ void k_msgset_check(size_t n_groups, const uint32_t* msg_idx, uint64_t n_msgs, const int32_t* nolines, uint32_t* cmsg, uint32_t* walk);
// per item, with group_of[i] the item's group: a skipped group puts MSGSET_E_ARG into status[i] (before the pairing, which then skips
// the item, and once more after a key set's precedence, which it outranks); msg_of != nullptr: the item's entry (0 for a skipped one)
__global__ void k_msgset_mark(size_t n, const uint32_t* group_of, const uint32_t* cmsg, int32_t* status, uint32_t* msg_of);
// One wave per item, Bls12381G2Impl: pair 0 is (pk, H(m)) with H(m)'s rows read from `table` at the 32-bit WORD offset
// msg_of[i] 68 4 FP_NL from a wave-uniform base (the host keeps the table below 2^32 bytes), pair 1 is (-g1, sig), walked
// (coop_rows.cuh).  The record's pair-0 Q is not read.  easy == nullptr: final exponentiation and verdict into status[i]; else the
// easy-part value in k_pairing_coop_easy's layout and status stays as it is.  An item that is not BLS_OK on entry reads nothing.
__global__ void k_pairing_coop_rows(size_t n, const uint32_t* pairs, int32_t* status, const uint32_t* table, const uint32_t* msg_of, uint32_t* easy);
#endif
