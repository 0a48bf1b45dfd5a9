// Registered signature sets (blsgpu_sigset_*, blsgpu_pairing_sigset_batch, blsgpu_timecrypt_open_indexed_batch): a long-lived, growing
// table of round SIGNATURES on the device, and time-lock ciphertexts (or bare points) that name one by position.  Per entry the table
// keeps what blsgpu_timecrypt_open_batch works out per group before its items start: the signature as a RAW_AFFINE record of its group
// (all-zero for the identity AND for an entry that did not decode), its scheme tag and its creation status -- on the wire formats
// the decode status, subgroup test included, as k_decompress gives it.  With BLSGPU_SIGSET_LINES a Bls12381G2Impl set also keeps the
// 68 normalised Miller rows of every entry (group_lines_build: the *_LINES_N layout, entry k's row e at word (k 68 + e) 4 FP_NL, what
// a key set keeps per G2 key and a message set per hashed message), so that K = e(u, sig) evaluates rows at u and walks nothing
// (coop_row1.cuh).
// Shared by the kernels (tu_sigset.hip) and the library:
//   * SIGSET_E_ARG: an item that names no entry;
//   * the kernels' declarations.
#pragma once
#include "keyset.cuh"

#define SIGSET_E_ARG (-3)                 // BLSGPU_E_ARG (include/blsgpu.h), in a status slot: the item's index lies outside the set
#define SIGSET_ENTRY_LINE_BYTES KEYSET_LINES_KEY_BYTES

#if defined(__HIPCC__)
#include "kernels.cuh"
// ---- kernels (tu_sigset.hip)
// create / append: input signature l (any raw format of group SG; RAW_PROJ from k_decompress on the wire formats) -> entry first + l:
// its RAW_AFFINE record, all-zero for the identity and -- dec != nullptr, dec[l] != BLS_OK -- for a point that did not decode, which
// is never read; est[first + l] = dec ? dec[l] : BLS_OK
template <int SG>
__global__ void k_sigset_seal(size_t cnt, const uint8_t* pts, int fmt, const int32_t* dec, size_t first, uint8_t* recs, int32_t* est);
// One lane per item of either call over a set of n_entries entries (recs, tags, est as above).  k = idx[i]; pts: the items' other
// members (group 3 - SG) in format fmt, dec_pt their decode statuses (null for the raw formats).
//   k outside the set: status[i] = SIGSET_E_ARG, flag[i] = PV_ZERO, ent[i] = 0; nothing of the set is read.
//   ct_schemes != nullptr (blsgpu_timecrypt_open_indexed_batch): status[i] = the first that applies of dec_pt[i], est[k],
//     BLS_ERR_INVALID_SCHEME (ct_schemes[i] != tags[k]), BLS_ERR_SIG_IDENTITY, BLS_ERR_PK_IDENTITY, BLS_OK -- k_timecrypt_prepare's
//     order under the entry's signature and tag; an OK item gets flag PV_RUN, every other PV_ZERO.
//   ct_schemes == nullptr (blsgpu_pairing_sigset_batch): status[i] = the decode status of the G1 member, then of the G2 member, with
//     flag PV_ZERO; else BLS_OK and PV_ONE when a member is the identity, PV_RUN otherwise -- k_pairing_value_prepare's outcomes.
//   A PV_RUN item gets its pair, the G1 member first and both made affine, in the one-pair workspace (word-major, stride n), and
//   ent[i] = k, the entry whose rows k_pairing_value_rows reads.
//   nolines != nullptr (a set with rows): *walk |= 1 when an item names an entry inside the set without usable rows (the caller
//   clears the word before the launch).
template <int SG>
__global__ void k_sigset_prepare(size_t n, const uint32_t* idx, uint64_t n_entries, const uint8_t* recs, const uint8_t* tags, const int32_t* est,
                                 const int32_t* nolines, const uint8_t* pts, int fmt, const int32_t* dec_pt, const uint8_t* ct_schemes, uint32_t* pairs,
                                 int32_t* flag, int32_t* status, uint32_t* ent, uint32_t* walk);
// items first .. first + count - 1, one wave each, Bls12381G2Impl: coop_miller1_rows over the rows of entry ent[i], read from `table`
// at the 32-bit WORD offset ent[i] 68 4 FP_NL from a wave-uniform base (the host keeps the table below 2^32 bytes), then
// coop_final_value and coop_gt_bytes -> out_gt[576 i ..).  The workspace's Q is not read.  An item whose flag is not PV_RUN reads no
// table and gets k_pairing_value's constants.
__global__ void k_pairing_value_rows(size_t n, size_t first, size_t count, const uint32_t* pairs, const int32_t* flag, const uint32_t* table,
                                     const uint32_t* ent, uint8_t* out_gt);
// The Miller loop of the same tabled pair on the lane-split kernels (tu_millerf_rows1.hip), two lanes per item: items
// [first, first + count) of a batch of n, item i's line of entry e being n0 + (c xP) w^2 + (yP, 0) w^3 with (n0, c) row e of set entry
// ent[i], read at the same 32-bit word offset from a wave-uniform base.  Nothing is walked and nothing passes through the line
// workspace; conj(f) goes to item i of the Fp12 workspace fws (stride n), as k_millerfp3 leaves it.  An item whose flag is not PV_RUN
// returns before any table read.
__global__ void k_millerf_rows1(size_t n, size_t first, size_t count, const uint32_t* pairs, const int32_t* flag, const uint32_t* table, const uint32_t* ent,
                                uint32_t* fws);
#endif
