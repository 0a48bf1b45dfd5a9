// Registered key sets (blsgpu_keyset_*, the *_indexed_batch entry points): a long-lived table of public keys on the device, and
// sets named as lists of positions in it.  Per entry the table keeps the affine record (RAW_AFFINE layout, all-zero for the
// identity AND for an invalid entry), the Modern compressed bytes and the status its deserialisation gave.
// Shared by the kernels (tu_keyset.inc), the library and the host harness (tests/hostsim_keyset):
//   * the fixed-base table of a key P: the affine points d 2^(4 j) P for the positive digits d = 1 .. 8 of a signed 4-bit window
//     and the windows j of ONE endomorphism sub-scalar (128 bits for G1 keys, 64 for G2 keys), plus the single point of the
//     carry window above them.  The E images of the endomorphism split (msm2.cuh) are derived from a table point when it is
//     used, so one table serves every sub-scalar;
//   * keyset_digit: the signed recoding of a sub-scalar, digits in [-7, 8], the carry of the top window leaving as one more digit
//     (0 or 1);
//   * keyset_pre_key / keyset_pre_status: what k_keyset_check leaves per set -- an out-of-range index first, then the creation
//     status of the first invalid entry in input order -- packed so that one atomicMin per position decides it;
//   * the line table of a G2 key (BLSGPU_KEYSET_LINES): the 68 normalised Miller rows of verify_shared.cuh, derived once at
//     creation, and the rule that says whether a set may have them;
//   * keyset_positions_check: which position lists blsgpu_keyset_update and blsgpu_keyset_append accept.
#pragma once
#include <algorithm>
#include <vector>
#include "multi_batch.cuh"
#include "verify_shared.cuh"

#define KEYSET_W 4
#define KEYSET_ROW 8                      // positive digits of a window: 1 .. 2^(W - 1)
#define KEYSET_SKIP 0xffffffffu           // an index k_keyset_check did not accept: the kernels after it read nothing for it
#define KEYSET_PRE_NONE 0xffffffffffffffffull
#define KEYSET_E_ARG (-3)                 // BLSGPU_E_ARG (include/blsgpu.h), in a status slot: the set names an index outside the table

// G: the keys' group.  WINDOWS counts the carry window; POINTS is the table's records per key.
template <int G>
struct keyset_shape;
template <>
struct keyset_shape<1> {
  enum { E = 2, WORDS = 2, FULL = 32, WINDOWS = 33, POINTS = 32 * KEYSET_ROW + 1, REC_BYTES = 96 };
};
template <>
struct keyset_shape<2> {
  enum { E = 4, WORDS = 1, FULL = 16, WINDOWS = 17, POINTS = 16 * KEYSET_ROW + 1, REC_BYTES = 192 };
};

// digit j of the sub-scalar a (`words` 64-bit words), recoded from the low end: the caller walks j upwards from 0 with carry = 0
// and threads `carry` through.  Window j = 16 words (one past the value) holds the carry alone.
BLS_FN int keyset_digit(const uint64_t* a, int words, int j, uint32_t& carry) {
  const int wi = j >> 4, sh = (j & 15) * KEYSET_W;
  const uint32_t v = wi < words ? (uint32_t)(a[wi] >> sh) & 15u : 0u;
  int d = (int)v + (int)carry;
  if (d > KEYSET_ROW) {
    d -= 2 * KEYSET_ROW;
    carry = 1;
  } else {
    carry = 0;
  }
  return d;
}
// the record of |d| 2^(4 j) P in a key's table (d != 0; in the carry window, j == full, d is 1)
BLS_FN uint32_t keyset_record(int j, int dabs) { return (uint32_t)(j * KEYSET_ROW + dabs - 1); }

BLS_FN uint64_t keyset_pre_key(bool out_of_range, uint64_t pos_in_set, int32_t entry_status) {
  if (out_of_range) return 0;
  if (entry_status != 0) return ((pos_in_set + 1) << 8) | (uint64_t)(entry_status & 0xff);
  return KEYSET_PRE_NONE;
}
BLS_FN int32_t keyset_pre_status(uint64_t key) { return key == 0 ? KEYSET_E_ARG : (int32_t)(key & 0xff); }

// ---- line tables per key (Bls12381G1Impl: keys in G2).  One verification is e(H'(m), pk) e(sig, -[c] g2) = 1, and a registered
// key is known long before any signature: its rows (n0, c)_e = (l0 / h, g / h)_e are group_lines_build's, SHARED_TABLE_WORDS words
// per entry in the *_LINES_N layout, entry k's row e at word (k 68 + e) 4 FP_NL.  The line kernel (kernels.cuh k_lines2s_keyed)
// reaches a row by a 32-bit BYTE offset from a wave-uniform base, so the whole table stays below 2^32 bytes: 281,970 keys.
#define KEYSET_LINES_KEY_BYTES ((uint64_t)SHARED_TABLE_WORDS * 4)
#define KEYSET_NOLINES_EMPTY 1            // the identity or an invalid entry: no verification under it reaches the line kernel
#define KEYSET_NOLINES_FINITE 2           // a finite point whose walk met h = 0 (no key of order r; trusted raw input only)
// may a set of n_keys keys have line tables?  other_bytes: its fixed-base tables, which share the cap of cap_mib MiB (a host rule:
// the library and the host harness call it)
static inline bool keyset_lines_fit(uint64_t n_keys, uint64_t other_bytes, uint64_t cap_mib) {
  if (n_keys == 0 || n_keys > 0xffffffffull / KEYSET_LINES_KEY_BYTES) return false;
  return n_keys * KEYSET_LINES_KEY_BYTES + other_bytes <= cap_mib << 20;
}
// The positions of one blsgpu_keyset_update over a set of n_keys entries, or (pos == nullptr) the tail [n_keys, n_keys + count) that
// blsgpu_keyset_append adds: every lane of the positional kernels writes the rows of its own entry, so a list is accepted only when
// all positions are below n_keys and no two are equal; an append only while the grown set keeps fewer than 2^32 - 1 entries (as at
// creation: KEYSET_SKIP stays free).  Range is decided before duplicates.  (A host rule: the library and the host harness call it.)
#define KEYSET_POS_OK 0
#define KEYSET_POS_RANGE 1                // a position not below the set's size
#define KEYSET_POS_DUP 2                  // the same position twice
#define KEYSET_POS_FULL 3                 // an append past 2^32 - 2 entries
static inline int keyset_positions_check(const uint32_t* pos, uint64_t count, uint64_t n_keys) {
  if (!pos) return n_keys >= 0xffffffffull || count >= 0xffffffffull - n_keys ? KEYSET_POS_FULL : KEYSET_POS_OK;
  for (uint64_t i = 0; i < count; i++)
    if ((uint64_t)pos[i] >= n_keys) return KEYSET_POS_RANGE;
  std::vector<uint32_t> sorted(pos, pos + count);
  std::sort(sorted.begin(), sorted.end());
  return std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end() ? KEYSET_POS_DUP : KEYSET_POS_OK;
}
BLS_FN void keyset_raw_hfp2(hfp2& r, const uint32_t* w) {
#if defined(__HIPCC__)
  fp_from_raw(r.v, w + (lane_hi() ? 12 : 0));
#else
  fp_from_raw(r.c[0], w);
  fp_from_raw(r.c[1], w + 12);
#endif
}
// the rows of the entry whose stored record (RAW_AFFINE G2, 48 words, all-zero for the identity and for an invalid entry) is rec,
// through io (group_lines_build's); 0 when they are usable, else KEYSET_NOLINES_*
template <class IO>
BLS_FN int keyset_lines_entry(const uint32_t* rec, const IO& io) {
  bool inf = true;
  for (int k = 0; k < 48; k++) inf = inf && rec[k] == 0;
  hfp2 qx, qy;
  keyset_raw_hfp2(qx, rec);
  keyset_raw_hfp2(qy, rec + 24);
  const bool ok = group_lines_build(qx, qy, inf, io);
  return ok ? 0 : inf ? KEYSET_NOLINES_EMPTY : KEYSET_NOLINES_FINITE;
}

#if defined(__HIPCC__)
#include "kernels.cuh"
// ---- kernels (tu_keyset1.hip: the group-independent ones and G1 keys, tu_keyset2.hip: G2 keys)
// create: any raw format -> the stored affine record and Modern bytes; an entry whose status is not OK becomes the zero record
template <int G>
__global__ void k_keyset_seal(size_t n, const uint8_t* pts, int fmt, const int32_t* status, uint8_t* recs, uint8_t* comp);
// update / append: the same per key, input key l (and status[l]) into entry pos[l]; the entry's creation status becomes status[l]
template <int G>
__global__ void k_keyset_seal_at(size_t n, const uint8_t* pts, int fmt, const int32_t* status, const uint32_t* pos, uint8_t* recs, uint8_t* comp,
                                 int32_t* kstatus);
// create, with tables: the multiples of keys [k0, k0 + cnt) as Jacobian points in jac_ws, their running Z products in prod_ws
// (POINTS records per lane each), one inversion per lane, the affine records into table
template <int G>
__global__ void k_keyset_build(size_t k0, size_t cnt, const uint8_t* recs, uint8_t* jac_ws, uint8_t* prod_ws, uint8_t* table);
// update / append: lane l builds the table of entry pos[l]; workspace rows by l, table rows by pos[l]
template <int G>
__global__ void k_keyset_build_at(size_t cnt, const uint32_t* pos, const uint8_t* recs, uint8_t* jac_ws, uint8_t* prod_ws, uint8_t* table);
// create, with line tables (G2 keys): one lane pair per key of [k0, k0 + cnt) runs keyset_lines_entry into the key's rows of
// `table`; scratch: SHARED_TABLE_WORDS words per key of the CHUNK; nolines[k] = 0 or KEYSET_NOLINES_*
__global__ void k_keyset_lines(size_t k0, size_t cnt, const uint8_t* recs, uint32_t* table, uint32_t* scratch, int32_t* nolines);
// update / append: lane pair l builds the rows of entry pos[l]; scratch rows by l, table rows and nolines by pos[l]
__global__ void k_keyset_lines_at(size_t cnt, const uint32_t* pos, const uint8_t* recs, uint32_t* table, uint32_t* scratch, int32_t* nolines);
// per position: the index against the table's size and the entry's status; cidx[i] = idx[i] or KEYSET_SKIP, pre[set] by atomicMin
// (offs == nullptr: every position is its own set).  nolines != nullptr (a set with line tables): *walk |= 1 when a position names
// a finite entry without usable rows (the caller clears the word before the launch)
__global__ void k_keyset_check(size_t n, const uint64_t* offs, size_t n_sets, const uint32_t* idx, uint64_t n_keys, const int32_t* kstatus,
                               uint32_t* cidx, unsigned long long* pre, const int32_t* nolines, uint32_t* walk);
__global__ void k_keyset_fin(size_t n_sets, const unsigned long long* pre, int32_t* status);
// ... and over a call that also reports two aux words per set (blsgpu_aggregate_verify_indexed_batch): a set the precedence decides
// gets aux (0, 0); aux may be null
__global__ void k_keyset_fin_aux(size_t n_sets, const unsigned long long* pre, int32_t* status, uint64_t* aux);
// dst record i = src record cidx[i] (words 32-bit words each; zeros for KEYSET_SKIP); legacy: the Dash header transcode of byte 0
__global__ void k_keyset_gather(size_t n, size_t words, const uint32_t* cidx, const uint32_t* src, int legacy, uint32_t* dst);
// RAW_AFFINE -> RAW_PROJ (blsgpu_keyset_get)
template <int G>
__global__ void k_keyset_to_proj(size_t n, const uint8_t* recs, uint8_t* out);
// the strip sum of multi_batch.cuh over table[cidx[i]]: every addition is the mixed one
template <int G>
__global__ void k_keyset_accumulate_seg(size_t n_strips, const uint8_t* recs, const uint32_t* cidx, const uint64_t* key_offs,
                                        const uint64_t* strip_offs, const uint32_t* strip_sid, uint8_t* part);
template <>
__global__ void k_keyset_accumulate_seg<1>(size_t, const uint8_t*, const uint32_t*, const uint64_t*, const uint64_t*, const uint32_t*, uint8_t*);
template <>
__global__ void k_keyset_accumulate_seg<2>(size_t, const uint8_t*, const uint32_t*, const uint64_t*, const uint64_t*, const uint32_t*, uint8_t*);
// part[i] = scal[i] * key[cidx[i]]: TAB = 1 from the fixed-base table, TAB = 0 by share_ladder.  With sid / flags (the batched
// verify_secure) a set that carries a flag leaves the identity, as k_share_ladder.
template <int G, int TAB>
__global__ void k_keyset_mul(size_t n, const uint8_t* recs, const uint8_t* table, const uint32_t* cidx, const uint8_t* scal, const uint32_t* sid,
                             const uint32_t* flags, uint8_t* part);
#endif
