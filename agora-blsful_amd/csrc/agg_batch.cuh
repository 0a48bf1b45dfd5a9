// Batched aggregate verify: AggregateSignature::verify (reference src/aggregate_signature.rs:230-239 -> src/traits/sig_basic.rs:46-58,
// src/traits/sig_core.rs:149-178) for many independent (keys, messages, signature) sets in one call.
// The sets below BLSGPU_AGG_BATCH_MAX pairs ("batched sets", b = 0 .. n_b) run through the kernels of tu_agg_batch.inc as ONE flat
// list of M = T_b + n_b items: the T_b (key, message) pairs first, set after set (set b owns items boffs[b] .. boffs[b + 1]), then
// one signature item per set (item T_b + b).  sid[i] is the set of pair item i, src[i] its index in the caller's pks / msg_offsets,
// bset[b] the set's index in the caller's sigs / status / aux.  Larger sets reuse the single call's machinery.
// The per-item functions below are shared by the kernels and the host harness (tests/hostsim_agg_batch):
//   * agg_dup_insert / agg_dup_find: Basic's duplicate-message rule per set, the open-addressing table of k_dup_insert / k_dup_find
//     (util_kernels.cuh) keyed by (set, message bytes);
//   * agg_first_bad_item: per set, the first identity key and whether the signature is the identity;
//   * agg_fold_partner: which item multiplies into which in round r of the segmented product;
//   * agg_decide: the reference's precedence;
//   * agg_batch_plan / agg_flat_pair / agg_flat_key: which sets are batched, where flat item i lies in the caller's arrays, and --
//     for a call over a registered key set (blsgpu_aggregate_verify_indexed_batch) -- which entry of the set is its key.
#pragma once
#include <stddef.h>
#include "verify.cuh"

#define AGG_NONE 0xffffffffu      // no index: an empty table slot, a set without a duplicate / an identity key

#if defined(__HIPCC__)
#define AGG_CAS(p, cmp, v) atomicCAS(p, cmp, v)
#define AGG_MIN(p, v) atomicMin(p, v)
#else                             // the host harness runs the items one after another
static inline uint32_t AGG_CAS(uint32_t* p, uint32_t cmp, uint32_t v) {
  const uint32_t old = *p;
  if (old == cmp) *p = v;
  return old;
}
static inline void AGG_MIN(uint32_t* p, uint32_t v) {
  if (v < *p) *p = v;
}
#endif

// 64-bit hash of (set, message bytes); the length enters so that a prefix of a message hashes apart from it.  Whatever it does,
// the rule below stays exact: equality is confirmed on the set and the bytes.
BLS_FN uint64_t agg_msg_hash(uint32_t set, const uint8_t* p, size_t len) {
  uint64_t h = 0x9e3779b97f4a7c15ull ^ (len * 0xff51afd7ed558ccdull) ^ ((uint64_t)set * 0xd6e8feb86659fd93ull);
  for (size_t k = 0; k < len; k++) {
    h = (h ^ p[k]) * 0x100000001b3ull;
    h ^= h >> 29;
  }
  h *= 0xc4ceb9fe1a85ec53ull;
  return h ^ (h >> 32);
}
// Pair item i claims a slot of the table (tab, minidx: mask + 1 entries preset to AGG_NONE, more entries than items): the first
// claimant of a slot is the representative of its (set, message) class, a later one compares set, length and bytes with it and
// moves on when they differ; every member lowers the slot's minimum item index.  Returns the slot.  A zero-length message is a
// message like any other (one class per set), as in the reference's HashMap<Vec<u8>, usize>.
BLS_FN uint32_t agg_dup_insert(uint32_t i, const uint8_t* msgs, const uint64_t* moffs, const uint32_t* sid, const uint32_t* src, uint32_t mask,
                               uint32_t* tab, uint32_t* minidx) {
  const uint32_t b = sid[i];
  const uint8_t* p = msgs + moffs[src[i]];
  const size_t len = (size_t)(moffs[src[i] + 1] - moffs[src[i]]);
  uint32_t s = (uint32_t)agg_msg_hash(b, p, len) & mask;
  for (;;) {
    uint32_t rep = AGG_CAS(&tab[s], AGG_NONE, i);
    if (rep == AGG_NONE) rep = i;
    bool eq = rep == i;
    if (!eq && sid[rep] == b && (size_t)(moffs[src[rep] + 1] - moffs[src[rep]]) == len) {
      const uint8_t* q = msgs + moffs[src[rep]];
      eq = true;
      for (size_t k = 0; k < len; k++) eq = eq && p[k] == q[k];
    }
    if (eq) break;
    s = (s + 1) & mask;
  }
  AGG_MIN(&minidx[s], i);
  return s;
}
// after every insert: the reference's i of set b is the smallest LOCAL index whose class holds an earlier item (best[b], preset
// to AGG_NONE), and its `old` is that class's minimum
BLS_FN void agg_dup_find(uint32_t i, const uint32_t* sid, const uint64_t* boffs, const uint32_t* slot_of, const uint32_t* minidx, uint32_t* best) {
  if (minidx[slot_of[i]] < i) AGG_MIN(&best[sid[i]], i - (uint32_t)boffs[sid[i]]);
}
// item i of the M = T_b + n_b items: a pair item lowers its set's first identity key (local index; first preset to AGG_NONE), a
// signature item states whether the set's signature is the identity
BLS_FN void agg_first_bad_item(size_t i, size_t T_b, const uint32_t* sid, const uint64_t* boffs, const int32_t* bad, uint32_t* first, uint32_t* sig_id) {
  if (i >= T_b) sig_id[i - T_b] = bad[i] ? 1u : 0u;
  else if (bad[i]) AGG_MIN(&first[sid[i]], (uint32_t)(i - boffs[sid[i]]));
}
// Segmented product, the halving of k_f12_fold per set: before round r a set of len items holds cur = ceil(len / 2^r) live values
// at its first cur items; the round multiplies item l + half into item l for every l with l + half < cur (half = ceil(cur / 2)).
// No item is read and written in the same round, and after agg_fold_rounds(len) rounds the product is at the set's first item.
BLS_FN bool agg_fold_partner(uint64_t len, int r, uint64_t l, uint64_t* partner) {
  const uint64_t cur = (len + (((uint64_t)1 << r) - 1)) >> r, half = (cur + 1) >> 1;
  if (l + half >= cur) return false;
  *partner = l + half;
  return true;
}
static inline int agg_fold_rounds(uint64_t len) {
  int r = 0;
  while (((len + (((uint64_t)1 << r) - 1)) >> r) > 1) r++;
  return r;
}
// The verdict of a set before its pairing product counts (reference order: sig_basic.rs:46-58, then sig_core.rs:155-167): BLS_OK
// means "the product decides".  dup_i / dup_old: the duplicate pair (AGG_NONE: none; never set outside Basic), first_bad: the
// first identity key.  aux gets the indices of the single call: (old, i) 0-based, or the key's 1-based index, else (0, 0).
BLS_FN int32_t agg_decide(uint32_t dup_old, uint32_t dup_i, bool sig_is_id, uint32_t first_bad, uint64_t aux[2]) {
  aux[0] = aux[1] = 0;
  if (dup_i != AGG_NONE) {
    aux[0] = dup_old;
    aux[1] = dup_i;
    return BLS_ERR_DUPLICATE_MESSAGE;
  }
  if (sig_is_id) return BLS_ERR_SIG_IDENTITY;
  if (first_bad != AGG_NONE) {
    aux[0] = (uint64_t)first_bad + 1;
    return BLS_ERR_PK_IDENTITY;
  }
  return BLS_OK;
}

// The plan of a call (host): set s of offs[s] .. offs[s + 1] is batched when it has fewer than max_small pairs, else large.  The
// batched sets form the flat list in the caller's order: boffs (their item ranges in it, n_b + 1 entries), bsrc (where a set's pairs
// start in the caller's arrays), bset (its index in the caller's sigs / status / aux).  Returns the largest batched set's size.
template <class V64, class V32, class VSZ>
static inline uint64_t agg_batch_plan(const uint64_t* offs, size_t n_sets, uint64_t max_small, V64& boffs, V64& bsrc, V32& bset, VSZ& large,
                                      uint64_t* tmax_large) {
  uint64_t tmax_b = 0;
  *tmax_large = 0;
  boffs.assign(1, 0);
  for (size_t s = 0; s < n_sets; s++) {
    const uint64_t t = offs[s + 1] - offs[s];
    if (t >= max_small) {
      large.push_back(s);
      if (t > *tmax_large) *tmax_large = t;
    } else {
      bsrc.push_back(offs[s]);
      bset.push_back((uint32_t)s);
      boffs.push_back(boffs.back() + t);
      if (t > tmax_b) tmax_b = t;
    }
  }
  return tmax_b;
}
// pair item i of the flat list (i < T_b = boffs[n_b]), a member of batched set b: its index in the caller's pks / idx / msg_offsets
BLS_FN uint64_t agg_flat_pair(const uint64_t* boffs, const uint64_t* bsrc, uint32_t b, size_t i) { return bsrc[b] + (i - boffs[b]); }
// ... and, over a registered key set, the entry that is its key: the flat list REORDERS the caller's pairs (batched sets only, then
// the signature items), so the sanitised index cidx (one per caller position, k_keyset_check) is reached through src
// (k_prepare_agg_seg's map), never by the flat index itself
BLS_FN uint32_t agg_flat_key(const uint32_t* src, const uint32_t* cidx, size_t i) { return cidx[src[i]]; }
// The Miller values of the M flat items are formed in rounds of at most `round` items (one machine round of lane pairs), all of
// the same size, a multiple of 32: the round that starts at `first` takes the items first .. first + size, lane pair j the flat item
// first + j -- key_of, like the pairs and the flags, is indexed by that, not by j
static inline size_t agg_round_size(size_t M, size_t round) {
  const size_t n_rounds = (M + round - 1) / round;
  return n_rounds ? ((M + n_rounds - 1) / n_rounds + 31) / 32 * 32 : 0;
}

#if defined(__HIPCC__)
#include "kernels.cuh"
// two (or one) lanes per item: k_prepare_agg's item (kernels.cuh prepare_agg_item) for every item of the flat list; also writes sid / src
template <int SG>
__global__ void k_prepare_agg_seg(size_t M, size_t T_b, size_t n_b, const uint64_t* boffs, const uint64_t* bsrc, const uint32_t* bset,
                                  const uint8_t* pks, const uint8_t* sigs, int fmt, int aug, const uint8_t* msgs, const uint64_t* moffs, dst_arg dst,
                                  uint32_t* pairs, int32_t* bad, uint32_t* sid, uint32_t* src, int two_lanes);
// one lane per item
__global__ void k_first_bad_seg(size_t M, size_t T_b, const uint32_t* sid, const uint64_t* boffs, const int32_t* bad, uint32_t* first, uint32_t* sig_id);
__global__ void k_dup_insert_seg(size_t T_b, const uint8_t* msgs, const uint64_t* moffs, const uint32_t* sid, const uint32_t* src, uint32_t mask,
                                 uint32_t* tab, uint32_t* minidx, uint32_t* slot_of);
__global__ void k_dup_find_seg(size_t T_b, const uint32_t* sid, const uint64_t* boffs, const uint32_t* slot_of, const uint32_t* minidx, uint32_t* best);
// key_of[i] = agg_flat_key(src, cidx, i) for every pair item: what k_linesp_keyed (kernels.cuh) indexes by the flat index
__global__ void k_agg_flat_keys(size_t T_b, const uint32_t* src, const uint32_t* cidx, uint32_t* key_of);
// round r of the segmented product over the pair items of the Fp12 workspace; then, one lane per set, the set's product times its
// signature item as record b of a workspace of stride n_b
__global__ void k_f12_fold_seg(size_t T_b, int r, const uint32_t* sid, const uint64_t* boffs, uint32_t* fws, size_t stride);
__global__ void k_f12_fold_seg_out(size_t n_b, size_t T_b, const uint64_t* boffs, const uint32_t* fws, size_t stride, uint32_t* rec);
// one lane per set: the status the final exponentiation starts from (decided sets are non-OK and skipped), and after it the
// caller's status / aux entries (aux may be null)
__global__ void k_agg_batch_mark(size_t n_b, const uint64_t* boffs, const uint32_t* best, const uint32_t* slot_of, const uint32_t* minidx,
                                 const uint32_t* first, const uint32_t* sig_id, int32_t* st_b);
__global__ void k_agg_batch_fin(size_t n_b, const uint64_t* boffs, const uint32_t* bset, const uint32_t* best, const uint32_t* slot_of,
                                const uint32_t* minidx, const uint32_t* first, const uint32_t* sig_id, const int32_t* st_b, int32_t* status,
                                uint64_t* aux);
// one lane: a large set's results of the single call's kernels (aggregate_enqueue's first / verdict, k_dup_fin's pair) -> its entries
__global__ void k_agg_large_fin(size_t n, const int64_t* first, const int32_t* verdict, const uint64_t* dup2, int32_t* status, uint64_t* aux);
#endif
