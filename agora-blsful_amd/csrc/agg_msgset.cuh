// Aggregate verify by message index (blsgpu_aggregate_verify_msgset_batch / _indexed_batch): AggregateSignature::verify for many
// sets in one call, pair i's message named as entry msg_idx[i] of a registered message set (msgset.cuh).  By bilinearity the pairs
// of one set that name the same message are one factor e(sum of their keys, H(m)), so the pairs of a set are grouped into CLASSES and
// the flat list of agg_batch.cuh is formed over classes: M = C + n_sets items, the C class items first, set after set (set b owns
// items coffs[b] .. coffs[b + 1]), then one signature item per set.  No message is hashed and the Miller stages of agg_batch.cuh run
// over the class items as they run over pair items.
//   * A class is keyed by (set, entry).  Under ProofOfPossession the entry's position is the key.  Under Basic two positions whose
//     affine hash records are equal are the same entry -- the duplicate rule needs "the same message" and a message set keeps no
//     message bytes; equal bytes give equal records, unequal bytes with equal records would be a hash-to-curve collision.  A pair
//     whose index is outside the set (MSGSET_SKIP) is keyed by that value: nothing is read for it.
//   * The rules of the reference are decided on the PAIRS, before anything is merged: the first identity key per set in input
//     order, Basic's duplicate pair from the class table (the table of agg_dup_insert, so agg_dup_find applies as it is), the
//     signature's identity flag.  A class of P and -P sums to the identity with no identity key in it: its factor is 1, no error.
//   * Numbering: the first claimant of a table slot is the class's representative; rank = exclusive prefix sum of "is a
//     representative" over the pairs numbers the classes set after set (pairs are stored set after set), so coffs[b] =
//     rank[offs[b]].  Members per class, their prefix sum moffs and a scatter through one cursor per class give perm: the pair
//     indices in class order (the order inside a class is free: the sum does not depend on it).
//   * The class key sum is the segmented strip sum of multi_batch.cuh with moffs in the place of the key offsets and a gather: strip
//     g sums pts[perm[k]] for k = first, first + stride, ... below end (aggm_strip_of); the strips of a class fold by k_share_fold.
// The per-item functions below are shared by the kernels (tu_agg_msgset.inc) and the host harness (tests/hostsim_agg_msgset).
#pragma once
#include "agg_batch.cuh"
#include "msgset.cuh"

#define AGGM_HASH_WORDS 6         // words of a record that enter the class hash (the low half of x: equality is confirmed on all)

#if defined(__HIPCC__)
#define AGGM_INC(p) atomicAdd(p, 1u)
#else                             // the host harness runs the items one after another
static inline uint32_t AGGM_INC(uint32_t* p) { return (*p)++; }
#endif

// do the entries ka and kb (sanitised: below the set's size, or MSGSET_SKIP) name the same message?  by_record (Basic): equal
// records of `words` 32-bit words are the same message; otherwise the position decides.  recs is read for real entries only.
BLS_FN bool aggm_same_entry(bool by_record, uint32_t ka, uint32_t kb, const uint32_t* recs, size_t words) {
  if (ka == kb) return true;
  if (!by_record || ka == MSGSET_SKIP || kb == MSGSET_SKIP) return false;
  const uint32_t *p = recs + (size_t)ka * words, *q = recs + (size_t)kb * words;
  bool eq = true;
  for (size_t w = 0; w < words; w++) eq = eq && p[w] == q[w];
  return eq;
}
// 64-bit hash of (set, entry): equal classes hash alike (by_record: from the record's words, never from the position)
BLS_FN uint64_t aggm_class_hash(bool by_record, uint32_t set, uint32_t k, const uint32_t* recs, size_t words) {
  uint64_t h = 0x9e3779b97f4a7c15ull ^ ((uint64_t)set * 0xd6e8feb86659fd93ull);
  if (by_record && k != MSGSET_SKIP) {
    const uint32_t* p = recs + (size_t)k * words;
    for (size_t w = 0; w < AGGM_HASH_WORDS && w < words; w++) {
      h = (h ^ p[w]) * 0x100000001b3ull;
      h ^= h >> 29;
    }
  } else {
    h = (h ^ k) * 0x100000001b3ull;
    h ^= h >> 29;
  }
  h *= 0xc4ceb9fe1a85ec53ull;
  return h ^ (h >> 32);
}
// Pair i claims a slot of the class table (tab, minidx: mask + 1 entries preset to AGG_NONE, more entries than pairs), as
// agg_dup_insert does with message bytes: the first claimant of a slot is the representative of its (set, entry) class, a later one
// compares set and entry with it and moves on when they differ; every member lowers the slot's minimum pair index.  Returns the slot.
BLS_FN uint32_t aggm_class_insert(uint32_t i, bool by_record, const uint32_t* cmsg, const uint32_t* sid, const uint32_t* recs, size_t words, uint32_t mask,
                                  uint32_t* tab, uint32_t* minidx) {
  const uint32_t b = sid[i], k = cmsg[i];
  uint32_t s = (uint32_t)aggm_class_hash(by_record, b, k, recs, words) & mask;
  for (;;) {
    uint32_t rep = AGG_CAS(&tab[s], AGG_NONE, i);
    if (rep == AGG_NONE) rep = i;
    if (rep == i || (sid[rep] == b && aggm_same_entry(by_record, k, cmsg[rep], recs, words))) break;
    s = (s + 1) & mask;
  }
  AGG_MIN(&minidx[s], i);
  return s;
}
// ---- numbering, after every insert.  is_rep over the T pairs (entry T of the scanned array is 0, so that rank[T] = C):
BLS_FN uint32_t aggm_is_rep(uint32_t i, const uint32_t* slot_of, const uint32_t* tab) { return tab[slot_of[i]] == i ? 1u : 0u; }
// the class of pair i: its representative's rank
BLS_FN uint32_t aggm_class_of(uint32_t i, const uint32_t* slot_of, const uint32_t* tab, const uint32_t* rank) { return rank[tab[slot_of[i]]]; }
// where set b's classes start in the flat list (b = n_sets: C)
BLS_FN uint64_t aggm_class_offset(const uint64_t* offs, const uint32_t* rank, size_t b) { return rank[offs[b]]; }
// pair i takes the next free place of its class in perm (cursor: one word per class, preset to 0)
BLS_FN void aggm_scatter(uint32_t i, const uint32_t* cid, const uint64_t* moffs, uint32_t* cursor, uint32_t* perm) {
  const uint32_t c = cid[i];
  perm[moffs[c] + AGGM_INC(&cursor[c])] = i;
}
// the members of strip g of the class sum: places first, first + stride, ... below end of perm (multi_strip_of over the classes)
BLS_FN multi_strip aggm_strip_of(uint64_t g, const uint64_t* moffs, const uint64_t* strip_offs, const uint32_t* strip_cid) {
  return multi_strip_of(g, moffs, strip_offs, strip_cid);
}
// ---- precedence.  Below the two rules of this file lies agg_decide (and, over a key set, the key set's two rules, which outrank
// agg_decide: keyset_pre_status).  A set that names a message index outside the message set is BLSGPU_E_ARG with aux (0, 0),
// whatever else holds for it.  Returns whether the rule applied.
BLS_FN bool aggm_top(bool msg_skipped, int32_t* status, uint64_t aux[2]) {
  if (!msg_skipped) return false;
  *status = MSGSET_E_ARG;
  aux[0] = aux[1] = 0;
  return true;
}
// is set b decided before its pairing product counts?  (its class items are then flagged and contribute nothing)
BLS_FN bool aggm_set_decided(uint32_t b, const uint32_t* skipped, const uint32_t* first, const uint32_t* best) {
  return skipped[b] != 0 || first[b] != AGG_NONE || (best && best[b] != AGG_NONE);
}

#if defined(__HIPCC__)
#include "kernels.cuh"
// ---- kernels (tu_agg_msgset1.hip: the group-independent ones and Bls12381G1Impl, tu_agg_msgset2.hip: Bls12381G2Impl).  SG: sig group.
// a. per pair: its set (sid), its sanitised entry (cmsg); skipped[set] = 1 when a pair of the set names no entry (preset 0);
// nolines != nullptr: *walk |= 1 when a named entry has no usable rows (the caller clears the word)
__global__ void k_aggm_check(size_t T, size_t n_sets, const uint64_t* offs, const uint32_t* msg_idx, uint64_t n_msgs, const int32_t* nolines, uint32_t* cmsg,
                             uint32_t* sid, uint32_t* skipped, uint32_t* walk);
// b. per pair: the class table, and the set's first identity key over the keys in input order (first preset to AGG_NONE)
template <int SG>
__global__ void k_aggm_insert(size_t T, int by_record, const uint32_t* cmsg, const uint32_t* sid, const uint32_t* recs, uint32_t mask, uint32_t* tab,
                              uint32_t* minidx, uint32_t* slot_of, const uint8_t* pks, int fmt, const uint64_t* offs, uint32_t* first);
// c. is_rep[i] for i < T, 0 for i == T (T + 1 lanes); then, with rank = its exclusive prefix sum: the class of every pair, the
// class's set / entry / representative, its member count (preset 0); the class offsets per set as 64-bit words (n_sets + 1 lanes)
__global__ void k_aggm_reps(size_t T, const uint32_t* slot_of, const uint32_t* tab, uint32_t* is_rep);
__global__ void k_aggm_number(size_t T, const uint32_t* slot_of, const uint32_t* tab, const uint32_t* rank, const uint32_t* sid, const uint32_t* cmsg,
                              uint32_t* cid, uint32_t* csid, uint32_t* cent, uint32_t* crep, uint32_t* count);
__global__ void k_aggm_offsets(size_t n_sets, const uint64_t* offs, const uint32_t* rank, uint64_t* coffs);
__global__ void k_aggm_widen(size_t n, const uint32_t* in, uint64_t* out);
__global__ void k_aggm_scatter(size_t T, const uint32_t* cid, const uint64_t* moffs, uint32_t* cursor, uint32_t* perm);
// d. the strip sum with a gather, KG: the keys' group (1: one lane per strip, 2: one lane pair per strip)
template <int KG>
__global__ void k_aggm_sum(size_t n_strips, const uint8_t* pts, int fmt, const uint32_t* perm, const uint64_t* moffs, const uint64_t* strip_offs,
                           const uint32_t* strip_cid, uint8_t* part);
template <>
__global__ void k_aggm_sum<1>(size_t, const uint8_t*, int, const uint32_t*, const uint64_t*, const uint64_t*, const uint32_t*, uint8_t*);
template <>
__global__ void k_aggm_sum<2>(size_t, const uint8_t*, int, const uint32_t*, const uint64_t*, const uint64_t*, const uint32_t*, uint8_t*);
// e. one lane per item of the flat list (stride M = C + n_sets): class item c < C is (summed key, H(m)) in k_prepare_agg_seg's
// pair layout -- the key from part[strip_offs[c]] (RAW_PROJ), or part == nullptr: pks[crep[c]] in fmt (every class a singleton) --
// flagged when the sum or the entry is the identity or the set is decided; item C + b is set b's signature item, and sig_id[b]
// says whether the signature is the identity
template <int SG>
__global__ void k_aggm_items(size_t M, size_t C, const uint32_t* csid, const uint32_t* cent, const uint32_t* crep, const uint32_t* skipped,
                             const uint32_t* first, const uint32_t* best, const uint8_t* pks, int fmt, const uint8_t* part, const uint64_t* strip_offs,
                             const uint8_t* recs, const uint8_t* sigs, uint32_t* pairs, int32_t* bad, uint32_t* sig_id);
// f. one lane per set: a skipped set is marked decided before the final exponentiation (after k_agg_batch_mark); after
// k_agg_batch_fin and the key set's precedence, aggm_top on the caller's status / aux (aux may be null)
__global__ void k_aggm_mark(size_t n_sets, const uint32_t* skipped, int32_t* st_b);
__global__ void k_aggm_fin(size_t n_sets, const uint32_t* skipped, int32_t* status, uint64_t* aux);
#endif
