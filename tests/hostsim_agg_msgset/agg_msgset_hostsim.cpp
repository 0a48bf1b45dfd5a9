// TEST-ONLY harness for tests/test_hostsim_agg_msgset.py: compiles the per-item functions of the aggregate verify by message index
// (agora-blsful_amd/csrc/agg_msgset.cuh) as plain host C++, so that the `-m "not gpu"` suite checks the class table, the class
// numbering, the member permutation, the strips' member ranges, the duplicate pair and the precedence without a GPU.  The "kernels"
// here run the items of a launch one after another, in the order the caller gives.  Never linked into libblsgpu.so.
#include <string.h>
#include <vector>
#include "../../agora-blsful_amd/csrc/agg_msgset.cuh"

extern "C" {
// k_aggm_insert (the class table), k_dup_find_seg, k_aggm_reps, the prefix sum, k_aggm_number, k_aggm_offsets, the prefix sum of the
// member counts and k_aggm_scatter over T pairs visited in `order`.  cap: table entries (a power of two above T).  Outputs: cid[T],
// coffs[n_sets + 1], csid / cent / crep / moffs (T + 1 entries each, the first C (+ 1) used), perm[T], dup[2 n_sets] (old, i) local or
// AGG_NONE.  Returns C.
uint32_t hs_aggm_classes(uint32_t T, uint32_t n_sets, int by_record, const uint32_t* cmsg, const uint32_t* sid, const uint64_t* offs, const uint32_t* recs,
                         uint32_t words, uint32_t cap, const uint32_t* order, uint32_t* cid, uint64_t* coffs, uint32_t* csid, uint32_t* cent, uint32_t* crep,
                         uint64_t* moffs, uint32_t* perm, uint32_t* dup) {
  std::vector<uint32_t> tab(cap, AGG_NONE), minidx(cap, AGG_NONE), slot_of(T + 1), is_rep(T + 1, 0), rank(T + 1, 0), count(T + 1, 0), cursor(T + 1, 0),
      best(n_sets, AGG_NONE);
  for (uint32_t k = 0; k < T; k++) slot_of[order[k]] = aggm_class_insert(order[k], by_record != 0, cmsg, sid, recs, words, cap - 1, tab.data(), minidx.data());
  for (uint32_t k = 0; k < T; k++) agg_dup_find(order[k], sid, offs, slot_of.data(), minidx.data(), best.data());
  for (uint32_t i = 0; i < T; i++) is_rep[i] = aggm_is_rep(i, slot_of.data(), tab.data());
  for (uint32_t i = 0; i < T; i++) rank[i + 1] = rank[i] + is_rep[i];
  const uint32_t C = rank[T];
  for (uint32_t k = 0; k < T; k++) {
    const uint32_t i = order[k], c = aggm_class_of(i, slot_of.data(), tab.data(), rank.data());
    cid[i] = c;
    count[c]++;
    if (aggm_is_rep(i, slot_of.data(), tab.data())) {
      csid[c] = sid[i];
      cent[c] = cmsg[i];
      crep[c] = i;
    }
  }
  for (uint32_t b = 0; b <= n_sets; b++) coffs[b] = aggm_class_offset(offs, rank.data(), b);
  moffs[0] = 0;
  for (uint32_t c = 0; c < C; c++) moffs[c + 1] = moffs[c] + count[c];
  for (uint32_t k = 0; k < T; k++) aggm_scatter(order[k], cid, moffs, cursor.data(), perm);
  for (uint32_t b = 0; b < n_sets; b++) {
    dup[2 * b] = best[b] == AGG_NONE ? AGG_NONE : minidx[slot_of[offs[b] + best[b]]] - (uint32_t)offs[b];
    dup[2 * b + 1] = best[b];
  }
  return C;
}
// the strips of the class sum over C classes with member offsets moffs and strip length L: visits[k]++ for every place k of perm a
// strip reaches, strip_class[g] = the class strip g sums into; returns the number of strips, or -1 when a strip leaves its class
int64_t hs_aggm_strips(uint32_t C, const uint64_t* moffs, uint64_t L, uint32_t* visits, uint32_t* strip_class) {
  std::vector<uint64_t> soffs;
  std::vector<uint32_t> ssid;
  multi_strip_plan(moffs, C, L, soffs, ssid);
  for (size_t g = 0; g < ssid.size(); g++) {
    const multi_strip st = aggm_strip_of(g, moffs, soffs.data(), ssid.data());
    strip_class[g] = ssid[g];
    for (uint64_t k = st.first; k < st.end; k += st.stride) {
      if (k < moffs[ssid[g]] || k >= moffs[ssid[g] + 1]) return -1;
      visits[k]++;
    }
  }
  return (int64_t)ssid.size();
}
// the precedence of one set as the call applies it: agg_decide on the pairs' rules (BLS_OK: the product's verdict stands), the key
// set's rules over it (key_pre: keyset_pre_key's word, KEYSET_PRE_NONE without a key set), aggm_top over both
int32_t hs_aggm_decide(int msg_skipped, uint64_t key_pre, uint32_t dup_old, uint32_t dup_i, int sig_is_id, uint32_t first_bad, int32_t product, uint64_t* aux) {
  int32_t st = agg_decide(dup_old, dup_i, sig_is_id != 0, first_bad, aux);
  if (st == BLS_OK) st = product;
  if (key_pre != KEYSET_PRE_NONE) {
    st = keyset_pre_status(key_pre);
    aux[0] = aux[1] = 0;
  }
  aggm_top(msg_skipped != 0, &st, aux);
  return st;
}
uint64_t hs_keyset_pre_key(int out_of_range, uint64_t pos_in_set, int32_t entry_status) { return keyset_pre_key(out_of_range != 0, pos_in_set, entry_status); }
uint32_t hs_msgset_entry_of(uint32_t msg_idx, uint64_t n_msgs) { return msgset_entry_of(msg_idx, n_msgs); }
int hs_aggm_set_decided(uint32_t skipped, uint32_t first, uint32_t best, int has_best) { return aggm_set_decided(0, &skipped, &first, has_best ? &best : nullptr); }
}
