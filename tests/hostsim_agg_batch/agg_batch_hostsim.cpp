// TEST-ONLY harness for tests/test_hostsim_agg_batch.py: compiles the per-item functions of the batched aggregate verify
// (agora-blsful_amd/csrc/agg_batch.cuh) as plain host C++, so that the `-m "not gpu"` suite checks the segmented duplicate rule,
// the segmented first-identity reduction, the index arithmetic of the segmented product and the precedence without a GPU.  The
// "kernels" here run the items of a launch one after another, in the order the caller gives.  Never linked into libblsgpu.so.
#include <string.h>
#include <vector>
#include "../../agora-blsful_amd/csrc/agg_batch.cuh"

extern "C" {
// k_dup_insert_seg + k_dup_find_seg over T_b pair items visited in `order`; cap: table entries (a power of two above T_b).
// out: per set (old, i) local indices, or (AGG_NONE, AGG_NONE).
void hs_agg_dup(uint32_t T_b, uint32_t n_b, const uint8_t* msgs, const uint64_t* moffs, const uint32_t* sid, const uint32_t* src, const uint64_t* boffs,
                uint32_t cap, const uint32_t* order, uint32_t* out) {
  std::vector<uint32_t> tab(cap, AGG_NONE), minidx(cap, AGG_NONE), slot_of(T_b ? T_b : 1), best(n_b, AGG_NONE);
  for (uint32_t k = 0; k < T_b; k++) slot_of[order[k]] = agg_dup_insert(order[k], msgs, moffs, sid, src, cap - 1, tab.data(), minidx.data());
  for (uint32_t k = 0; k < T_b; k++) agg_dup_find(order[k], sid, boffs, slot_of.data(), minidx.data(), best.data());
  for (uint32_t b = 0; b < n_b; b++) {
    out[2 * b] = best[b] == AGG_NONE ? AGG_NONE : minidx[slot_of[boffs[b] + best[b]]] - (uint32_t)boffs[b];
    out[2 * b + 1] = best[b];
  }
}
uint64_t hs_agg_hash(uint32_t set, const uint8_t* p, size_t len) { return agg_msg_hash(set, p, len); }
// k_first_bad_seg over the M = T_b + n_b items
void hs_agg_first_bad(uint32_t T_b, uint32_t n_b, const uint32_t* sid, const uint64_t* boffs, const int32_t* bad, const uint32_t* order, uint32_t* first,
                      uint32_t* sig_id) {
  for (uint32_t b = 0; b < n_b; b++) first[b] = AGG_NONE;
  for (uint32_t k = 0; k < T_b + n_b; k++) agg_first_bad_item(order[k], T_b, sid, boffs, bad, first, sig_id);
}
// the rounds of k_f12_fold_seg and k_f12_fold_seg_out on integers mod 2^61 - 1 standing in for the Fp12 values: f holds the M item
// values, rec gets one product per set.  Every round reads a snapshot of f, as lanes that run side by side would; returns the
// number of rounds, or -1 when some round reads an item that the same round writes.
static uint64_t mulm(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % 2305843009213693951ull); }
int hs_agg_fold(uint32_t T_b, uint32_t n_b, const uint32_t* sid, const uint64_t* boffs, uint64_t tmax, uint64_t* f, uint64_t* rec, uint64_t* products) {
  const int nr = agg_fold_rounds(tmax);
  *products = 0;
  for (int r = 0; r < nr; r++) {
    std::vector<uint64_t> snap(f, f + T_b);
    std::vector<char> written(T_b, 0), read(T_b, 0);
    for (uint32_t i = 0; i < T_b; i++) {
      const uint64_t lo = boffs[sid[i]], len = boffs[sid[i] + 1] - lo;
      uint64_t partner;
      if (!agg_fold_partner(len, r, i - lo, &partner)) continue;
      if (partner >= len) return -2;
      f[i] = mulm(snap[i], snap[lo + partner]);
      written[i] = 1;
      read[lo + partner] = 1;
      ++*products;
    }
    for (uint32_t i = 0; i < T_b; i++)
      if (written[i] && read[i]) return -1;
  }
  for (uint32_t b = 0; b < n_b; b++) rec[b] = boffs[b + 1] != boffs[b] ? mulm(f[boffs[b]], f[T_b + b]) : f[T_b + b];
  return nr;
}
int32_t hs_agg_decide(uint32_t dup_old, uint32_t dup_i, int sig_is_id, uint32_t first_bad, uint64_t* aux) {
  return agg_decide(dup_old, dup_i, sig_is_id != 0, first_bad, aux);
}
}
