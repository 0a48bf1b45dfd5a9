// TEST-ONLY harness for tests/test_hostsim_multi_batch.py: compiles the strip plan of the batched multi verify and the index
// arithmetic of its accumulate and fold kernels (agora-blsful_amd/csrc/multi_batch.cuh, shares.cuh share_fold_adds) as plain host
// C++, so that the `-m "not gpu"` suite checks them without a GPU.  Points are integers mod 2^61 - 1, the "kernels" run their
// lanes one after another, and every fold level reads a snapshot, as lanes that run side by side would.  Never linked into
// libblsgpu.so.
#include <string.h>
#include <vector>
#include "../../agora-blsful_amd/csrc/multi_batch.cuh"

static const uint64_t PRIME = 2305843009213693951ull;
static uint64_t addm(uint64_t a, uint64_t b) { return (a + b) % PRIME; }

extern "C" {
uint64_t hs_multi_strip_len(uint64_t N, uint64_t lanes, uint64_t forced) { return multi_strip_len(N, lanes, forced); }

// plan, k_multi_accumulate_seg, the levels of k_share_fold over the strips, k_set_out's pick.
//   in : key_offs (n_sets + 1), L, vals (one per key)
//   out: strip_offs (n_sets + 1), strip_sid (cap entries), reads (per key: how many strips read it), sums (per set:
//        part[strip_offs[s]], untouched for an empty set), n_strips, qmax
// returns the number of fold levels, or: -1 a level reads a record it also writes, -2 more strips than cap, -3 a fold step
// reaches into another set's strips, -4 a strip reads a key outside its set
int hs_multi_run(const uint64_t* key_offs, uint32_t n_sets, uint64_t L, const uint64_t* vals, uint64_t* strip_offs, uint32_t* strip_sid,
                 uint64_t cap, uint32_t* reads, uint64_t* sums, uint64_t* n_strips, uint64_t* qmax) {
  std::vector<uint64_t> soffs;
  std::vector<uint32_t> ssid;
  *qmax = multi_strip_plan(key_offs, n_sets, L, soffs, ssid);
  const uint64_t Q = ssid.size();
  *n_strips = Q;
  if (Q > cap) return -2;
  memcpy(strip_offs, soffs.data(), 8 * (n_sets + 1));
  if (Q) memcpy(strip_sid, ssid.data(), 4 * Q);
  std::vector<uint64_t> part(Q, 0);
  for (uint64_t g = 0; g < Q; g++) {
    const multi_strip st = multi_strip_of(g, key_offs, soffs.data(), ssid.data());
    for (uint64_t i = st.first; i < st.end; i += st.stride) {
      if (i < key_offs[ssid[g]] || i >= key_offs[ssid[g] + 1]) return -4;
      reads[i]++;
      part[g] = addm(part[g], vals[i]);
    }
  }
  int levels = 0;
  for (uint64_t step = 1; step < *qmax; step <<= 1, levels++) {
    const std::vector<uint64_t> snap(part);
    std::vector<char> written(Q, 0), read(Q, 0);
    for (uint64_t i = 0; i < Q; i++) {
      const uint32_t s = ssid[i];
      if (!share_fold_adds(i, step, soffs[s], soffs[s + 1])) continue;
      if (i + step >= Q || ssid[i + step] != s) return -3;
      part[i] = addm(snap[i], snap[i + step]);
      written[i] = 1;
      read[i + step] = 1;
    }
    for (uint64_t i = 0; i < Q; i++)
      if (written[i] && read[i]) return -1;
  }
  for (uint32_t s = 0; s < n_sets; s++)
    if (key_offs[s + 1] != key_offs[s]) sums[s] = part[soffs[s]];
  return levels;
}
}
