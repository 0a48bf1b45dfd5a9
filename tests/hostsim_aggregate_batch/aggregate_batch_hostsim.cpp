// TEST-ONLY harness for tests/test_hostsim_aggregate_batch.py: compiles the first-occurrence search of the batched secure aggregation
// (agora-blsful_amd/csrc/secure.cuh secure_first_tile, the per-lane body of k_secure_first) as plain host C++, so that the
// `-m "not gpu"` suite checks it without a GPU.  The "kernel" below walks the tiles exactly as k_secure_first does -- workgroups of
// BLOCK consecutive keys, the range [min lo, max i) of their live lanes, tile k to slice y = k mod S, the slices meeting by a
// minimum -- and runs its lanes one after another.  Never linked into libblsgpu.so.
#include <string.h>
#include <vector>
#include "../../agora-blsful_amd/csrc/secure.cuh"

static const size_t BLOCK = 64;

template <int WPK>
static int run_first(const uint8_t* kb, const uint64_t* offs, uint32_t n_sets, const uint8_t* large, size_t S, uint32_t* first) {
  const size_t n = (size_t)offs[n_sets];
  const uint32_t* kw = (const uint32_t*)kb;
  std::vector<uint32_t> sid(n);
  for (uint32_t s = 0; s < n_sets; s++)
    for (uint64_t i = offs[s]; i < offs[s + 1]; i++) sid[i] = s;
  for (size_t i = 0; i < n; i++) first[i] = ~0u;
  for (size_t b0 = 0; b0 < n; b0 += BLOCK) {
    uint64_t rlo = ~0ull, rhi = 0;
    for (size_t i = b0; i < b0 + BLOCK && i < n; i++)
      if (!large[sid[i]]) {
        if (offs[sid[i]] < rlo) rlo = offs[sid[i]];
        if (i > rhi) rhi = i;
      }
    for (size_t y = 0; y < S; y++) {
      std::vector<uint32_t> best(BLOCK);
      for (size_t l = 0; l < BLOCK; l++) best[l] = (uint32_t)(b0 + l);
      for (size_t t0 = (size_t)rlo + y * BLOCK; t0 < rhi; t0 += S * BLOCK) {
        uint32_t tile[BLOCK * WPK];
        memset(tile, 0xa5, sizeof tile);                       // what the kernel never loads must never decide a comparison
        const size_t tile_keys = rhi - t0 < BLOCK ? (size_t)(rhi - t0) : BLOCK;
        if (t0 + tile_keys > n) return -1;                     // a load past the end of the keys
        memcpy(tile, kw + t0 * WPK, tile_keys * WPK * 4);
        for (size_t l = 0; l < BLOCK; l++) {
          const size_t i = b0 + l;
          if (i >= n || large[sid[i]]) continue;
          best[l] = secure_first_tile<WPK>(best[l], tile, t0, tile_keys, (size_t)offs[sid[i]], kw + i * WPK);
        }
      }
      for (size_t l = 0; l < BLOCK; l++) {
        const size_t i = b0 + l;
        if (i < n && !large[sid[i]] && best[l] < first[i]) first[i] = best[l];
      }
    }
  }
  return 0;
}

extern "C" {
// kb: n keys of 4 wpk bytes (wpk = 12 or 24); offs: n_sets + 1; large: one byte per set (non-zero: the kernel skips the set);
// S: gridDim.y; first: n entries out (~0 for the keys of a skipped set).  Returns 0, or -1 for an out-of-range tile load, -2 for wpk.
int hs_secure_first(const uint8_t* kb, uint32_t wpk, const uint64_t* offs, uint32_t n_sets, const uint8_t* large, uint32_t S, uint32_t* first) {
  if (wpk == 12) return run_first<12>(kb, offs, n_sets, large, S, first);
  if (wpk == 24) return run_first<24>(kb, offs, n_sets, large, S, first);
  return -2;
}
}
