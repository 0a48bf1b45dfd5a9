// TEST-ONLY harness for tests/test_hostsim_keyset_update.py: compiles the position rule of blsgpu_keyset_update and
// blsgpu_keyset_append (agora-blsful_amd/csrc/keyset.cuh: keyset_positions_check) as plain host C++.  Built twice: as a shared
// object driven from Python, and -- with KEYSET_UPDATE_HOSTSIM_MAIN -- as a stand-alone program under the address and
// undefined-behaviour sanitizers that walks the same function over its own inputs.  Never linked into libblsgpu.so.
#include <stdio.h>
#include <vector>
#include "../../agora-blsful_amd/csrc/keyset.cuh"

extern "C" {
// an update's list of `count` positions over a set of n_keys entries: KEYSET_POS_OK, _RANGE or _DUP
int hs_update_rule(const uint32_t* pos, uint64_t count, uint64_t n_keys) {
  static const uint32_t none = 0;
  return keyset_positions_check(count ? pos : &none, count, n_keys);
}
// an append of `count` entries to a set of n_keys: KEYSET_POS_OK or _FULL
int hs_append_rule(uint64_t n_keys, uint64_t count) { return keyset_positions_check(nullptr, count, n_keys); }
}

#ifdef KEYSET_UPDATE_HOSTSIM_MAIN
static long bad = 0, seen = 0;
static void expect(const std::vector<uint32_t>& pos, uint64_t n_keys, int want) {
  bad += hs_update_rule(pos.data(), pos.size(), n_keys) != want;
  seen++;
}
int main() {
  const uint64_t n = 320;
  expect({}, n, KEYSET_POS_OK);
  expect({}, 0, KEYSET_POS_OK);
  expect({0}, n, KEYSET_POS_OK);
  expect({0}, 0, KEYSET_POS_RANGE);
  expect({319}, n, KEYSET_POS_OK);
  expect({320}, n, KEYSET_POS_RANGE);
  expect({0xffffffffu}, n, KEYSET_POS_RANGE);
  expect({1, 2, 3, 63, 64, 65}, n, KEYSET_POS_OK);
  expect({65, 0, 319, 64, 5, 63}, n, KEYSET_POS_OK);
  expect({9, 8, 7, 6, 5, 4, 3, 2, 1, 0}, n, KEYSET_POS_OK);
  expect({4, 4}, n, KEYSET_POS_DUP);
  expect({1, 7, 7, 9}, n, KEYSET_POS_DUP);
  expect({7, 1, 2, 3, 7}, n, KEYSET_POS_DUP);
  expect({7, 1, 2, 3, 7, 320}, n, KEYSET_POS_RANGE);       // range is decided before duplicates
  {
    std::vector<uint32_t> all(4100);                      // a whole table reversed, then with one position repeated at the far end
    for (size_t i = 0; i < all.size(); i++) all[i] = (uint32_t)(all.size() - 1 - i);
    expect(all, 4100, KEYSET_POS_OK);
    expect(all, 4099, KEYSET_POS_RANGE);
    all.back() = all.front();
    expect(all, 4100, KEYSET_POS_DUP);
  }
  const uint64_t top = 0xfffffffeull;                     // 2^32 - 2: the most entries a set may have
  bad += hs_append_rule(0, 0) != KEYSET_POS_OK;
  bad += hs_append_rule(0, top) != KEYSET_POS_OK;
  bad += hs_append_rule(0, top + 1) != KEYSET_POS_FULL;
  bad += hs_append_rule(320, top - 320) != KEYSET_POS_OK;
  bad += hs_append_rule(320, top - 319) != KEYSET_POS_FULL;
  bad += hs_append_rule(top, 0) != KEYSET_POS_OK;
  bad += hs_append_rule(top, 1) != KEYSET_POS_FULL;
  bad += hs_append_rule(320, ~0ull) != KEYSET_POS_FULL;   // no wrap-around
  seen += 8;
  printf("keyset_update_hostsim: %ld checks, %ld bad\n", seen, bad);
  return bad ? 1 : 0;
}
#endif
