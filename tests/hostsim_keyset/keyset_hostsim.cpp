// TEST-ONLY harness for tests/test_hostsim_keyset.py: compiles the recoding header of the registered key sets
// (agora-blsful_amd/csrc/keyset.cuh: keyset_shape, keyset_digit, keyset_record, keyset_pre_key / keyset_pre_status) and the scalar
// decomposition it recodes (msm2.cuh) as plain host C++, so that the `-m "not gpu"` suite checks them without a GPU.  Built twice:
// as a shared object driven from Python, and -- with KEYSET_HOSTSIM_MAIN -- as a stand-alone program under the address and
// undefined-behaviour sanitizers that walks the same functions over its own edge values.  Never linked into libblsgpu.so.
#include <stdio.h>
#include <string.h>
#include "../../agora-blsful_amd/csrc/keyset.cuh"

template <int G>
static int recode(const uint64_t* a, int32_t* digits, uint32_t* records) {
  typedef keyset_shape<G> S;
  uint32_t carry = 0;
  for (int j = 0; j < S::WINDOWS; j++) {
    const int d = keyset_digit(a, S::WORDS, j, carry);
    digits[j] = d;
    records[j] = d ? keyset_record(j, d < 0 ? -d : d) : 0xffffffffu;
  }
  return (int)carry;
}

extern "C" {
// out: E, WORDS, FULL, WINDOWS, POINTS, W, ROW
void hs_keyset_shape(int G, int* out) {
  const int s1[5] = {keyset_shape<1>::E, keyset_shape<1>::WORDS, keyset_shape<1>::FULL, keyset_shape<1>::WINDOWS, keyset_shape<1>::POINTS};
  const int s2[5] = {keyset_shape<2>::E, keyset_shape<2>::WORDS, keyset_shape<2>::FULL, keyset_shape<2>::WINDOWS, keyset_shape<2>::POINTS};
  memcpy(out, G == 1 ? s1 : s2, sizeof s1);
  out[5] = KEYSET_W;
  out[6] = KEYSET_ROW;
}
// the digits of one sub-scalar (WORDS 64-bit words) and the table record of each non-zero one; returns the carry left after the
// last window (must be 0)
int hs_keyset_recode(int G, const uint64_t* a, int32_t* digits, uint32_t* records) {
  return G == 1 ? recode<1>(a, digits, records) : recode<2>(a, digits, records);
}
// the E sub-scalars of a 256-bit scalar (8 little-endian 32-bit words), as the table ladder gets them
void hs_keyset_decompose(int G, const uint32_t* k, uint64_t* a) {
  if (G == 1) msm2_decompose_g1(a, k);
  else msm2_decompose_g2(a, k);
}
uint64_t hs_keyset_pre_key(int oob, uint64_t pos, int32_t st) { return keyset_pre_key(oob != 0, pos, st); }
int32_t hs_keyset_pre_status(uint64_t key) { return keyset_pre_status(key); }
}

#ifdef KEYSET_HOSTSIM_MAIN
// sum d_j 16^j from the top window down, in 192-bit two's complement; must give the sub-scalar back
template <int G>
static bool check(const uint64_t* a) {
  typedef keyset_shape<G> S;
  int32_t d[S::WINDOWS];
  uint32_t rec[S::WINDOWS];
  if (recode<G>(a, d, rec) != 0) return false;
  uint64_t acc[3] = {0, 0, 0};
  for (int j = S::WINDOWS - 1; j >= 0; j--) {
    if (d[j] < -(KEYSET_ROW - 1) || d[j] > KEYSET_ROW) return false;
    if (j == S::FULL && d[j] != 0 && d[j] != 1) return false;
    if (d[j] && rec[j] >= (uint32_t)S::POINTS) return false;
    acc[2] = (acc[2] << 4) | (acc[1] >> 60);
    acc[1] = (acc[1] << 4) | (acc[0] >> 60);
    acc[0] <<= 4;
    const uint64_t add[3] = {(uint64_t)(int64_t)d[j], d[j] < 0 ? ~0ull : 0ull, d[j] < 0 ? ~0ull : 0ull};
    unsigned __int128 c = 0;
    for (int k = 0; k < 3; k++) {
      c += (unsigned __int128)acc[k] + add[k];
      acc[k] = (uint64_t)c;
      c >>= 64;
    }
  }
  return acc[0] == a[0] && acc[1] == (S::WORDS == 2 ? a[1] : 0) && acc[2] == 0;
}
int main() {
  const uint64_t edge[] = {0, 1, 15, 8, 7, 9, ~0ull, 0x9999999999999999ull, 0x8888888888888888ull, 0x8f8f8f8f8f8f8f8full, 0xf000000000000000ull,
                           BLS_X_ABS - 1, BLS_X_ABS, 0x7777777777777777ull, 0x8000000000000000ull};
  const int ne = (int)(sizeof edge / sizeof edge[0]);
  long bad = 0, seen = 0;
  for (int i = 0; i < ne; i++) {
    bad += !check<2>(&edge[i]);
    for (int j = 0; j < ne; j++) {
      const uint64_t a[2] = {edge[i], edge[j]};
      bad += !check<1>(a);
      seen++;
    }
  }
  uint64_t x = 0x243f6a8885a308d3ull;             // xorshift: the same values on every run
  for (int t = 0; t < 2000; t++) {
    uint32_t k[8];
    for (int w = 0; w < 8; w++) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      k[w] = (uint32_t)(x >> 16);
    }
    uint64_t a[4];
    msm2_decompose_g1(a, k);
    bad += !check<1>(a) + !check<1>(a + 2);
    msm2_decompose_g2(a, k);
    for (int e = 0; e < 4; e++) bad += !check<2>(a + e);
    seen += 6;
  }
  bad += keyset_pre_status(keyset_pre_key(true, 5, 7)) != KEYSET_E_ARG;
  bad += keyset_pre_status(keyset_pre_key(false, 0xfffffffeull, 8)) != 8;
  bad += keyset_pre_key(false, 3, 0) != KEYSET_PRE_NONE;
  printf("keyset_hostsim: %ld values, %ld bad\n", seen, bad);
  return bad ? 1 : 0;
}
#endif
