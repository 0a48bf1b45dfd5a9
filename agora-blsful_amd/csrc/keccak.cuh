// Keccak-f[1600] and the SHAKE128 sponge (FIPS 202) as plain functions, one state per lane: twenty-five 64-bit words that stay in
// registers -- every loop below has a constant trip count and is unrolled, so every state index, rotation count and round constant
// is a compile-time value and nothing is addressed through scratch.  Rotations are 64-bit funnel shifts.
// Compiles as plain C++ too (tests/hostsim_signcrypt).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KECCAK_FN __host__ __device__ __forceinline__
#else
#define KECCAK_FN static inline
#endif

#define SHAKE128_RATE 168            // bytes per block
#define SHAKE128_RATE_WORDS 21

struct keccak_state {
  uint64_t s[25];
};

KECCAK_FN uint64_t keccak_rol(uint64_t x, int n) { return n ? (x << n) | (x >> (64 - n)) : x; }

KECCAK_FN void keccak_f1600(keccak_state& st) {
  constexpr uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
                               0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
                               0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
                               0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
                               0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  // rotation of lane (x, y), index x + 5 y
  constexpr int ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
  uint64_t* a = st.s;
#pragma unroll
  for (int round = 0; round < 24; round++) {
    uint64_t c[5], b[25];
#pragma unroll
    for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
    for (int x = 0; x < 5; x++) {
      const uint64_t d = c[(x + 4) % 5] ^ keccak_rol(c[(x + 1) % 5], 1);
#pragma unroll
      for (int y = 0; y < 5; y++) a[x + 5 * y] ^= d;
    }
    // rho and pi: B[y, 2x + 3y] = rol(A[x, y])
#pragma unroll
    for (int x = 0; x < 5; x++)
#pragma unroll
      for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = keccak_rol(a[x + 5 * y], ROT[x + 5 * y]);
    // chi
#pragma unroll
    for (int y = 0; y < 5; y++)
#pragma unroll
      for (int x = 0; x < 5; x++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
    a[0] ^= RC[round];
  }
}

// SHAKE128 of a message shorter than one block (the compressed points this library feeds it are 48 or 96 bytes): the state after
// the single absorbing permutation, i.e. with the first SHAKE128_RATE output bytes in words 0 .. 20 (little-endian).  Every
// further block of output is one more keccak_f1600.  len must be a multiple of 8 below SHAKE128_RATE.
template <int LEN>
KECCAK_FN void shake128_absorb_short(keccak_state& st, const uint8_t* msg) {
  static_assert(LEN % 8 == 0 && LEN < SHAKE128_RATE, "one block, whole words");
#pragma unroll
  for (int k = 0; k < 25; k++) st.s[k] = 0;
#pragma unroll
  for (int k = 0; k < LEN / 8; k++) {
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) w |= (uint64_t)msg[8 * k + j] << (8 * j);
    st.s[k] = w;
  }
  st.s[LEN / 8] ^= 0x1full;                                // domain separation of the SHAKE functions and the first padding bit
  st.s[SHAKE128_RATE_WORDS - 1] ^= 0x8000000000000000ull;  // the last padding bit, in the last byte of the block
  keccak_f1600(st);
}
