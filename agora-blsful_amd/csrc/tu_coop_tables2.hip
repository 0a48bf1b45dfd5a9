// translation unit: k_pairing_coop_tables2, the one-wave pairing of TWO tabled pairs whose rows both lie in global memory
// (blsgpu_signcrypt_share_verify_indexed_batch, Bls12381G2Impl: both G2 members belong to the ciphertext; signcrypt.cuh).
// A unit of its own: the kernels of tu_coop.hip, tu_coop_keyed.hip and tu_coop_rows.hip stay what they are.
#include "kernels.cuh"
#include "coop.cuh"
#include "signcrypt.cuh"

// coop_miller2_tables with the second table in global memory too: the loop reads `rows1` only as a plain row pointer (lane pair 31),
// so the constant-table form serves both and stays, text and code, what it is.
__device__ __forceinline__ void coop_miller2_tables2(coop_shared& S, const g1_aff* P, const uint32_t* rows0, const uint32_t* rows1) {
  coop_miller2_tables(S, P, rows0, reinterpret_cast<const uint32_t (*)[4 * FP_NL]>(rows1));
}

// Pair k is (P_k, entry tk[i] of `table`): the record's Q members are not read.  The table's base is wave-uniform and an entry's rows
// start at the 32-bit WORD offset tk[i] 68 4 FP_NL, as in k_pairing_coop_keyed (the host keeps the table below 2^32 bytes).  An item
// whose status is not OK on entry reads no row.
__global__ void __launch_bounds__(BLS_BLOCK, 2) k_pairing_coop_tables2(size_t n, const uint32_t* pairs, int32_t* status, const uint32_t* table,
                                                                       const uint32_t* t0, const uint32_t* t1, uint32_t* easy) {
  __shared__ coop_shared S;
  const size_t i = blockIdx.x;
  if (i >= n) return;
  if (status[i] != BLS_OK) return;                     // before any table read
  g1_aff P[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int w0 = k * 3 * W2;
    ws_ld_fp(P[k].x, pairs, n, i, w0);
    ws_ld_fp(P[k].y, pairs, n, i, w0 + W1);
    P[k].inf = false;
  }
  const uint32_t off0 = t0[i] * (uint32_t)(MILLER_ENTRIES * 4 * FP_NL), off1 = t1[i] * (uint32_t)(MILLER_ENTRIES * 4 * FP_NL);
  coop_miller2_tables2(S, P, table + off0, table + off1);
  if (!easy) {
    int st = coop_final_verdict(S);
    if (threadIdx.x == 0) status[i] = st;
    return;
  }
  coop_final_easy(S);
  uint32_t* e = easy + i * WIDE_EASY_WORDS;
  for (int t = threadIdx.x; t < WIDE_EASY_WORDS; t += BLS_BLOCK) {
    const int v = t >> 4, l = t & 15;                  // value v = 2 k + component
    e[t] = l < FP_NL ? S.f.c[v >> 1][(v & 1) * FP_NL + l] : 0u;
  }
}
