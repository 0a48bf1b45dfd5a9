// translation unit: k_pairing_coop_rows, the one-wave pairing that reads a registered message's line rows (msgset.cuh, coop_rows.cuh).
// A unit of its own: the kernels of tu_coop.hip and tu_coop_keyed.hip stay what they are.
#include "kernels.cuh"
#include "coop_rows.cuh"
#include "msgset.cuh"

__global__ void __launch_bounds__(BLS_BLOCK, 2) k_pairing_coop_rows(size_t n, const uint32_t* pairs, int32_t* status, const uint32_t* table,
                                                                    const uint32_t* msg_of, uint32_t* easy) {
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
  aff<hfp2> Q1;                                        // pair 1's G2 member, the walked one; pair 0's is the entry's rows
  ws_ld_fp(Q1.x.v, pairs, n, i, 3 * W2 + W2 + (lane_hi() ? W1 : 0));
  ws_ld_fp(Q1.y.v, pairs, n, i, 3 * W2 + 2 * W2 + (lane_hi() ? W1 : 0));
  Q1.inf = false;
  const uint32_t moff = msg_of[i] * (uint32_t)(MILLER_ENTRIES * 4 * FP_NL);
  coop_miller2_rows(S, P, Q1, table + moff);
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
