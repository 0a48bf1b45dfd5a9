// translation unit: k_lines2s_tables2, the lane-split line kernel of TWO tabled pairs whose rows both lie in global memory
// (blsgpu_signcrypt_share_verify_indexed_batch, Bls12381G2Impl; signcrypt.cuh).  A unit of its own: the kernels of tu_lines.hip stay
// what they are.
#define BLS_TU_LINES_TABLES2 1
#include "kernels.cuh"
#include "signcrypt.cuh"

// As k_lines2s_keyed (kernels.cuh), with the constant's row replaced by a second per-lane row: pair k is (P_k, entry tk[i] of `table`),
// its normalised rows at table + (tk[i] 68 + e) 4 FP_NL.  Nothing is doubled or added on the curve: an entry costs two row loads, the
// two c x products and the sparse merge with both w^3 coefficients in Fp (tower.cuh lines_merge_yy).  The only state is the two G1
// points, in LDS (x on the even lane, y on the odd one).  The table's base stays wave-uniform and both rows are 32-bit per-lane WORD
// offsets (the host keeps the table below 2^32 bytes).  A step function whose arguments are scalars.
#define LT_P0 0
#define LT_P1 FP_NL
#define LT_WORDS (2 * FP_NL)
static __device__ __noinline__ void lines_step_tables2(lds_u32* sh, const uint32_t* table, uint32_t off0, uint32_t off1, uint32_t* lines, size_t lanes,
                                                       uint32_t t, int e) {
  hfp2 a0, a2, b0, b2, c;
  fp x, ya, yb;
  gc_u32* tr = uni_global(table);
  const uint32_t eo = uni_u32((uint32_t)e) * (4 * FP_NL) + (lane_hi() ? FP_NL : 0);
  {
    const uint32_t o = off0 + eo;
#pragma unroll
    for (int k = 0; k < FP_NL; k++) {
      a0.v.l[k] = (int32_t)g_ld(tr, o + k);
      c.v.l[k] = (int32_t)g_ld(tr, o + 2 * FP_NL + k);
    }
  }
  ls_ld_coord(x, sh, LT_P0, false);
  fp2_mul_fp(a2, c, x);
  {
    const uint32_t o = off1 + eo;
#pragma unroll
    for (int k = 0; k < FP_NL; k++) {
      b0.v.l[k] = (int32_t)g_ld(tr, o + k);
      c.v.l[k] = (int32_t)g_ld(tr, o + 2 * FP_NL + k);
    }
  }
  ls_ld_coord(x, sh, LT_P1, false);
  fp2_mul_fp(b2, c, x);
  ls_ld_coord(ya, sh, LT_P0, true);
  ls_ld_coord(yb, sh, LT_P1, true);
  line5_t<hfp2> L;
  lines_merge_yy(L, a0, a2, ya, b0, b2, yb);
  line5_st(lines, lanes, t, e, L);
}
__global__ void __launch_bounds__(BLS_BLOCK, BLS_SPLIT_WAVES) __attribute__((disable_tail_calls))
k_lines2s_tables2(size_t n, size_t first, size_t count, const uint32_t* pairs, const int32_t* status, uint32_t* lines, size_t lanes, const uint32_t* table,
                  const uint32_t* t0, const uint32_t* t1) {
  const uint32_t t = blockIdx.x * BLS_BLOCK + threadIdx.x;
  const size_t j = t >> 1;
  if (j >= count) return;
  const size_t i = first + j;                          // the item's index in the BATCH: t0, t1 and the pairs are indexed by it
  if (status[i] != BLS_OK) return;                     // before any table read
  __shared__ uint32_t lsh[LT_WORDS * BLS_BLOCK];
  lds_u32* sh = lds_column(lsh);
  {
    fp p;
    ws_ld_fp(p, pairs, n, i, lane_hi() ? W1 : 0);                   // pair 0's G1 point: x on the even lane, y on the odd lane
    ls_st(sh, LT_P0, p);
    ws_ld_fp(p, pairs, n, i, 3 * W2 + (lane_hi() ? W1 : 0));        // pair 1's G1 point
    ls_st(sh, LT_P1, p);
  }
  const uint32_t off0 = t0[i] * (uint32_t)(MILLER_ENTRIES * 4 * FP_NL), off1 = t1[i] * (uint32_t)(MILLER_ENTRIES * 4 * FP_NL);
  for (int e = 0; e < MILLER_ENTRIES; e++) lines_step_tables2(sh, table, off0, off1, lines, lanes, t, e);
}
