// jac_dbl_quad: one lane-split G2 doubling shared by two lane pairs (k_msm_chunk_g2q, k_msm2_chunk_g2q of kernels.cuh; the self-test
// row G2Q_DBL of debug_ops.h).  DPP code: device only.
#pragma once
#include "tower_split.cuh"

// One G2 doubling by the FOUR lanes of a chunk -- two lane pairs that hold the same lane-split point: the schedule of
// jac_dbl_pair (h2c.cuh) one level up, lane PAIR 0 taking A = X^2, F = (3A)^2, YZ, E (D - X3) and lane pair 1 B = Y^2,
// C = B^2, (X + B)^2; the pairs exchange by DPP quad_perm [2,3,0,1].  Same operation order and reductions as jac_dbl_body.
__device__ __forceinline__ void hfp2_swap2(hfp2& r, const hfp2& a) {
#pragma unroll
  for (int i = 0; i < FP_NL; i++) r.v.l[i] = __builtin_amdgcn_mov_dpp(a.v.l[i], 0x4E, 0xF, 0xF, true);
}
__device__ __forceinline__ void hfp2_sel(hfp2& r, bool c, const hfp2& a, const hfp2& b) { fp_sel(r.v, c, a.v, b.v); }
__device__ __forceinline__ void jac_dbl_quad(jac<hfp2>& p, bool hi2) {
  hfp2 s1, s2, s3, in, a, b, o2, o3, D, E, t, x3, y3, z3, c8;
  hfp2_sel(in, hi2, p.y, p.x);
  fp2_sqr(s1, in);                // pair 0: A = X^2          pair 1: B = Y^2
  fp2_dbl(E, s1);
  fp2_add(E, E, s1);
  fp2_reduce(E, E);               // pair 0: E = 3A
  hfp2_sel(in, hi2, s1, E);
  fp2_sqr(s2, in);                // pair 0: F = E^2          pair 1: C = B^2
  fp2_add(t, p.x, s1);
  fp2_norm(t, t);                 //                          pair 1: X + B
  hfp2_sel(a, hi2, t, p.y);
  hfp2_sel(b, hi2, t, p.z);
  fp2_mul(s3, a, b);              // pair 0: Y Z              pair 1: (X + B)^2
  hfp2_swap2(o2, s2);             // pair 0: C
  hfp2_swap2(o3, s3);             // pair 0: (X + B)^2
  fp2_sub(t, o3, s1);
  fp2_sub(t, t, o2);
  fp2_dbl(D, t);
  fp2_reduce(D, D);               // D = 2((X + B)^2 - A - C)
  fp2_dbl(t, D);
  fp2_sub(t, s2, t);
  fp2_reduce(x3, t);              // X3 = F - 2D
  fp2_sub(t, D, x3);
  fp2_norm(t, t);
  fp2_mul(t, E, t);               // E (D - X3)
  fp2_dbl(c8, o2);
  fp2_dbl(c8, c8);
  fp2_reduce(c8, c8);
  fp2_dbl(c8, c8);                // 8C
  fp2_sub(t, t, c8);
  fp2_reduce(y3, t);
  fp2_dbl(z3, s3);
  fp2_reduce(z3, z3);             // Z3 = 2YZ
  hfp2_swap2(a, x3);
  hfp2_swap2(b, y3);
  hfp2_swap2(t, z3);
  hfp2_sel(p.x, hi2, a, x3);
  hfp2_sel(p.y, hi2, b, y3);
  hfp2_sel(p.z, hi2, t, z3);
}
