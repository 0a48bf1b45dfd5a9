// record accessors shared by the self-test kernels of tu_debug_ops*.hip (debug_ops.h): limb vectors travel as they are
#pragma once
#include "tower_split.cuh"
#include "debug_ops.h"

__device__ __forceinline__ void dbg_ld(fp& r, const int32_t* p) {
#pragma unroll
  for (int i = 0; i < FP_NL; i++) r.l[i] = p[i];
}
__device__ __forceinline__ void dbg_st(int32_t* p, const fp& a) {
#pragma unroll
  for (int i = 0; i < FP_NL; i++) p[i] = a.l[i];
}
// Fp2 number k of a record: the even lane takes its c0, the odd lane its c1
__device__ __forceinline__ void dbg_ld2(hfp2& r, const int32_t* rec, int k) { dbg_ld(r.v, rec + (2 * k + (lane_hi() ? 1 : 0)) * FP_NL); }
__device__ __forceinline__ void dbg_st2(int32_t* rec, int k, const hfp2& a) { dbg_st(rec + (2 * k + (lane_hi() ? 1 : 0)) * FP_NL, a.v); }
// Fp12 in tower order starting at Fp2 number k0
__device__ __forceinline__ void dbg_ld12(fp12_t<hfp2>& f, const int32_t* rec, int k0) {
  dbg_ld2(f.c0.a0, rec, k0);
  dbg_ld2(f.c0.a1, rec, k0 + 1);
  dbg_ld2(f.c0.a2, rec, k0 + 2);
  dbg_ld2(f.c1.a0, rec, k0 + 3);
  dbg_ld2(f.c1.a1, rec, k0 + 4);
  dbg_ld2(f.c1.a2, rec, k0 + 5);
}
__device__ __forceinline__ void dbg_st12(int32_t* rec, const fp12_t<hfp2>& f) {
  dbg_st2(rec, 0, f.c0.a0);
  dbg_st2(rec, 1, f.c0.a1);
  dbg_st2(rec, 2, f.c0.a2);
  dbg_st2(rec, 3, f.c1.a0);
  dbg_st2(rec, 4, f.c1.a1);
  dbg_st2(rec, 5, f.c1.a2);
}
