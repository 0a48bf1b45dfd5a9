// translation unit: self-test kernels of blsgpu_debug_field_op (debug_ops.h) for what PRODUCES line values: the Miller steps of
// pairing.cuh on g2_hom_t<fp2>, one lane per item (MILLER1_*), and on g2_hom_t<hfp2>, two lanes per item (MILLER2_*), the merges of
// tower.cuh (LINES_MERGE*) and miller_line3_row (LINE3_ROW).  Headers only: no section of kernels.cuh is compiled here, so no kernel
// of the library changes.
// k_dbg_miller1 keeps the launch bounds of the other self-test kernels (two waves per SIMD).  The one-lane steps with their record
// staging do not fit that register budget: the kernel spills (2,296 VGPR slots, 6.9 KB of scratch per lane).  That is harmless at the
// few hundred items a test runs, but it is a budget no shipped one-lane kernel runs these steps under: the row tests the arithmetic
// and the output forms of miller_*_step<fp2>, not a shipped kernel's register allocation.
#include "debug_ops_io.cuh"

// limb VECTOR number v of a record (the records of these rows mix Fp2 and Fp operands): an Fp operand is read by both lanes alike,
// of an Fp2 that starts at vector v the even lane takes vector v, the odd lane v + 1
static __device__ __forceinline__ void dbg_ldv(fp& r, const int32_t* rec, int v) { dbg_ld(r, rec + v * FP_NL); }
static __device__ __forceinline__ void dbg_ldv(fp2& r, const int32_t* rec, int v) {
  dbg_ld(r.c0, rec + v * FP_NL);
  dbg_ld(r.c1, rec + (v + 1) * FP_NL);
}
static __device__ __forceinline__ void dbg_ldv(hfp2& r, const int32_t* rec, int v) { dbg_ld(r.v, rec + (v + (lane_hi() ? 1 : 0)) * FP_NL); }
static __device__ __forceinline__ void dbg_stv(int32_t* rec, int v, const fp2& a) {
  dbg_st(rec + v * FP_NL, a.c0);
  dbg_st(rec + (v + 1) * FP_NL, a.c1);
}
static __device__ __forceinline__ void dbg_stv(int32_t* rec, int v, const hfp2& a) { dbg_st(rec + (v + (lane_hi() ? 1 : 0)) * FP_NL, a.v); }

// one step row on either Fp2: x = T (vectors 0..5), [xq, yq (6..9),] xp, yp, form; y = T', l0, l2, l3
template <class F2>
static __device__ __forceinline__ void dbg_miller_row(bool add, int reps, const int32_t* x, int32_t* y) {
  g2_hom_t<F2> t;
  F2 xq, yq, l0, l2, l3;
  fp xp, yp;
  dbg_ldv(t.x, x, 0);
  dbg_ldv(t.y, x, 2);
  dbg_ldv(t.z, x, 4);
  int v = 6;
  if (add) {
    dbg_ldv(xq, x, 6);
    dbg_ldv(yq, x, 8);
    v = 10;
  }
  dbg_ldv(xp, x, v);
  dbg_ldv(yp, x, v + 1);
  const int form = x[(v + 2) * FP_NL];
  for (int k = 0; k < reps; k++) {
    if (form) {
      const miller_regs<F2> st = {t, xp, yp, &xq, &yq};
      if (add) miller_add_step_at(st, l0, l2, l3);
      else miller_dbl_step_at(st, l0, l2, l3);
    } else {
      if (add) miller_add_step(t, l0, l2, l3, xq, yq, xp, yp);
      else miller_dbl_step(t, l0, l2, l3, xp, yp);
    }
  }
  dbg_stv(y, 0, t.x);
  dbg_stv(y, 2, t.y);
  dbg_stv(y, 4, t.z);
  dbg_stv(y, 6, l0);
  dbg_stv(y, 8, l2);
  dbg_stv(y, 10, l3);
}

__global__ void __launch_bounds__(BLS_BLOCK, BLS_SPLIT_WAVES) __attribute__((disable_tail_calls))
k_dbg_miller1(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out) {
  const size_t j = (size_t)blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (j >= n) return;
  dbg_miller_row<fp2>(op == DBG_MILLER1_ADD, reps, in + j * (size_t)rec_in, out + j * (size_t)rec_out);
}

static __device__ __forceinline__ void dbg_st_line5(int32_t* y, const line5_t<hfp2>& L) {
  dbg_stv(y, 0, L.c0);
  dbg_stv(y, 2, L.c2);
  dbg_stv(y, 4, L.c4);
  dbg_stv(y, 6, L.c3);
  dbg_stv(y, 8, L.c5);
}

__global__ void __launch_bounds__(BLS_BLOCK, BLS_SPLIT_WAVES) __attribute__((disable_tail_calls))
k_dbg_miller2s(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out) {
  const size_t j = ((size_t)blockIdx.x * BLS_BLOCK + threadIdx.x) >> 1;
  if (j >= n) return;
  const int32_t* x = in + j * (size_t)rec_in;
  int32_t* y = out + j * (size_t)rec_out;
  hfp2 a0, a2, a3, b0, b2, b3;
  fp ya, yb;
  line5_t<hfp2> L;
  switch (op) {
    case DBG_MILLER2_DBL:
    case DBG_MILLER2_ADD:
      dbg_miller_row<hfp2>(op == DBG_MILLER2_ADD, reps, x, y);
      break;
    case DBG_LINES_MERGE:
      dbg_ldv(a0, x, 0);
      dbg_ldv(a2, x, 2);
      dbg_ldv(a3, x, 4);
      dbg_ldv(b0, x, 6);
      dbg_ldv(b2, x, 8);
      dbg_ldv(b3, x, 10);
      lines_merge(L, a0, a2, a3, b0, b2, b3);
      dbg_st_line5(y, L);
      break;
    case DBG_LINES_MERGE_Y:
      dbg_ldv(a0, x, 0);
      dbg_ldv(a2, x, 2);
      dbg_ldv(a3, x, 4);
      dbg_ldv(b0, x, 6);
      dbg_ldv(b2, x, 8);
      dbg_ldv(yb, x, 10);
      lines_merge_y(L, a0, a2, a3, b0, b2, yb);
      dbg_st_line5(y, L);
      break;
    case DBG_LINES_MERGE_YY:
      dbg_ldv(a0, x, 0);
      dbg_ldv(a2, x, 2);
      dbg_ldv(ya, x, 4);
      dbg_ldv(b0, x, 5);
      dbg_ldv(b2, x, 7);
      dbg_ldv(yb, x, 9);
      lines_merge_yy(L, a0, a2, ya, b0, b2, yb);
      dbg_st_line5(y, L);
      break;
    default:   // DBG_LINE3_ROW: n0, c, x, y
      dbg_ldv(a0, x, 0);
      dbg_ldv(a2, x, 2);
      dbg_ldv(ya, x, 4);
      dbg_ldv(yb, x, 5);
      miller_line3_row(b0, b2, b3, a0, a2, ya, yb);
      dbg_stv(y, 0, b0);
      dbg_stv(y, 2, b2);
      dbg_stv(y, 4, b3);
      break;
  }
}
