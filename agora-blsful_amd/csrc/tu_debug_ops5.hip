// translation unit: self-test kernel of blsgpu_debug_field_op (debug_ops.h) for the curve layer, one lane per item: the point
// functions of curve.cuh and msm2.cuh on jac<fp> (G1_*) and jac<fp2> (G2L_*).  Headers only: no section of kernels.cuh is compiled
// here, so no kernel of the library changes.
#include "debug_ops_io.cuh"
#include "msm2.cuh"

// field element number k of a record: one limb vector over Fp, two (c0, c1) over Fp2
static __device__ __forceinline__ void dbg_ldf(fp& r, const int32_t* rec, int k) { dbg_ld(r, rec + k * FP_NL); }
static __device__ __forceinline__ void dbg_ldf(fp2& r, const int32_t* rec, int k) {
  dbg_ld(r.c0, rec + 2 * k * FP_NL);
  dbg_ld(r.c1, rec + (2 * k + 1) * FP_NL);
}
static __device__ __forceinline__ void dbg_stf(int32_t* rec, int k, const fp& a) { dbg_st(rec + k * FP_NL, a); }
static __device__ __forceinline__ void dbg_stf(int32_t* rec, int k, const fp2& a) {
  dbg_st(rec + 2 * k * FP_NL, a.c0);
  dbg_st(rec + (2 * k + 1) * FP_NL, a.c1);
}
template <class F>
static __device__ __forceinline__ void dbg_ldj(jac<F>& p, const int32_t* rec, int k0) {
  dbg_ldf(p.x, rec, k0);
  dbg_ldf(p.y, rec, k0 + 1);
  dbg_ldf(p.z, rec, k0 + 2);
}
template <class F>
static __device__ __forceinline__ void dbg_stj(int32_t* rec, const jac<F>& p) {
  dbg_stf(rec, 0, p.x);
  dbg_stf(rec, 1, p.y);
  dbg_stf(rec, 2, p.z);
}
static __device__ __forceinline__ bool dbg_in_subgroup(const g1_aff& a) { return g1_in_subgroup(a); }
static __device__ __forceinline__ bool dbg_in_subgroup(const g2_aff& a) { return g2_in_subgroup(a); }

// row number `row` of a group's block (G1_DBL / G2L_DBL = 0); W: limb vectors per field element
template <class F, int W>
static __device__ __forceinline__ void dbg_point_row(int row, int reps, const int32_t* x, int32_t* y) {
  jac<F> p, q;
  switch (row) {
    case DBG_G1_DBL - DBG_G1_DBL: {
      dbg_ldj(p, x, 0);
      const int form = x[3 * W * FP_NL];
      for (int k = 0; k < reps; k++) {
        if (form) jac_dbl_body(p, p);
        else jac_dbl(p, p);
      }
      dbg_stj(y, p);
      break;
    }
    case DBG_G1_ADD - DBG_G1_DBL: {
      dbg_ldj(p, x, 0);
      dbg_ldj(q, x, 3);
      const int form = x[6 * W * FP_NL];
      for (int k = 0; k < reps; k++) {
        if (form) jac_add_body(p, p, q);
        else jac_add(p, p, q);
      }
      dbg_stj(y, p);
      break;
    }
    case DBG_G1_MADD - DBG_G1_DBL: {
      F x2, y2;
      dbg_ldj(p, x, 0);
      dbg_ldf(x2, x, 3);
      dbg_ldf(y2, x, 4);
      const int form = x[5 * W * FP_NL];
      for (int k = 0; k < reps; k++) {
        if (form) jac_madd_body(p, p, x2, y2);
        else jac_madd(p, p, x2, y2);
      }
      dbg_stj(y, p);
      break;
    }
    case DBG_G1_TO_AFF - DBG_G1_DBL: {
      aff<F> a;
      dbg_ldj(p, x, 0);
      jac_to_aff(a, p);
      dbg_stf(y, 0, a.x);
      dbg_stf(y, 1, a.y);
      for (int k = 0; k < FP_NL; k++) y[2 * W * FP_NL + k] = 0;
      y[2 * W * FP_NL] = a.inf ? 1 : 0;
      break;
    }
    case DBG_G1_MUL_U64 - DBG_G1_DBL: {
      dbg_ldj(p, x, 0);
      const int32_t* par = x + 3 * W * FP_NL;
      jac_mul_u64(q, p, ((uint64_t)(uint32_t)par[1] << 32) | (uint32_t)par[0]);
      dbg_stj(y, q);
      break;
    }
    case DBG_G1_MUL_SCALAR - DBG_G1_DBL: {
      dbg_ldj(p, x, 0);
      uint32_t k[8];
      for (int i = 0; i < 8; i++) k[i] = (uint32_t)x[3 * W * FP_NL + i];
      jac_mul_scalar(q, p, k);
      dbg_stj(y, q);
      break;
    }
    case DBG_G1_IN_SUBGROUP - DBG_G1_DBL: {
      aff<F> a;
      dbg_ldf(a.x, x, 0);
      dbg_ldf(a.y, x, 1);
      a.inf = x[2 * W * FP_NL] != 0;
      const bool in = dbg_in_subgroup(a);
      for (int k = 0; k < FP_NL; k++) y[k] = 0;
      y[0] = in ? 1 : 0;
      break;
    }
    default:
      if constexpr (W == 2) {
        dbg_ldj(p, x, 0);
        if (row == DBG_G2L_PSI - DBG_G2L_DBL) g2_psi(q, p);
        else if (row == DBG_G2L_PSI2 - DBG_G2L_DBL) g2_psi2(q, p);
        else g2_clear_cofactor(q, p);
        dbg_stj(y, q);
      }
      break;
  }
}

__global__ void __launch_bounds__(BLS_BLOCK, BLS_SPLIT_WAVES) __attribute__((disable_tail_calls))
k_dbg_pt1(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out) {
  const size_t i = (size_t)blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t* x = in + i * (size_t)rec_in;
  int32_t* y = out + i * (size_t)rec_out;
  if (op >= DBG_G2L_DBL) dbg_point_row<fp2, 2>(op - DBG_G2L_DBL, reps, x, y);
  else dbg_point_row<fp, 1>(op - DBG_G1_DBL, reps, x, y);
}
