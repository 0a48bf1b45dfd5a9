// translation unit: self-test kernels of blsgpu_debug_field_op (debug_ops.h) for the curve layer on the lane-split Fp2: the point
// functions of curve.cuh and msm2.cuh on jac<hfp2>, two lanes per item (G2S_*), and jac_dbl_quad of curve_quad.cuh, four lanes per
// item (G2Q_DBL).  Headers only: no section of kernels.cuh is compiled here, so no kernel of the library changes.
#include "debug_ops_io.cuh"
#include "msm2.cuh"
#include "curve_quad.cuh"

// the Jacobian point whose X is Fp2 number k0 of the record: each lane takes its component of every coordinate
static __device__ __forceinline__ void dbg_ldj2(jac<hfp2>& p, const int32_t* rec, int k0) {
  dbg_ld2(p.x, rec, k0);
  dbg_ld2(p.y, rec, k0 + 1);
  dbg_ld2(p.z, rec, k0 + 2);
}
static __device__ __forceinline__ void dbg_stj2(int32_t* rec, int k0, const jac<hfp2>& p) {
  dbg_st2(rec, k0, p.x);
  dbg_st2(rec, k0 + 1, p.y);
  dbg_st2(rec, k0 + 2, p.z);
}

__global__ void __launch_bounds__(BLS_BLOCK, BLS_SPLIT_WAVES) __attribute__((disable_tail_calls))
k_dbg_pt2s(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out) {
  const size_t j = ((size_t)blockIdx.x * BLS_BLOCK + threadIdx.x) >> 1;
  if (j >= n) return;
  const int32_t* x = in + j * (size_t)rec_in;
  int32_t* y = out + j * (size_t)rec_out;
  jac<hfp2> p, q;
  dbg_ldj2(p, x, 0);
  switch (op) {
    case DBG_G2S_DBL: {
      const int form = x[6 * FP_NL];
      for (int k = 0; k < reps; k++) {
        if (form) jac_dbl_body(p, p);
        else jac_dbl(p, p);
      }
      dbg_stj2(y, 0, p);
      break;
    }
    case DBG_G2S_ADD: {
      dbg_ldj2(q, x, 3);
      const int form = x[12 * FP_NL];
      for (int k = 0; k < reps; k++) {
        if (form) jac_add_body(p, p, q);
        else jac_add(p, p, q);
      }
      dbg_stj2(y, 0, p);
      break;
    }
    case DBG_G2S_MADD: {
      hfp2 x2, y2;
      dbg_ld2(x2, x, 3);
      dbg_ld2(y2, x, 4);
      const int form = x[10 * FP_NL];
      for (int k = 0; k < reps; k++) {
        if (form) jac_madd_body(p, p, x2, y2);
        else jac_madd(p, p, x2, y2);
      }
      dbg_stj2(y, 0, p);
      break;
    }
    case DBG_G2S_PSI:
      g2_psi(q, p);
      dbg_stj2(y, 0, q);
      break;
    case DBG_G2S_PSI2:
      g2_psi2(q, p);
      dbg_stj2(y, 0, q);
      break;
    default:
      g2_clear_cofactor(q, p);
      dbg_stj2(y, 0, q);
      break;
  }
}

// four lanes per item: both lane pairs load the same point (k_msm_chunk_g2q holds its accumulator so) and each writes the point it
// ends with -- pair 0 to Fp2 numbers 0..2 of the output record, pair 1 to 3..5
__global__ void __launch_bounds__(BLS_BLOCK, BLS_SPLIT_WAVES) __attribute__((disable_tail_calls))
k_dbg_g2q(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out) {
  const size_t gid = (size_t)blockIdx.x * BLS_BLOCK + threadIdx.x, j = gid >> 2;
  const bool hi2 = ((gid >> 1) & 1) != 0;
  if (j >= n) return;
  (void)op;
  jac<hfp2> p;
  dbg_ldj2(p, in + j * (size_t)rec_in, 0);
  for (int k = 0; k < reps; k++) jac_dbl_quad(p, hi2);
  dbg_stj2(out + j * (size_t)rec_out, hi2 ? 3 : 0, p);
}
