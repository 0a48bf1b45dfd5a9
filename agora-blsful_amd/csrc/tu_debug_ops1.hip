// translation unit: self-test kernels of blsgpu_debug_field_op (debug_ops.h) for the field leaves and the lane-split Fp2.
// Tower headers only: no section of kernels.cuh is compiled here, so no kernel of the library changes.
#include "debug_ops_io.cuh"

// the two halves of the pack / unpack round trip behind calls: inlined into one kernel the compiler forwards the stores to the loads and
// drops the LDS array, and the column addressing would go untested
static __device__ __noinline__ void dbg_pack_st(lds_u32* sh, const fp12_t<hfp2>& f) { sh_st_f12(sh, f); }
static __device__ __noinline__ void dbg_pack_ld(fp12_t<hfp2>& f, const lds_u32* sh) { sh_ld_f12(f, sh); }

// one lane per item: the one-lane code of k_prepare, the MSM and the point kernels
__global__ void __launch_bounds__(BLS_BLOCK, BLS_SPLIT_WAVES) __attribute__((disable_tail_calls))
k_dbg_fp1(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out) {
  const size_t i = (size_t)blockIdx.x * BLS_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t* x = in + i * (size_t)rec_in;
  int32_t* y = out + i * (size_t)rec_out;
  fp a, b, c, d, r, s;
  switch (op) {
    case DBG_FP_NORM:
      dbg_ld(a, x);
      fp_norm(r, a);
      dbg_st(y, r);
      break;
    case DBG_FP_REDUCE:
      dbg_ld(a, x);
      fp_reduce(r, a);
      dbg_st(y, r);
      break;
    case DBG_FP_CANON: {
      dbg_ld(a, x);
      fp_canon(r, a);
      dbg_st(y, r);
      uint32_t w[12];
      fp_to_raw(w, a);
      y[FP_NL] = fp_is_zero(a) ? 1 : 0;
      for (int k = 0; k < 12; k++) y[FP_NL + 1 + k] = (int32_t)w[k];
      y[2 * FP_NL - 1] = 0;
      break;
    }
    case DBG_FP_REDUCE_LIN2:
      dbg_ld(a, x);
      dbg_ld(b, x + FP_NL);
      // the function takes its coefficients as scalars (the kernels pass constants): the pairs of the kernels and of the case list
      {
        const int ka = x[2 * FP_NL], kb = x[2 * FP_NL + 1];
        fp_zero(r);
#define DBG_LIN2(KA, KB) if (ka == (KA) && kb == (KB)) fp_reduce_lin2(r, a, (KA), b, (KB));
        DBG_LIN2(3, 2) else DBG_LIN2(3, -2) else DBG_LIN2(1, 1) else DBG_LIN2(12, 0) else DBG_LIN2(1, -12) else DBG_LIN2(-3, 5)
#undef DBG_LIN2
      }
      dbg_st(y, r);
      break;
    case DBG_FP_MUL:
      dbg_ld(a, x);
      dbg_ld(b, x + FP_NL);
      for (int k = 0; k < reps; k++) fp_mul(a, a, b);
      dbg_st(y, a);
      break;
    case DBG_FP_SQR:
      dbg_ld(a, x);
      for (int k = 0; k < reps; k++) fp_sqr(a, a);
      dbg_st(y, a);
      break;
    case DBG_FP_INV:
      dbg_ld(a, x);
      fp_inv(r, a);
      dbg_st(y, r);
      break;
    case DBG_FP_INV_VAR:
      dbg_ld(a, x);
      fp_inv_var(r, a);
      dbg_st(y, r);
      break;
    case DBG_FP_SQRT: {
      dbg_ld(a, x);
      const bool ok = fp_sqrt(r, a);
      const bool sq = fp_is_square(a);
      dbg_st(y, r);
      for (int k = 0; k < FP_NL; k++) y[FP_NL + k] = 0;
      y[FP_NL] = ok ? 1 : 0;
      y[FP_NL + 1] = sq ? 1 : 0;
      break;
    }
    case DBG_FP_FROM_RAW: {
      uint32_t w[12];
      for (int k = 0; k < 12; k++) w[k] = (uint32_t)x[k];
      fp_from_raw(r, w);
      dbg_st(y, r);
      break;
    }
    case DBG_FP2_KARA_PRODUCTS:
    case DBG_FP2_KARA_DIFFS:
      dbg_ld(a, x);
      dbg_ld(b, x + FP_NL);
      dbg_ld(c, x + 2 * FP_NL);
      dbg_ld(d, x + 3 * FP_NL);
      if (op == DBG_FP2_KARA_PRODUCTS) fp2_kara_products(r, s, a, b, c, d);
      else fp2_kara_diffs(r, s, a, b, c, d);
      dbg_st(y, r);
      dbg_st(y + FP_NL, s);
      break;
    case DBG_FP2L_MUL:
    case DBG_FP2L_SQR:
    case DBG_FP2L_INV: {
      fp2 u, v, w;
      dbg_ld(u.c0, x);
      dbg_ld(u.c1, x + FP_NL);
      if (op == DBG_FP2L_MUL) {
        dbg_ld(v.c0, x + 2 * FP_NL);
        dbg_ld(v.c1, x + 3 * FP_NL);
        fp2_mul(w, u, v);
      } else if (op == DBG_FP2L_SQR) {
        fp2_sqr(w, u);
      } else {
        fp2_inv(w, u);
      }
      dbg_st(y, w.c0);
      dbg_st(y + FP_NL, w.c1);
      break;
    }
    default:
      break;
  }
}

// two lanes per item: the lane-split Fp2 and the packed LDS form of an Fp12
__global__ void __launch_bounds__(BLS_BLOCK, BLS_SPLIT_WAVES) __attribute__((disable_tail_calls))
k_dbg_fp2s(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out) {
  const size_t j = ((size_t)blockIdx.x * BLS_BLOCK + threadIdx.x) >> 1;
  if (j >= n) return;
  const int32_t* x = in + j * (size_t)rec_in;
  int32_t* y = out + j * (size_t)rec_out;
  __shared__ uint32_t fsh[F12_SH_WORDS * BLS_BLOCK];
  hfp2 a, b, r;
  switch (op) {
    case DBG_FP2_MUL:
      dbg_ld2(a, x, 0);
      dbg_ld2(b, x, 1);
      for (int k = 0; k < reps; k++) fp2_mul(a, a, b);
      dbg_st2(y, 0, a);
      break;
    case DBG_FP2_SQR:
      dbg_ld2(a, x, 0);
      for (int k = 0; k < reps; k++) fp2_sqr(a, a);
      dbg_st2(y, 0, a);
      break;
    case DBG_FP2_MUL_XI:
      dbg_ld2(a, x, 0);
      fp2_mul_xi(r, a);
      dbg_st2(y, 0, r);
      break;
    case DBG_FP2_MUL_FP: {
      fp k;
      dbg_ld2(a, x, 0);
      dbg_ld(k, x + 2 * FP_NL);
      fp2_mul_fp(r, a, k);
      dbg_st2(y, 0, r);
      break;
    }
    case DBG_FP2_CONJ:
      dbg_ld2(a, x, 0);
      fp2_conj(r, a);
      dbg_st2(y, 0, r);
      break;
    case DBG_FP2_INV:
      dbg_ld2(a, x, 0);
      fp2_inv(r, a);
      dbg_st2(y, 0, r);
      break;
    case DBG_F12_PACK: {
      lds_u32* sh = lds_column(fsh);
      fp12_t<hfp2> f, g;
      dbg_ld12(f, x, 0);
      dbg_pack_st(sh, f);
      dbg_pack_ld(g, sh);
      dbg_st12(y, g);
      break;
    }
    default:
      break;
  }
}
