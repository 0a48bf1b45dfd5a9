// translation unit: self-test kernels of blsgpu_debug_field_op (debug_ops.h) for the Fp12 accumulator in LDS and the compressed
// squarings.  Tower headers only; the Fp12-level functions stay non-inlined, as in the kernels they are taken from.
#include "debug_ops_io.cuh"

// the forceinline bodies of tower_split.cuh behind calls, as k_millerf2s and k_finalexp2s wrap them
static __device__ __noinline__ void dbg_sh_mul_line5(lds_u32* sh, const line5_t<hfp2>& L) { f12_sh_mul_line5(sh, L); }
static __device__ __noinline__ void dbg_cyc_c_sqr_unpacked(lds_u32* sh) { f12_sh_cyc_c_sqr_unpacked_body(sh); }
static __device__ __noinline__ void dbg_cyc_c_sqr_kara(lds_u32* sh, const lds_u32* pa, const lds_u32* pb) { f12_sh_cyc_c_sqr_kara_body(sh, pa, pb); }

__global__ void __launch_bounds__(BLS_BLOCK, BLS_SPLIT_WAVES) __attribute__((disable_tail_calls))
k_dbg_f12acc(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out) {
  const size_t j = ((size_t)blockIdx.x * BLS_BLOCK + threadIdx.x) >> 1;
  if (j >= n) return;
  const int32_t* x = in + j * (size_t)rec_in;
  int32_t* y = out + j * (size_t)rec_out;
  __shared__ uint32_t fsh[F12_SH_WORDS * BLS_BLOCK];   // the accumulator, packed
  lds_u32* sh = lds_column(fsh);
  {
    fp12_t<hfp2> f;
    dbg_ld12(f, x, 0);
    sh_st_f12(sh, f);
  }
  switch (op) {
    case DBG_F12_SH_SQR:
      for (int k = 0; k < reps; k++) f12_sh_sqr(sh);
      break;
    case DBG_F12_SH_MUL: {
      fp12_t<hfp2> b;
      dbg_ld12(b, x, 6);
      for (int k = 0; k < reps; k++) f12_sh_mul(sh, b);
      break;
    }
    case DBG_F12_SH_MUL_LINE: {
      hfp2 l0, l2, l3;
      dbg_ld2(l0, x, 6);
      dbg_ld2(l2, x, 7);
      dbg_ld2(l3, x, 8);
      for (int k = 0; k < reps; k++) f12_sh_mul_line(sh, l0, l2, l3);
      break;
    }
    case DBG_F12_SH_MUL_2LINES: {
      hfp2 a0, a2, a3, b0, b2, b3;
      dbg_ld2(a0, x, 6);
      dbg_ld2(a2, x, 7);
      dbg_ld2(a3, x, 8);
      dbg_ld2(b0, x, 9);
      dbg_ld2(b2, x, 10);
      dbg_ld2(b3, x, 11);
      for (int k = 0; k < reps; k++) f12_sh_mul_2lines(sh, a0, a2, a3, b0, b2, b3);
      break;
    }
    case DBG_F12_SH_MUL_LINE5: {
      line5_t<hfp2> L;
      dbg_ld2(L.c0, x, 6);
      dbg_ld2(L.c2, x, 7);
      dbg_ld2(L.c4, x, 8);
      dbg_ld2(L.c3, x, 9);
      dbg_ld2(L.c5, x, 10);
      for (int k = 0; k < reps; k++) dbg_sh_mul_line5(sh, L);
      break;
    }
    case DBG_F12_SH_CYC_SQR:
      for (int k = 0; k < reps; k++) f12_sh_cyclotomic_sqr(sh);
      break;
    default:
      break;
  }
  fp12_t<hfp2> g;
  sh_ld_f12(g, sh);
  dbg_st12(y, g);
}

// the three compiled bodies of the compressed squaring on (z2, z3, z4, z5); k_finalexp2s runs the third one
__global__ void __launch_bounds__(BLS_BLOCK, BLS_SPLIT_WAVES) __attribute__((disable_tail_calls))
k_dbg_cyc(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out) {
  const size_t j = ((size_t)blockIdx.x * BLS_BLOCK + threadIdx.x) >> 1;
  if (j >= n) return;
  const int32_t* x = in + j * (size_t)rec_in;
  int32_t* y = out + j * (size_t)rec_out;
  __shared__ uint32_t fsh[F12_SH_WORDS * BLS_BLOCK];
  lds_u32* sh = lds_column(fsh);
  hfp2 z2, z3, z4, z5;
  dbg_ld2(z2, x, 0);
  dbg_ld2(z3, x, 1);
  dbg_ld2(z4, x, 2);
  dbg_ld2(z5, x, 3);
  switch (op) {
    case DBG_CYC_C_SQR:
      sh_st_fp(sh, 39, z2.v);
      sh_st_fp(sh, 26, z3.v);
      sh_st_fp(sh, 13, z4.v);
      sh_st_fp(sh, 65, z5.v);
      for (int k = 0; k < reps; k++) f12_sh_cyc_c_sqr(sh);
      sh_ld_fp(z2.v, sh, 39);
      sh_ld_fp(z3.v, sh, 26);
      sh_ld_fp(z4.v, sh, 13);
      sh_ld_fp(z5.v, sh, 65);
      break;
    case DBG_CYC_C_SQR_UNPACKED:
      shu_st_fp(sh, CYCU_Z2, z2.v);
      shu_st_fp(sh, CYCU_Z3, z3.v);
      shu_st_fp(sh, CYCU_Z4, z4.v);
      shu_st_fp(sh, CYCU_Z5, z5.v);
      for (int k = 0; k < reps; k++) dbg_cyc_c_sqr_unpacked(sh);
      shu_ld_fp(z2.v, sh, CYCU_Z2);
      shu_ld_fp(z3.v, sh, CYCU_Z3);
      shu_ld_fp(z4.v, sh, CYCU_Z4);
      shu_ld_fp(z5.v, sh, CYCU_Z5);
      break;
    case DBG_CYC_C_SQR_KARA: {
      cyck_from_split(sh, z2.v, z3.v, z4.v, z5.v);
      const bool hi = lane_hi();
      const lds_u32* pa = sh + (hi ? CYCK_Q : CYCK_P) * BLS_SH_STRIDE;
      const lds_u32* pb = sh + (hi ? CYCK_P : CYCK_Q) * BLS_SH_STRIDE;
      for (int k = 0; k < reps; k++) dbg_cyc_c_sqr_kara(sh, pa, pb);
      cyck_to_split(z2.v, z3.v, z4.v, z5.v, sh);
      break;
    }
    default:
      break;
  }
  dbg_st2(y, 0, z2);
  dbg_st2(y, 1, z3);
  dbg_st2(y, 2, z4);
  dbg_st2(y, 3, z5);
}
