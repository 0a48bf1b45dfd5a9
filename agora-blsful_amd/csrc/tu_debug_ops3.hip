// translation unit: self-test kernel of blsgpu_debug_field_op (debug_ops.h) for fp12_pow_x, the Fp12 inversion and the Frobenius
// maps on the lane-split tower.  Tower headers only.
#include "debug_ops_io.cuh"

static __device__ __noinline__ void dbg_frob1(fp12_t<hfp2>& r, const fp12_t<hfp2>& a) { fp12_frob<1>(r, a); }
static __device__ __noinline__ void dbg_frob2(fp12_t<hfp2>& r, const fp12_t<hfp2>& a) { fp12_frob<2>(r, a); }

__global__ void __launch_bounds__(BLS_BLOCK, BLS_SPLIT_WAVES) __attribute__((disable_tail_calls))
k_dbg_f12misc(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out) {
  const size_t j = ((size_t)blockIdx.x * BLS_BLOCK + threadIdx.x) >> 1;
  if (j >= n) return;
  const int32_t* x = in + j * (size_t)rec_in;
  int32_t* y = out + j * (size_t)rec_out;
  fp12_t<hfp2> a, r;
  dbg_ld12(a, x, 0);
  switch (op) {
    case DBG_F12_POW_X:
      fp12_pow_x(r, a);
      break;
    case DBG_F12_INV:
      fp12_inv(r, a);
      break;
    case DBG_F12_FROB1:
      dbg_frob1(r, a);
      break;
    default:
      dbg_frob2(r, a);
      break;
  }
  dbg_st12(y, r);
}
