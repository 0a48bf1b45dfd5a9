// translation unit: the wave and workgroup kernels of hash-to-curve (kernels.cuh k_hash_to_g1_wide, k_hash_to_g1_engine,
// k_hash_to_g2_engine, k_hash_to_g2_maps) in their UB = true form, which reads the uniform bytes from memory where the product runs
// expand_message_xmd_wave: the self-test door blsgpu_debug_map_to_curve.  Compiled as tu_wide.hip is.
#define BLS_TU_DEBUG_H2C_WIDE 1
#define BLS_FP_INV_VAR 1
#include "kernels.cuh"
#include "debug_ops.h"
template __global__ void k_hash_to_g1_wide<true>(size_t, const uint8_t*, const uint64_t*, int, dst_arg, uint8_t*, uint32_t*);
template __global__ void k_hash_to_g1_engine<true>(size_t, const uint8_t*, const uint64_t*, int, dst_arg, uint8_t*, uint32_t*);
template __global__ void k_hash_to_g2_engine<true>(size_t, const uint8_t*, const uint64_t*, int, dst_arg, uint8_t*, uint32_t*);
template __global__ void k_hash_to_g2_maps<true>(size_t, const uint8_t*, const uint64_t*, int, dst_arg, uint32_t*);

// where a form's only output is the cut check's record: its three engine values at WREC_P0 as a RAW_PROJ point, one lane per item
__global__ void __launch_bounds__(BLS_BLOCK) k_dbg_rec_g1_to_raw(size_t n, const uint32_t* rec, uint8_t* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int v = 0; v < 3; v++) {
    fp x;
    w_load_local(x, rec + i * WREC_WORDS + 16 * (WREC_P0 + v));
    fp_to_raw((uint32_t*)(out + i * 144) + 12 * v, x);
  }
}
