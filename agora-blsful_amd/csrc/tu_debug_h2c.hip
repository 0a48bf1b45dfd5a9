// translation unit: the lane kernels of hash-to-curve (kernels.cuh k_hash_to_g1, k_hash_to_g2) in their UB = true form, which reads
// the uniform bytes from memory where the product runs expand_message_xmd: the self-test door blsgpu_debug_map_to_curve
#define BLS_TU_DEBUG_H2C 1
#include "kernels.cuh"
template __global__ void k_hash_to_g1<true>(size_t, const uint8_t*, const uint64_t*, dst_arg, uint8_t*, int);
template __global__ void k_hash_to_g2<true>(size_t, const uint8_t*, const uint64_t*, dst_arg, uint8_t*, int);
