// Kernels of the batched multi verify (blsgpu_multi_verify_batch, multi_batch.cuh), included by tu_multi_batch1.hip
// (BLS_TU_MULTI_BATCH = 1: G1 keys, i.e. Bls12381G2Impl) and tu_multi_batch2.hip (BLS_TU_MULTI_BATCH = 2: G2 keys, i.e.
// Bls12381G1Impl).  The fold after it is k_share_fold (tu_shares.inc); the hand-over to the verification tail is k_set_out
// (tu_secure.inc).
//   k_multi_accumulate_seg : every strip's plain sum of its keys, one RAW_PROJ partial per strip
#include "kernels.cuh"
#include "multi_batch.cuh"

#if BLS_TU_MULTI_BATCH == 1
// one lane per strip.  A key with Z = 1 (deserialised, RAW_AFFINE) takes the mixed addition, as in k_accumulate<1, 0>
template <>
__global__ void __launch_bounds__(BLS_BLOCK) k_multi_accumulate_seg<1>(size_t n_strips, const uint8_t* pts, int fmt, const uint64_t* key_offs,
                                                                     const uint64_t* strip_offs, const uint32_t* strip_sid, uint8_t* part) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_strips) return;
  const multi_strip st = multi_strip_of(g, key_offs, strip_offs, strip_sid);
  g1_jac acc, p;
  fp one;
  fp_one(one);
  jac_set_inf(acc);
  for (uint64_t i = st.first; i < st.end; i += st.stride) {
    load_g1_pt(p, pts, i, fmt);
    if (fp_eq(p.z, one)) jac_madd(acc, acc, p.x, p.y);
    else jac_add(acc, acc, p);
  }
  store_g1_pt(part, g, acc);
}
#else
// one lane pair per strip on the lane-split tower, as k_accumulate_g2s: both lanes of a pair walk the same strip
template <>
__global__ void __launch_bounds__(BLS_BLOCK, 2) k_multi_accumulate_seg<2>(size_t n_strips, const uint8_t* pts, int fmt, const uint64_t* key_offs,
                                                                        const uint64_t* strip_offs, const uint32_t* strip_sid, uint8_t* part) {
  const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (g >= n_strips) return;
  const multi_strip st = multi_strip_of(g, key_offs, strip_offs, strip_sid);
  jac<hfp2> acc, p;
  hfp2 one, d;
  fe_one(one);
  jac_set_inf(acc);
  for (uint64_t i = st.first; i < st.end; i += st.stride) {
    ld_g2s_fmt(p, pts, i, fmt);
    fe_sub(d, p.z, one);
    if (fe_is_zero(d)) jac_madd_body(acc, acc, p.x, p.y);     // the bodies: the accumulator stays in registers (k_accumulate_g2s)
    else jac_add_body(acc, acc, p);
  }
  st_g2s(part, g, acc);
}
#endif
