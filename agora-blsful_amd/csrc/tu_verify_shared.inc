// Kernels of the shared-message verify calls (blsgpu_verify_shared_batch, blsgpu_verify_shared_indexed_batch; verify_shared.cuh),
// included by tu_verify_shared1.hip (BLS_TU_VERIFY_SHARED = 1: Bls12381G1Impl's instances and the group-independent kernel) and
// tu_verify_shared2.hip (BLS_TU_VERIFY_SHARED = 2: Bls12381G2Impl's instances, and the per-group line tables of its lane-split path).
//   k_group_affine   : H(m_g) of every group to affine, one inversion per group
//   k_prepare_shared : one item per lane -> its group, the identity checks and the two-pair record
//   k_shared_expand  : MessageAugmentation only: the groups' messages copied out per item
//   k_group_lines    : Bls12381G2Impl, lane-split path: the normalised line table of every group's H(m), one lane pair per group
#include "kernels.cuh"
#include "verify_shared.cuh"

template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK) k_group_affine(size_t n_groups, const uint8_t* hashes, uint8_t* aff) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  typedef grp<SG> HG;
  typename HG::jac_t h;
  typename HG::aff_t a;
  HG::load(h, hashes, g, 0);
  jac_to_aff(a, h);                       // the identity: zero coordinates, which the RAW_AFFINE reader takes for the identity again
  uint32_t* w = (uint32_t*)(aff + g * (size_t)(96 * SG));
  if constexpr (SG == 1) {
    fp_to_raw(w, a.x);
    fp_to_raw(w + 12, a.y);
  } else {
    fp2_to_raw(w, a.x);
    fp2_to_raw(w + 24, a.y);
  }
}

template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK) k_prepare_shared(size_t n, size_t n_groups, const uint64_t* item_offs, const uint8_t* pks,
                                                            const uint8_t* sigs, int fmt, const uint8_t* group_aff, uint32_t* pairs,
                                                            int32_t* status, int swap, uint32_t* group_of) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t g = shared_group_of(item_offs, n_groups, (uint64_t)i);
  typedef grp<SG> HG;
  typedef grp<3 - SG> KG;
  typename KG::jac_t pk;
  typename HG::jac_t sig, hj;
  typename HG::aff_t h;
  KG::load(pk, pks, i, fmt);
  HG::load(sig, sigs, i, fmt);
  HG::load(hj, group_aff, g, 1);          // Z = 1, or the identity for the zero record
  h.x = hj.x;
  h.y = hj.y;
  h.inf = jac_is_inf(hj);
  if (h.inf) {
    fe_zero(h.x);
    fe_zero(h.y);
  }
  g1_aff P[2];
  g2_aff Q[2];
  int st;
  if constexpr (SG == 1) st = prepare_shared_item(P, Q, pk, sig, h);
  else st = prepare_shared_item(P, Q, pk, sig, h, swap != 0);
  status[i] = st;
  if (group_of) group_of[i] = (uint32_t)g;
  if (st != BLS_OK) return;
  ws_st_pair(pairs, n, i, 0, P[0], Q[0]);
  ws_st_pair(pairs, n, i, 1, P[1], Q[1]);
}

template __global__ void k_group_affine<BLS_TU_VERIFY_SHARED>(size_t, const uint8_t*, uint8_t*);
template __global__ void k_prepare_shared<BLS_TU_VERIFY_SHARED>(size_t, size_t, const uint64_t*, const uint8_t*, const uint8_t*, int, const uint8_t*, uint32_t*,
                                                                int32_t*, int, uint32_t*);

#if BLS_TU_VERIFY_SHARED == 1
__global__ void __launch_bounds__(BLS_BLOCK) k_shared_expand(size_t total, const uint64_t* x_offs, size_t n_items, const uint64_t* item_offs,
                                                           size_t n_groups, const uint64_t* msg_offs, const uint8_t* msgs, uint8_t* out) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= total) return;
  out[b] = msgs[shared_expand_src(x_offs, n_items, item_offs, n_groups, msg_offs, (uint64_t)b)];
}
#endif

#if BLS_TU_VERIFY_SHARED == 2
// (group_lines_io, where the lane pair keeps a group's values: verify_shared.cuh)
__global__ void __launch_bounds__(BLS_BLOCK) k_group_lines(size_t n_groups, const uint8_t* group_aff, uint32_t* table, uint32_t* scratch, int32_t* flags) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t g = t >> 1;                                  // both lanes of a pair are inside or outside: BLS_BLOCK is even
  if (g >= n_groups) return;
  const uint32_t* w = (const uint32_t*)(group_aff + g * 192);
  const bool inf = words_all_zero(w, 48);
  const uint32_t o = lane_hi() ? 12 : 0;
  hfp2 qx, qy;
  fp_from_raw(qx.v, w + o);
  fp_from_raw(qy.v, w + 24 + o);
  const size_t base = g * (size_t)SHARED_TABLE_WORDS + (lane_hi() ? FP_NL : 0);
  const group_lines_io io = {table + base, scratch + base};
  const bool ok = group_lines_build(qx, qy, inf, io);
  if (!lane_hi()) {
    flags[g] = ok ? 0 : 1;
    if (!ok) atomicOr(&flags[n_groups], 1);
  }
}
#endif
