// Kernels of the registered message sets (blsgpu_msgset_*, blsgpu_verify_msgset_batch, blsgpu_verify_msgset_indexed_batch; msgset.cuh),
// included by tu_msgset1.hip (BLS_TU_MSGSET = 1: the group-independent kernels and Bls12381G1Impl) and tu_msgset2.hip (BLS_TU_MSGSET = 2:
// Bls12381G2Impl).  The rows of a Bls12381G2Impl set are built by the key sets' k_keyset_lines / k_keyset_lines_at: a stored G2 record
// is the same 192 bytes in both tables.
//   k_msgset_seal  : create / update / append: a hash output to the stored affine record of its entry
//   k_msgset_check : every group's index against the set, once; whether every named entry has rows
//   k_msgset_mark  : BLSGPU_E_ARG into the items of a group that names no entry; the items' entries
#include "kernels.cuh"
#include "msgset.cuh"

template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK) k_msgset_seal(size_t cnt, const uint8_t* hashes, const uint32_t* pos, size_t first, uint8_t* recs) {
  const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= cnt) return;
  typedef grp<SG> HG;
  typename HG::jac_t h;
  typename HG::aff_t a;
  HG::load(h, hashes, l, 0);
  jac_to_aff(a, h);                       // the identity: zero coordinates, which the RAW_AFFINE reader takes for the identity again
  const size_t k = pos ? (size_t)pos[l] : first + l;
  uint32_t* w = (uint32_t*)(recs + k * (size_t)(96 * SG));
  if constexpr (SG == 1) {
    fp_to_raw(w, a.x);
    fp_to_raw(w + 12, a.y);
  } else {
    fp2_to_raw(w, a.x);
    fp2_to_raw(w + 24, a.y);
  }
}
template __global__ void k_msgset_seal<BLS_TU_MSGSET>(size_t, const uint8_t*, const uint32_t*, size_t, uint8_t*);

#if BLS_TU_MSGSET == 1
__global__ void __launch_bounds__(BLS_BLOCK) k_msgset_check(size_t n_groups, const uint32_t* msg_idx, uint64_t n_msgs, const int32_t* nolines, uint32_t* cmsg,
                                                          uint32_t* walk) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  const uint32_t k = msgset_entry_of(msg_idx[g], n_msgs);
  cmsg[g] = k;
  if (nolines && k != MSGSET_SKIP && nolines[k] != 0) atomicOr(walk, 1u);     // nothing outside the set is read
}
__global__ void __launch_bounds__(BLS_BLOCK) k_msgset_mark(size_t n, const uint32_t* group_of, const uint32_t* cmsg, int32_t* status, uint32_t* msg_of) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = cmsg[group_of[i]];
  if (k == MSGSET_SKIP) status[i] = MSGSET_E_ARG;
  if (msg_of) msg_of[i] = k == MSGSET_SKIP ? 0u : k;
}
#endif
