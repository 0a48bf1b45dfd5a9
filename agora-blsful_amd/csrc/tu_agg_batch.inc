// Kernels of the batched aggregate verify (blsgpu_aggregate_verify_batch, agg_batch.cuh), included by tu_agg_batch1.hip
// (BLS_TU_AGG_BATCH = 1: k_prepare_agg_seg<1> and the index kernels) and tu_agg_batch2.hip (BLS_TU_AGG_BATCH = 2:
// k_prepare_agg_seg<2> and the segmented Fp12 product).  Only the sets below BLSGPU_AGG_BATCH_MAX pairs run here, as one flat list
// of M = T_b + n_b items (pairs, then one signature item per set); the Miller values between k_prepare_agg_seg and k_f12_fold_seg
// are k_linesp pass 1 + k_millerfp3, the verdicts between k_agg_batch_mark and k_agg_batch_fin k_finalexp2s (kernels.cuh).
//   k_prepare_agg_seg : hash-to-curve, identity flag and affine pair of every item (k_prepare_agg's item), and the maps sid / src
//   k_agg_flat_keys   : over a registered key set, the entry that is each pair item's key (k_linesp_keyed reads its rows)
//   k_first_bad_seg   : per set the first identity key and whether the signature is the identity (sig_core.rs:155-167)
//   k_dup_insert_seg / k_dup_find_seg : Basic's duplicate rule per set (sig_basic.rs:46-58)
//   k_f12_fold_seg    : one halving round of every set's product; k_f12_fold_seg_out: times the signature's value, one record per set
//   k_agg_batch_mark  : the sets the rules above decide, marked so that the final exponentiation skips them
//   k_agg_batch_fin   : the reference's precedence -> the caller's status / aux
//   k_agg_large_fin   : the same for a large set run through the single call's kernels
#include "kernels.cuh"
#include "agg_batch.cuh"

// Item i < T_b is pair i - boffs[b] of set b = the last one with boffs[b] <= i, the caller's pair bsrc[b] + that; item T_b + b is
// set b's signature, the caller's signature bset[b].  The workspace stride is M.
template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK, 2) k_prepare_agg_seg(size_t M, size_t T_b, size_t n_b, const uint64_t* boffs, const uint64_t* bsrc,
                                                                const uint32_t* bset, const uint8_t* pks, const uint8_t* sigs, int fmt, int aug,
                                                                const uint8_t* msgs, const uint64_t* moffs, dst_arg dst, uint32_t* pairs,
                                                                int32_t* bad, uint32_t* sid, uint32_t* src, int two_lanes) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = (two_lanes & 1) ? gid >> 1 : gid;
  const int lane2 = (two_lanes & 1) ? (int)(gid & 1) : -1;
  if (i >= M) return;
  if (i >= T_b) {
    prepare_agg_item<SG>(true, sigs, bset[i - T_b], fmt, aug, nullptr, 0, dst, pairs, M, i, bad, two_lanes, lane2);
    return;
  }
  const uint32_t b = ragged_set_of(boffs, n_b, i);
  const size_t p = (size_t)agg_flat_pair(boffs, bsrc, b, i);
  if (lane2 <= 0) {
    sid[i] = b;
    src[i] = (uint32_t)p;
  }
  prepare_agg_item<SG>(false, pks, p, fmt, aug, msgs + moffs[p], (uint32_t)(moffs[p + 1] - moffs[p]), dst, pairs, M, i, bad, two_lanes, lane2);
}

#if BLS_TU_AGG_BATCH == 1
template __global__ void k_prepare_agg_seg<1>(size_t, size_t, size_t, const uint64_t*, const uint64_t*, const uint32_t*, const uint8_t*, const uint8_t*, int, int,
                                              const uint8_t*, const uint64_t*, dst_arg, uint32_t*, int32_t*, uint32_t*, uint32_t*, int);

__global__ void __launch_bounds__(BLS_BLOCK) k_first_bad_seg(size_t M, size_t T_b, const uint32_t* sid, const uint64_t* boffs, const int32_t* bad,
                                                          uint32_t* first, uint32_t* sig_id) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M) agg_first_bad_item(i, T_b, sid, boffs, bad, first, sig_id);
}
__global__ void __launch_bounds__(BLS_BLOCK) k_dup_insert_seg(size_t T_b, const uint8_t* msgs, const uint64_t* moffs, const uint32_t* sid,
                                                           const uint32_t* src, uint32_t mask, uint32_t* tab, uint32_t* minidx, uint32_t* slot_of) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < T_b) slot_of[i] = agg_dup_insert((uint32_t)i, msgs, moffs, sid, src, mask, tab, minidx);
}
__global__ void __launch_bounds__(BLS_BLOCK) k_dup_find_seg(size_t T_b, const uint32_t* sid, const uint64_t* boffs, const uint32_t* slot_of,
                                                         const uint32_t* minidx, uint32_t* best) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < T_b) agg_dup_find((uint32_t)i, sid, boffs, slot_of, minidx, best);
}
__global__ void __launch_bounds__(BLS_BLOCK) k_agg_flat_keys(size_t T_b, const uint32_t* src, const uint32_t* cidx, uint32_t* key_of) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < T_b) key_of[i] = agg_flat_key(src, cidx, i);
}
// what the rules decide for set b, and its aux
__device__ __forceinline__ int32_t agg_batch_decide(size_t b, const uint64_t* boffs, const uint32_t* best, const uint32_t* slot_of, const uint32_t* minidx,
                                                    const uint32_t* first, const uint32_t* sig_id, uint64_t aux[2]) {
  const uint32_t dup_i = best ? best[b] : AGG_NONE;
  const uint32_t dup_old = dup_i != AGG_NONE ? minidx[slot_of[boffs[b] + dup_i]] - (uint32_t)boffs[b] : AGG_NONE;
  return agg_decide(dup_old, dup_i, sig_id[b] != 0, first[b], aux);
}
// best == nullptr: no duplicate rule (MessageAugmentation, ProofOfPossession)
__global__ void __launch_bounds__(BLS_BLOCK) k_agg_batch_mark(size_t n_b, const uint64_t* boffs, const uint32_t* best, const uint32_t* slot_of,
                                                           const uint32_t* minidx, const uint32_t* first, const uint32_t* sig_id, int32_t* st_b) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_b) return;
  uint64_t a[2];
  st_b[b] = agg_batch_decide(b, boffs, best, slot_of, minidx, first, sig_id, a);
}
__global__ void __launch_bounds__(BLS_BLOCK) k_agg_batch_fin(size_t n_b, const uint64_t* boffs, const uint32_t* bset, const uint32_t* best,
                                                          const uint32_t* slot_of, const uint32_t* minidx, const uint32_t* first, const uint32_t* sig_id,
                                                          const int32_t* st_b, int32_t* status, uint64_t* aux) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_b) return;
  uint64_t a[2];
  const int32_t decided = agg_batch_decide(b, boffs, best, slot_of, minidx, first, sig_id, a);
  const size_t s = bset[b];
  status[s] = decided != BLS_OK ? decided : st_b[b];       // an undecided set: the final exponentiation's OK / INVALID_SIGNATURE
  if (aux) {
    aux[2 * s] = a[0];
    aux[2 * s + 1] = a[1];
  }
}
// first: the first identity key, n for the identity signature, -1 for none (k_first_bad_fin); dup2: (old, i) or (~0, ~0), null outside Basic
__global__ void __launch_bounds__(BLS_BLOCK) k_agg_large_fin(size_t n, const int64_t* first, const int32_t* verdict, const uint64_t* dup2, int32_t* status,
                                                          uint64_t* aux) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int64_t f = *first;
  const bool dup = dup2 && dup2[1] != ~0ull;
  uint64_t a[2];
  const int32_t decided = agg_decide(dup ? (uint32_t)dup2[0] : AGG_NONE, dup ? (uint32_t)dup2[1] : AGG_NONE, f == (int64_t)n,
                                     f >= 0 && f < (int64_t)n ? (uint32_t)f : AGG_NONE, a);
  *status = decided != BLS_OK ? decided : *verdict;
  if (aux) {
    aux[0] = a[0];
    aux[1] = a[1];
  }
}
#endif

#if BLS_TU_AGG_BATCH == 2
template __global__ void k_prepare_agg_seg<2>(size_t, size_t, size_t, const uint64_t*, const uint64_t*, const uint32_t*, const uint8_t*, const uint8_t*, int, int,
                                              const uint8_t*, const uint64_t*, dst_arg, uint32_t*, int32_t*, uint32_t*, uint32_t*, int);

// one lane per pair item, one product per lane as in k_f12_fold: item l of its set takes item l + half in (agg_fold_partner)
__global__ void __launch_bounds__(BLS_BLOCK) k_f12_fold_seg(size_t T_b, int r, const uint32_t* sid, const uint64_t* boffs, uint32_t* fws, size_t stride) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T_b) return;
  const uint64_t lo = boffs[sid[i]], len = boffs[sid[i] + 1] - lo;
  uint64_t partner;
  if (!agg_fold_partner(len, r, i - lo, &partner)) return;
  fp12 a, b;
  ws_ld_fp12(a, fws, stride, i);
  ws_ld_fp12(b, fws, stride, lo + partner);
  fp12_mul(a, a, b);
  ws_st_fp12(fws, stride, i, a);
}
// record b = (product of set b's pair values, at its first item; 1 for an empty set) * the value of its signature item
__global__ void __launch_bounds__(BLS_BLOCK) k_f12_fold_seg_out(size_t n_b, size_t T_b, const uint64_t* boffs, const uint32_t* fws, size_t stride,
                                                             uint32_t* rec) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_b) return;
  fp12 a, s;
  ws_ld_fp12(s, fws, stride, T_b + b);
  if (boffs[b + 1] != boffs[b]) {
    ws_ld_fp12(a, fws, stride, boffs[b]);
    fp12_mul(s, a, s);
  }
  ws_st_fp12(rec, n_b, b, s);
}
#endif
