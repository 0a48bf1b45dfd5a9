// Kernels of the aggregate verify by message index (blsgpu_aggregate_verify_msgset_batch / _indexed_batch, agg_msgset.cuh), included
// by tu_agg_msgset1.hip (BLS_TU_AGG_MSGSET = 1: the group-independent kernels and Bls12381G1Impl) and tu_agg_msgset2.hip
// (BLS_TU_AGG_MSGSET = 2: Bls12381G2Impl).  Between k_aggm_items and k_aggm_mark run k_linesp / k_linesp_keyed, k_millerfp3 and the
// segmented product of agg_batch.cuh over the class items; the prefix sums between the numbering kernels are k_scan_* (util_kernels.cuh).
// No kernel here waits for another workgroup: every dependency is a launch boundary.
//   k_aggm_check   : every pair's set and sanitised entry; the sets that name no entry; whether every named entry has rows
//   k_aggm_insert  : the class table keyed by (set, entry); the first identity key per set
//   k_aggm_reps / k_aggm_number / k_aggm_offsets / k_aggm_widen / k_aggm_scatter : classes numbered set after set, members in class order
//   k_aggm_sum     : every strip's sum of its class members' keys (the strip sum of multi_batch.cuh with a gather)
//   k_aggm_items   : class items and signature items in k_prepare_agg_seg's layout
//   k_aggm_mark / k_aggm_fin : BLSGPU_E_ARG for a set that names no entry, on top of every other rule
#include "kernels.cuh"
#include "agg_msgset.cuh"

template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK) k_aggm_insert(size_t T, int by_record, const uint32_t* cmsg, const uint32_t* sid, const uint32_t* recs, uint32_t mask,
                                                         uint32_t* tab, uint32_t* minidx, uint32_t* slot_of, const uint8_t* pks, int fmt, const uint64_t* offs,
                                                         uint32_t* first) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T) return;
  slot_of[i] = aggm_class_insert((uint32_t)i, by_record != 0, cmsg, sid, recs, (size_t)(24 * SG), mask, tab, minidx);
  typename grp<3 - SG>::jac_t pk;
  grp<3 - SG>::load(pk, pks, i, fmt);
  if (jac_is_inf(pk)) atomicMin(&first[sid[i]], (uint32_t)(i - offs[sid[i]]));
}
template __global__ void k_aggm_insert<BLS_TU_AGG_MSGSET>(size_t, int, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*,
                                                          const uint8_t*, int, const uint64_t*, uint32_t*);

template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK) k_aggm_items(size_t M, size_t C, const uint32_t* csid, const uint32_t* cent, const uint32_t* crep,
                                                        const uint32_t* skipped, const uint32_t* first, const uint32_t* best, const uint8_t* pks, int fmt,
                                                        const uint8_t* part, const uint64_t* strip_offs, const uint8_t* recs, const uint8_t* sigs,
                                                        uint32_t* pairs, int32_t* bad, uint32_t* sig_id) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  g1_aff P;
  g2_aff Q;
  if (i >= C) {  // the signature item of set i - C, as prepare_agg_item makes it (Bls12381G1Impl: against -[c] g2, the entries are uncleared)
    const size_t b = i - C;
    typename grp<SG>::jac_t s;
    grp<SG>::load(s, sigs, b, fmt);
    const bool inf = jac_is_inf(s);
    bad[i] = inf ? 1 : 0;
    sig_id[b] = inf ? 1u : 0u;
    if (inf) return;
    if constexpr (SG == 1) {
      jac_to_aff(P, s);
      g2_negc_gen(Q);
    } else {
      jac_to_aff(Q, s);
      g1_neg_gen(P);
    }
    ws_st_pair(pairs, M, i, 0, P, Q);
    return;
  }
  bad[i] = 1;
  if (aggm_set_decided(csid[i], skipped, first, best)) return;       // before any read by entry: a skipped pair's class has none
  typename grp<3 - SG>::jac_t pk;
  typename grp<SG>::jac_t h;
  if (part) grp<3 - SG>::load(pk, part, (size_t)strip_offs[i], 0);   // a class's sum, at its first strip: RAW_PROJ
  else grp<3 - SG>::load(pk, pks, crep[i], fmt);
  grp<SG>::load(h, recs, cent[i], 1);                                // a stored entry: RAW_AFFINE
  if (jac_is_inf(pk) || jac_is_inf(h)) return;                       // the factor is 1 (P and -P in one class; no hash output is the identity in practice)
  if constexpr (SG == 1) g1g2_to_aff(P, Q, h, pk);
  else g1g2_to_aff(P, Q, pk, h);
  bad[i] = 0;
  ws_st_pair(pairs, M, i, 0, P, Q);
}
template __global__ void k_aggm_items<BLS_TU_AGG_MSGSET>(size_t, size_t, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*,
                                                         const uint32_t*, const uint8_t*, int, const uint8_t*, const uint64_t*, const uint8_t*, const uint8_t*,
                                                         uint32_t*, int32_t*, uint32_t*);

#if BLS_TU_AGG_MSGSET == 1
__global__ void __launch_bounds__(BLS_BLOCK) k_aggm_check(size_t T, size_t n_sets, const uint64_t* offs, const uint32_t* msg_idx, uint64_t n_msgs,
                                                        const int32_t* nolines, uint32_t* cmsg, uint32_t* sid, uint32_t* skipped, uint32_t* walk) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T) return;
  const uint32_t b = ragged_set_of(offs, n_sets, i), k = msgset_entry_of(msg_idx[i], n_msgs);
  sid[i] = b;
  cmsg[i] = k;
  if (k == MSGSET_SKIP) skipped[b] = 1u;
  else if (nolines && nolines[k] != 0) atomicOr(walk, 1u);          // nothing outside the set is read
}
__global__ void __launch_bounds__(BLS_BLOCK) k_aggm_reps(size_t T, const uint32_t* slot_of, const uint32_t* tab, uint32_t* is_rep) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= T) is_rep[i] = i < T ? aggm_is_rep((uint32_t)i, slot_of, tab) : 0u;
}
__global__ void __launch_bounds__(BLS_BLOCK) k_aggm_number(size_t T, const uint32_t* slot_of, const uint32_t* tab, const uint32_t* rank, const uint32_t* sid,
                                                         const uint32_t* cmsg, uint32_t* cid, uint32_t* csid, uint32_t* cent, uint32_t* crep, uint32_t* count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T) return;
  const uint32_t c = aggm_class_of((uint32_t)i, slot_of, tab, rank);
  cid[i] = c;
  atomicAdd(&count[c], 1u);
  if (aggm_is_rep((uint32_t)i, slot_of, tab)) {
    csid[c] = sid[i];
    cent[c] = cmsg[i];
    crep[c] = (uint32_t)i;
  }
}
__global__ void __launch_bounds__(BLS_BLOCK) k_aggm_offsets(size_t n_sets, const uint64_t* offs, const uint32_t* rank, uint64_t* coffs) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b <= n_sets) coffs[b] = aggm_class_offset(offs, rank, b);
}
__global__ void __launch_bounds__(BLS_BLOCK) k_aggm_widen(size_t n, const uint32_t* in, uint64_t* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i];
}
__global__ void __launch_bounds__(BLS_BLOCK) k_aggm_scatter(size_t T, const uint32_t* cid, const uint64_t* moffs, uint32_t* cursor, uint32_t* perm) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < T) aggm_scatter((uint32_t)i, cid, moffs, cursor, perm);
}
__global__ void __launch_bounds__(BLS_BLOCK) k_aggm_mark(size_t n_sets, const uint32_t* skipped, int32_t* st_b) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n_sets && skipped[b] != 0) st_b[b] = MSGSET_E_ARG;
}
__global__ void __launch_bounds__(BLS_BLOCK) k_aggm_fin(size_t n_sets, const uint32_t* skipped, int32_t* status, uint64_t* aux) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_sets) return;
  uint64_t a[2];
  if (aggm_top(skipped[b] != 0, &status[b], a) && aux) {
    aux[2 * b] = a[0];
    aux[2 * b + 1] = a[1];
  }
}

// Bls12381G1Impl: keys in G2, one lane pair per strip on the lane-split tower, as k_multi_accumulate_seg<2>
template <>
__global__ void __launch_bounds__(BLS_BLOCK, 2) k_aggm_sum<2>(size_t n_strips, const uint8_t* pts, int fmt, const uint32_t* perm, const uint64_t* moffs,
                                                            const uint64_t* strip_offs, const uint32_t* strip_cid, uint8_t* part) {
  const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (g >= n_strips) return;
  const multi_strip st = aggm_strip_of(g, moffs, strip_offs, strip_cid);
  jac<hfp2> acc, p;
  hfp2 one, d;
  fe_one(one);
  jac_set_inf(acc);
  for (uint64_t k = st.first; k < st.end; k += st.stride) {
    ld_g2s_fmt(p, pts, perm[k], fmt);
    fe_sub(d, p.z, one);
    if (fe_is_zero(d)) jac_madd_body(acc, acc, p.x, p.y);
    else jac_add_body(acc, acc, p);
  }
  st_g2s(part, g, acc);
}
#else
// Bls12381G2Impl: keys in G1, one lane per strip, as k_multi_accumulate_seg<1>
template <>
__global__ void __launch_bounds__(BLS_BLOCK) k_aggm_sum<1>(size_t n_strips, const uint8_t* pts, int fmt, const uint32_t* perm, const uint64_t* moffs,
                                                         const uint64_t* strip_offs, const uint32_t* strip_cid, uint8_t* part) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_strips) return;
  const multi_strip st = aggm_strip_of(g, moffs, strip_offs, strip_cid);
  g1_jac acc, p;
  fp one;
  fp_one(one);
  jac_set_inf(acc);
  for (uint64_t k = st.first; k < st.end; k += st.stride) {
    load_g1_pt(p, pts, perm[k], fmt);
    if (fp_eq(p.z, one)) jac_madd(acc, acc, p.x, p.y);
    else jac_add(acc, acc, p);
  }
  store_g1_pt(part, g, acc);
}
#endif
