// translation unit: the kernels of the registered signature sets (sigset.cuh) -- seal, prepare, and k_pairing_value_rows, the one-wave
// pairing value that reads a registered signature's line rows (coop_row1.cuh).  A unit of its own: the kernels of tu_coop.hip,
// tu_coop_keyed.hip, tu_coop_rows.hip and tu_timecrypt.hip stay what they are.
#define BLS_TU_TIMECRYPT               // the engine part of timecrypt.cuh: coop_gt_bytes, coop_gt_const
#include "kernels.cuh"
#include "timecrypt.cuh"
#include "coop_row1.cuh"
#include "sigset.cuh"

template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK) k_sigset_seal(size_t cnt, const uint8_t* pts, int fmt, const int32_t* dec, size_t first, uint8_t* recs, int32_t* est) {
  const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= cnt) return;
  const size_t k = first + l;
  const int st = dec ? dec[l] : BLS_OK;
  est[k] = st;
  uint32_t* w = (uint32_t*)(recs + k * (size_t)(96 * SG));
  if (st != BLS_OK) {                       // a point that did not decode is never read
    for (int j = 0; j < 24 * SG; j++) w[j] = 0u;
    return;
  }
  typedef grp<SG> HG;
  typename HG::jac_t h;
  typename HG::aff_t a;
  HG::load(h, pts, l, fmt);
  jac_to_aff(a, h);                         // the identity: zero coordinates, which the RAW_AFFINE reader takes for the identity again
  if constexpr (SG == 1) {
    fp_to_raw(w, a.x);
    fp_to_raw(w + 12, a.y);
  } else {
    fp2_to_raw(w, a.x);
    fp2_to_raw(w + 24, a.y);
  }
}
template __global__ void k_sigset_seal<1>(size_t, const uint8_t*, int, const int32_t*, size_t, uint8_t*, int32_t*);
template __global__ void k_sigset_seal<2>(size_t, const uint8_t*, int, const int32_t*, size_t, uint8_t*, int32_t*);

template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK) k_sigset_prepare(size_t n, const uint32_t* idx, uint64_t n_entries, const uint8_t* recs, const uint8_t* tags,
                                                              const int32_t* est, const int32_t* nolines, const uint8_t* pts, int fmt, const int32_t* dec_pt,
                                                              const uint8_t* ct_schemes, uint32_t* pairs, int32_t* flag, int32_t* status, uint32_t* ent,
                                                              uint32_t* walk) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = idx[i];
  ent[i] = 0u;
  if (k >= n_entries) {                     // nothing outside the set is read
    status[i] = SIGSET_E_ARG;
    flag[i] = PV_ZERO;
    return;
  }
  if (nolines && nolines[k] != 0) atomicOr(walk, 1u);
  const int du = dec_pt ? dec_pt[i] : BLS_OK, ds = est[k];
  int st = BLS_OK, fl = PV_ZERO;
  if (ct_schemes) {
    if (du != BLS_OK) st = du;
    else if (ds != BLS_OK) st = ds;
    else if (ct_schemes[i] != tags[k]) st = BLS_ERR_INVALID_SCHEME;
  } else {                                  // the G1 member's status first: the signature under Bls12381G1Impl, the point under Bls12381G2Impl
    const int d1 = SG == 1 ? ds : du, d2 = SG == 1 ? du : ds;
    st = d1 != BLS_OK ? d1 : d2;
  }
  if (st == BLS_OK) {
    typename grp<SG>::jac_t sig;
    typename grp<3 - SG>::jac_t u;
    grp<SG>::load(sig, recs, k, 1);         // the stored RAW_AFFINE record
    grp<3 - SG>::load(u, pts, i, fmt);
    const bool si = jac_is_inf(sig), ui = jac_is_inf(u);
    if (si || ui) {
      if (ct_schemes) st = si ? BLS_ERR_SIG_IDENTITY : BLS_ERR_PK_IDENTITY;
      else fl = PV_ONE;
    } else {
      g1_aff P;
      g2_aff Q;
      if constexpr (SG == 1) g1g2_to_aff(P, Q, sig, u);
      else g1g2_to_aff(P, Q, u, sig);
      ws_st_pair(pairs, n, i, 0, P, Q);
      ent[i] = (uint32_t)k;
      fl = PV_RUN;
    }
  }
  flag[i] = fl;
  status[i] = st;
}
template __global__ void k_sigset_prepare<1>(size_t, const uint32_t*, uint64_t, const uint8_t*, const uint8_t*, const int32_t*, const int32_t*, const uint8_t*, int,
                                             const int32_t*, const uint8_t*, uint32_t*, int32_t*, int32_t*, uint32_t*, uint32_t*);
template __global__ void k_sigset_prepare<2>(size_t, const uint32_t*, uint64_t, const uint8_t*, const uint8_t*, const int32_t*, const int32_t*, const uint8_t*, int,
                                             const int32_t*, const uint8_t*, uint32_t*, int32_t*, int32_t*, uint32_t*, uint32_t*);

// One workgroup (= one wave) per item.  LDS: the coop_shared of every one-wave pairing kernel and nothing else.
__global__ void __launch_bounds__(BLS_BLOCK, 2) k_pairing_value_rows(size_t n, size_t first, size_t count, const uint32_t* pairs, const int32_t* flag,
                                                                     const uint32_t* table, const uint32_t* ent, uint8_t* out_gt) {
  __shared__ coop_shared S;
  if (blockIdx.x >= count) return;
  const size_t i = first + blockIdx.x;
  if (i >= n) return;
  uint8_t* out = out_gt + (size_t)GT_BYTES * i;
  const int fl = flag[i];                              // wave-uniform
  if (fl != PV_RUN) {                                  // before any table read
    coop_gt_const(out, fl == PV_ZERO);
    return;
  }
  g1_aff P;
  ws_ld_fp(P.x, pairs, n, i, 0);
  ws_ld_fp(P.y, pairs, n, i, W1);
  P.inf = false;
  const uint32_t eoff = ent[i] * (uint32_t)(MILLER_ENTRIES * 4 * FP_NL);
  coop_miller1_rows(S, P, table + eoff);
  coop_final_value(S);
  coop_gt_bytes(out, S.t);
}
