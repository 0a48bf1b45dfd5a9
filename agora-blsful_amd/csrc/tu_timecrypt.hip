// translation unit: the pairing-value kernels of blsgpu_pairing_batch (timecrypt.cuh).  A unit of its own: the kernels of tu_coop.hip,
// tu_coop_keyed.hip and tu_coop_rows.hip stay what they are.
#define BLS_TU_TIMECRYPT
#include "kernels.cuh"
#include "timecrypt.cuh"

__global__ void __launch_bounds__(BLS_BLOCK) k_pairing_value_prepare(size_t n, const uint8_t* g1s, const uint8_t* g2s, int fmt, const int32_t* status,
                                                                     uint32_t* pairs, int32_t* flag) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (status && status[i] != BLS_OK) {
    flag[i] = PV_ZERO;
    return;
  }
  g1_jac a;
  g2_jac b;
  load_g1_pt(a, g1s, i, fmt);
  load_g2_pt(b, g2s, i, fmt);
  if (jac_is_inf(a) || jac_is_inf(b)) {
    flag[i] = PV_ONE;
    return;
  }
  flag[i] = PV_RUN;
  g1_aff P;
  g2_aff Q;
  g1g2_to_aff(P, Q, a, b);
  ws_st_pair(pairs, n, i, 0, P, Q);
}

// One workgroup (= one wave) per item.  LDS: the coop_shared of every one-wave pairing kernel and nothing else -- the export goes from
// registers to the output, twelve 32-bit words per lane of the six lane pairs that hold a coefficient.
__global__ void __launch_bounds__(BLS_BLOCK, 2) k_pairing_value(size_t n, size_t first, size_t count, const uint32_t* pairs, const int32_t* flag, uint8_t* out_gt) {
  __shared__ coop_shared S;
  if (blockIdx.x >= count) return;
  const size_t i = first + blockIdx.x;
  if (i >= n) return;
  uint8_t* out = out_gt + (size_t)GT_BYTES * i;
  const int fl = flag[i];                              // wave-uniform
  if (fl != PV_RUN) {
    coop_gt_const(out, fl == PV_ZERO);
    return;
  }
  g1_aff P;
  aff<hfp2> Q;
  ws_ld_fp(P.x, pairs, n, i, 0);
  ws_ld_fp(P.y, pairs, n, i, W1);
  ws_ld_fp(Q.x.v, pairs, n, i, W2 + (lane_hi() ? W1 : 0));
  ws_ld_fp(Q.y.v, pairs, n, i, 2 * W2 + (lane_hi() ? W1 : 0));
  P.inf = false;
  Q.inf = false;
  coop_miller1(S, P, Q);
  coop_final_value(S);
  coop_gt_bytes(out, S.t);
}

// ---- blsgpu_timecrypt_open_batch
template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK) k_timecrypt_prepare(size_t n, size_t n_groups, const uint64_t* item_offs, const uint8_t* us, const uint8_t* sigs, int fmt,
                                                                 const uint8_t* sig_schemes, const uint8_t* ct_schemes, const int32_t* dec_u, const int32_t* dec_sig,
                                                                 uint32_t* pairs, int32_t* flag, int32_t* status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  size_t lo = 0, hi = n_groups;                        // the last g with item_offs[g] <= i: i < item_offs[n_groups] = n, so g < n_groups
  while (hi - lo > 1) {
    const size_t mid = lo + (hi - lo) / 2;
    if (item_offs[mid] <= i) lo = mid;
    else hi = mid;
  }
  const size_t g = lo;
  int st = BLS_OK;
  if (dec_u && dec_u[i] != BLS_OK) st = dec_u[i];
  else if (dec_sig && dec_sig[g] != BLS_OK) st = dec_sig[g];
  else if (ct_schemes[i] != sig_schemes[g]) st = BLS_ERR_INVALID_SCHEME;
  flag[i] = PV_ZERO;
  if (st == BLS_OK) {
    typename grp<SG>::jac_t sig;
    typename grp<3 - SG>::jac_t u;
    grp<SG>::load(sig, sigs, g, fmt);
    grp<3 - SG>::load(u, us, i, fmt);
    if (jac_is_inf(sig)) st = BLS_ERR_SIG_IDENTITY;
    else if (jac_is_inf(u)) st = BLS_ERR_PK_IDENTITY;
    else {
      g1_aff P;
      g2_aff Q;
      if constexpr (SG == 1) g1g2_to_aff(P, Q, sig, u);
      else g1g2_to_aff(P, Q, u, sig);
      ws_st_pair(pairs, n, i, 0, P, Q);
      flag[i] = PV_RUN;
    }
  }
  status[i] = st;
}
template __global__ void k_timecrypt_prepare<1>(size_t, size_t, const uint64_t*, const uint8_t*, const uint8_t*, int, const uint8_t*, const uint8_t*, const int32_t*,
                                                const int32_t*, uint32_t*, int32_t*, int32_t*);
template __global__ void k_timecrypt_prepare<2>(size_t, size_t, const uint64_t*, const uint8_t*, const uint8_t*, int, const uint8_t*, const uint8_t*, const int32_t*,
                                                const int32_t*, uint32_t*, int32_t*, int32_t*);

template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK) k_timecrypt_open(size_t n, const uint8_t* gt, const uint8_t* us, int fmt, const uint8_t* vs, const uint8_t* ws,
                                                              const uint64_t* w_offs, uint8_t* frames, uint64_t* pt_range, int32_t* status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t off = 0, plen = 0;
  int st = status[i];
  if (st == BLS_OK) {
    const uint64_t lo = w_offs[i], len = w_offs[i + 1] - lo;
    uint32_t r[8];
    st = timecrypt_open_frame(frames + lo, ws + lo, len, gt + (size_t)GT_BYTES * i, vs + 32 * i, &off, &plen, r);   // the lane reads back its own stores
    if (st == BLS_OK) {
      typedef grp<3 - SG> KG;                          // the key group: u = g r there
      typename KG::jac_t u;
      typename KG::aff_t ga;
      KG::load(u, us, i, fmt);
      if constexpr (SG == 1) {
        fp2_load(ga.x, G2_GEN_X);
        fp2_load(ga.y, G2_GEN_Y);
      } else {
        fp_load(ga.x, G1_GEN_X);
        fp_load(ga.y, G1_GEN_Y);
      }
      ga.inf = false;
      if (!timecrypt_check<3 - SG>(ga, r, u)) st = BLS_ERR_INVALID_SIGNATURE;
    }
    status[i] = st;
  }
  if (st != BLS_OK) off = plen = 0;
  pt_range[2 * i] = off;
  pt_range[2 * i + 1] = plen;
}
template __global__ void k_timecrypt_open<1>(size_t, const uint8_t*, const uint8_t*, int, const uint8_t*, const uint8_t*, const uint64_t*, uint8_t*, uint64_t*, int32_t*);
template __global__ void k_timecrypt_open<2>(size_t, const uint8_t*, const uint8_t*, int, const uint8_t*, const uint8_t*, const uint64_t*, uint8_t*, uint64_t*, int32_t*);
