// Kernels of the threshold recovery (blsgpu_combine_shares, shares.cuh), included by tu_shares1.hip (BLS_TU_SHARES = 1: the
// coefficients and the G1 instances) and tu_shares2.hip (BLS_TU_SHARES = 2: the G2 instances).
//   k_share_lagrange : partial products of lambda_i's numerator and denominator, the share -> set map, the duplicate flags
//   k_share_lagrange_fin : lambda_i (one inversion per share) and the share's own error flags
//   k_share_ladder   : lambda_i P_i, one joint NAF ladder per share over the endomorphism split (shares.cuh share_ladder)
//   k_share_fold     : one level of a segmented pairwise tree sum inside every set (complete additions); ceil(log2 t_max) levels
//   k_share_out      : per set: the status, and the sum with Z = 1 (all-zero for the identity or a failed set)
#include "kernels.cuh"
#include "shares.cuh"

#if BLS_TU_SHARES == 1
// The lanes of a workgroup are consecutive shares of one or more sets, so the identifiers they need are ONE contiguous range
// [offs[first set], offs[last set + 1]): the workgroup streams it through LDS in tiles of BLS_BLOCK identifiers (each converted to
// Montgomery form once, by the lane that loads it), and every lane multiplies in those of its own set -- the n-body pattern:
// t products per lane for a set of t shares, whatever the mix of set sizes in the workgroup.  A large set would leave too few
// lanes busy for too long, so the range is split over gridDim.y workgroups (tile k goes to y = k mod gridDim.y), each leaving
// partial products in nd (16 words per (y, share)); k_share_lagrange_fin multiplies them and inverts.
__global__ void __launch_bounds__(BLS_BLOCK) k_share_lagrange(size_t n, const uint64_t* offs, size_t n_sets, const uint8_t* ids,
                                                            uint32_t* flags, uint32_t* nd, uint32_t* sid) {
  __shared__ fr tile[BLS_BLOCK];
  const size_t b0 = (size_t)blockIdx.x * BLS_BLOCK, i = b0 + threadIdx.x, S = gridDim.y;
  const size_t blast = b0 + BLS_BLOCK - 1 < n ? b0 + BLS_BLOCK - 1 : n - 1;
  const size_t range_lo = offs[ragged_set_of(offs, n_sets, b0)], range_hi = offs[ragged_set_of(offs, n_sets, blast) + 1];
  const bool live = i < n;
  uint32_t s = 0;
  size_t lo = 0, hi = 0;
  fr xi;
  share_lagrange L;
  share_lagrange_init(L);
  if (live) {
    s = ragged_set_of(offs, n_sets, i);
    lo = offs[s];
    hi = offs[s + 1];
    fr_to_mont(xi, (const uint32_t*)(ids + 32 * i));
    if (blockIdx.y == 0) sid[i] = s;
  }
  for (size_t t0 = range_lo + (size_t)blockIdx.y * BLS_BLOCK; t0 < range_hi; t0 += S * BLS_BLOCK) {
    const size_t j = t0 + threadIdx.x;
    if (j < range_hi) fr_to_mont(tile[threadIdx.x], (const uint32_t*)(ids + 32 * j));
    __syncthreads();
    if (live) {
      const size_t a = t0 > lo ? t0 : lo, e0 = t0 + BLS_BLOCK < hi ? t0 + BLS_BLOCK : hi;
      for (size_t j2 = a; j2 < e0; j2++)
        if (j2 != i) share_lagrange_acc(L, xi, tile[j2 - t0]);
    }
    __syncthreads();
  }
  if (!live) return;
  uint32_t* o = nd + ((size_t)blockIdx.y * n + i) * 16;
  for (int k = 0; k < 8; k++) {
    o[k] = L.num.w[k];
    o[8 + k] = L.den.w[k];
  }
  if (L.dup) atomicOr(&flags[s], SHARE_F_VSSS);
}
// the S partial products of share i -> lambda_i (canonical bytes); the share's own checks: encoding, scheme tag, zero identifier
__global__ void __launch_bounds__(BLS_BLOCK) k_share_lagrange_fin(size_t n, int S, const uint64_t* offs, const uint8_t* ids, const uint8_t* schemes,
                                                                const uint32_t* nd, const uint32_t* sid, uint32_t* flags, uint8_t* lam) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = sid[i];
  uint32_t v[8];
  for (int k = 0; k < 8; k++) v[k] = ((const uint32_t*)(ids + 32 * i))[k];
  uint32_t f = fr_words_canonical(v) ? 0u : SHARE_F_ENCODING;
  if (schemes && schemes[i] != schemes[offs[s]]) f |= SHARE_F_SCHEME;
  fr xi;
  fr_to_mont(xi, v);
  share_lagrange L;
  share_lagrange_init(L);
  for (int y = 0; y < S; y++) {
    const uint32_t* p = nd + ((size_t)y * n + i) * 16;
    fr a, b;
    for (int k = 0; k < 8; k++) {
      a.w[k] = p[k];
      b.w[k] = p[8 + k];
    }
    fr_mul(L.num, L.num, a);
    fr_mul(L.den, L.den, b);
  }
  uint32_t l[8];
  f |= share_lagrange_fin(l, L, xi);
  uint32_t* lw = (uint32_t*)(lam + 32 * i);
  for (int k = 0; k < 8; k++) lw[k] = l[k];
  if (f) atomicOr(&flags[s], f);
}
#endif

template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_share_ladder(size_t n, const uint8_t* pts, int fmt, const uint8_t* lam, const uint32_t* sid,
                                                          const uint32_t* flags, uint8_t* part) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  typedef typename grp<G>::F F;
  jac<F> p, acc;
  jac_set_inf(acc);
  if (!flags[sid[i]]) {            // a failed set's output is the identity, a large set runs as one MSM: no work here
    grp<G>::load(p, pts, i, fmt);
    if (!jac_is_inf(p)) {
      aff<F> a;
      jac_to_aff(a, p);
      share_ladder<G>(acc, a, (const uint32_t*)(lam + 32 * i));
    }
  }
  grp<G>::store(part, i, acc);
}
// level `step` (1, 2, 4, ...): the share at local index k (k a multiple of 2 step) adds in the one at k + step, if its set has it
template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_share_fold(size_t n, uint64_t step, const uint64_t* offs, const uint32_t* sid, uint8_t* part) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = sid[i];
  if (!share_fold_adds(i, step, offs[s], offs[s + 1])) return;
  typedef typename grp<G>::F F;
  jac<F> a, b;
  grp<G>::load(a, part, i, 0);
  grp<G>::load(b, part, i + step, 0);
  jac_add(a, a, b);
  grp<G>::store(part, i, a);
}
template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_share_out(size_t n_sets, const uint64_t* offs, const uint32_t* flags, const uint8_t* part,
                                                       uint8_t* out, int32_t* status) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_sets) return;
  const uint32_t f = flags[s];
  const uint64_t lo = offs[s], cnt = offs[s + 1] - lo;
  int32_t st = BLS_OK;
  if (f & SHARE_F_ENCODING) st = BLS_ERR_BAD_ENCODING;
  else if (f & SHARE_F_SCHEME) st = BLS_ERR_INVALID_SCHEME;
  else if ((f & SHARE_F_VSSS) || cnt < 2) st = BLS_ERR_VSSS;
  status[s] = st;
  typedef typename grp<G>::F F;
  jac<F> p;
  bool zero = st != BLS_OK;
  if (!zero) {
    grp<G>::load(p, part, lo, 0);
    zero = jac_is_inf(p);
  }
  uint32_t* w = (uint32_t*)(out + s * grp<G>::PROJ_BYTES);
  if (zero) {                      // the identity leaves as all-zero bytes: they depend on the group element only
    for (int k = 0; k < grp<G>::PROJ_BYTES / 4; k++) w[k] = 0;
    return;
  }
  F zi, zi2;
  fe_inv(zi, p.z);
  fe_sqr(zi2, zi);
  fe_mul(p.x, p.x, zi2);
  fe_mul(zi2, zi2, zi);
  fe_mul(p.y, p.y, zi2);
  fe_one(p.z);
  grp<G>::store(out, s, p);
}

template __global__ void k_share_ladder<BLS_TU_SHARES>(size_t, const uint8_t*, int, const uint8_t*, const uint32_t*, const uint32_t*, uint8_t*);
template __global__ void k_share_fold<BLS_TU_SHARES>(size_t, uint64_t, const uint64_t*, const uint32_t*, uint8_t*);
template __global__ void k_share_out<BLS_TU_SHARES>(size_t, const uint64_t*, const uint32_t*, const uint8_t*, uint8_t*, int32_t*);
