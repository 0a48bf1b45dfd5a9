// Kernels of the batched verify_secure (blsgpu_verify_secure_batch, secure.cuh), included by tu_secure1.hip (BLS_TU_SECURE = 1:
// the sort and the hashes) and tu_secure2.hip (BLS_TU_SECURE = 2: the point kernels).  Only the sets below
// BLSGPU_SECURE_BATCH_MAX keys run here (SECURE_F_LARGE clear); the key sum between k_secure_coeff and k_set_out is
// k_share_ladder / k_share_fold of the threshold recovery (tu_shares.inc).
//   k_secure_rank   : the key's position in its set under the stable byte-lexicographic order (reference src/secure_aggregation.rs:41-42)
//   k_secure_gather : every set's keys as one contiguous sorted stream
//   k_secure_digest : H_s = SHA-256 of set s's stream (:45-49), one wave per set
//   k_secure_coeff  : t = SHA-256(BE32(position) || H_s) mod r into the key's input slot (:61-100); a zero flags the set
//   k_set_out       : the signature as RAW_PROJ, the set's summed key, the status the verification tail starts from; shared
//                     with the batched multi verify (no flags there: status BLS_OK)
//   k_secure_fin    : after the tail, the verdict of the empty sets (:189-195)
// and of the batched aggregation (blsgpu_aggregate_secure_batch, blsgpu_sum_batch):
//   k_secure_first  : the first input position of the key's set that holds the same bytes (reference :138-147)
//   k_secure_ladder : t_i sig[first_i] in the signature group, one joint NAF ladder per key (shares.cuh share_ladder)
//   k_set_sum_out   : the set's sum (after k_share_fold) and its status to the caller's arrays
#include "kernels.cuh"
#include "secure.cuh"
#if BLS_TU_SECURE == 2
#include "shares.cuh"
#endif

#if BLS_TU_SECURE == 1
// key o sorts before key m: its big-endian words are smaller, or they are equal and o comes first in the input (tie)
template <int WPK>
__device__ __forceinline__ bool secure_key_less(const uint32_t* o, const uint32_t (&m)[WPK], bool tie) {
#pragma unroll
  for (int k = 0; k < WPK; k++)
    if (o[k] != m[k]) return o[k] < m[k];
  return tie;
}
// rank_i = #{ j in i's set : bytes_j < bytes_i, or bytes_j == bytes_i and j < i }: Rust's stable sort_by on to_bytes(), duplicates
// included.  The n-body pattern of k_share_lagrange: the lanes of a workgroup are consecutive keys, the keys their sets hold are
// one contiguous range, streamed through LDS in tiles of BLS_BLOCK keys (as big-endian words, converted once by the lane that
// loads them); every lane compares its own key with those of its set.  A large range is split over gridDim.y workgroups (tile
// k goes to y = k mod gridDim.y), whose counts meet in rank (zeroed by the caller) by atomicAdd.
template <int WPK>
__global__ void __launch_bounds__(BLS_BLOCK) k_secure_rank(size_t n, const uint64_t* offs, size_t n_sets, const uint8_t* kb, const uint32_t* flags,
                                                         uint32_t* rank, uint32_t* sid) {
  __shared__ uint32_t tile[BLS_BLOCK * WPK];
  __shared__ unsigned long long range_lo, range_hi;
  const size_t i = (size_t)blockIdx.x * BLS_BLOCK + threadIdx.x, S = gridDim.y;
  const uint32_t* kw = (const uint32_t*)kb;
  bool live = i < n;
  size_t lo = 0, hi = 0;
  uint32_t me[WPK];
  if (threadIdx.x == 0) {
    range_lo = ~0ull;
    range_hi = 0;
  }
  __syncthreads();
  if (live) {
    const uint32_t s = ragged_set_of(offs, n_sets, i);
    if (blockIdx.y == 0) sid[i] = s;
    live = !(flags[s] & SECURE_F_LARGE);
    lo = offs[s];
    hi = offs[s + 1];
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < WPK; k++) me[k] = __builtin_bswap32(kw[i * WPK + k]);
    atomicMin(&range_lo, (unsigned long long)lo);
    atomicMax(&range_hi, (unsigned long long)hi);
  }
  __syncthreads();
  const size_t rlo = range_lo, rhi = range_hi;
  if (rlo >= rhi) return;                     // no key of a small set here (uniform over the workgroup)
  uint32_t cnt = 0;
  for (size_t t0 = rlo + (size_t)blockIdx.y * BLS_BLOCK; t0 < rhi; t0 += S * BLS_BLOCK) {
    const size_t j = t0 + threadIdx.x;
    if (j < rhi) {
#pragma unroll
      for (int k = 0; k < WPK; k++) tile[threadIdx.x * WPK + k] = __builtin_bswap32(kw[j * WPK + k]);
    }
    __syncthreads();
    if (live) {
      const size_t a = t0 > lo ? t0 : lo, e = t0 + BLS_BLOCK < hi ? t0 + BLS_BLOCK : hi;
      for (size_t j2 = a; j2 < e; j2++)
        if (j2 != i && secure_key_less<WPK>(tile + (j2 - t0) * WPK, me, j2 < i)) cnt++;
    }
    __syncthreads();
  }
  if (live && cnt) atomicAdd(&rank[i], cnt);
}
// the keys of every small set at their sorted positions: sorted[offs[s] + rank_i] = key i, one 32-bit word per lane
__global__ void __launch_bounds__(BLS_BLOCK) k_secure_gather(size_t n, size_t width, const uint64_t* offs, const uint8_t* kb, const uint32_t* rank,
                                                           const uint32_t* sid, const uint32_t* flags, uint8_t* sorted) {
  const size_t wpk = width / 4, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * wpk) return;
  const size_t i = t / wpk, w = t % wpk;
  const uint32_t s = sid[i];
  if (flags[s] & SECURE_F_LARGE) return;
  ((uint32_t*)sorted)[(offs[s] + rank[i]) * wpk + w] = ((const uint32_t*)kb)[t];
}
// H_s = SHA-256(set s's sorted stream): one wave per set walks the stream block by block (the pieces of kernels.cuh expand_message_xmd_wave: lane
// L fetches byte L of the block, the block meets in LDS, every lane runs the compression on registers).  Sequential within a
// set, parallel across sets.  H leaves as 32 big-endian bytes.
__global__ void __launch_bounds__(BLS_BLOCK) k_secure_digest(size_t n_sets, size_t width, const uint64_t* offs, const uint8_t* sorted,
                                                           const uint32_t* flags, uint8_t* H) {
  __shared__ uint32_t blkw[16];
  uint8_t* blk = (uint8_t*)blkw;
  const size_t s = blockIdx.x;
  const uint32_t L = threadIdx.x & 63u;
  if (s >= n_sets) return;
  const uint64_t lo = offs[s], cnt = offs[s + 1] - lo;
  if (cnt == 0 || (flags[s] & SECURE_F_LARGE)) return;
  const uint8_t* m = sorted + lo * width;
  const uint64_t len = cnt * width, bits = len * 8;
  const uint64_t nblk = (len + 9 + 63) >> 6;
  u32x8_t h = sha256_iv();
  for (uint64_t b = 0; b < nblk; b++) {
    const uint64_t pos = b * 64 + L;
    uint32_t byte = 0;
    if (pos < len) byte = m[pos];
    else if (pos == len) byte = 0x80;
    else if (b == nblk - 1 && L >= 56) byte = (uint32_t)(bits >> (8 * (63 - L))) & 255u;
    blk[L] = (uint8_t)byte;
    h = sha256_compress_v(h, sha256_block_from_lds(blk));
  }
  if (L < 8) {
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) v = (uint32_t)j == L ? h[j] : v;
    ((uint32_t*)(H + 32 * s))[L] = __builtin_bswap32(v);
  }
}
// k_sha256_coeff's coefficient (sha256_coeff_mod_r), per set: the key's sorted position within its set and that set's H; the scalar goes to the key's INPUT
// slot, so the key sum needs no permutation
__global__ void __launch_bounds__(BLS_BLOCK) k_secure_coeff(size_t n, const uint32_t* rank, const uint32_t* sid, const uint8_t* H, uint32_t* flags,
                                                          uint8_t* scal) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = sid[i];
  if (flags[s] & SECURE_F_LARGE) return;
  const uint32_t* hw = (const uint32_t*)(H + 32 * (size_t)s);
  uint32_t hb[8], v[8];
#pragma unroll
  for (int k = 0; k < 8; k++) hb[k] = __builtin_bswap32(hw[k]);
  const bool nz = sha256_coeff_mod_r(v, rank[i], hb);
  uint32_t* o = (uint32_t*)(scal + 32 * i);
#pragma unroll
  for (int k = 0; k < 8; k++) o[k] = v[k];
  if (!nz) atomicOr(&flags[s], SECURE_F_ZERO);
}
// an empty set is Ok iff its signature is the identity (reference :189-195); the tail skipped it
__global__ void __launch_bounds__(BLS_BLOCK) k_secure_fin(size_t n_sets, const uint64_t* offs, const uint32_t* flags, int32_t* status) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_sets || offs[s + 1] != offs[s]) return;
  status[s] = (flags[s] & SECURE_F_IDSIG) ? BLS_OK : BLS_ERR_INVALID_SIGNATURE;
}
// first_i = min{ j in i's set : bytes_j == bytes_i } as a flat index.  The tile walk of k_secure_rank: the lanes of a workgroup are
// consecutive keys, the keys before them in their sets are one contiguous range [range_lo, range_hi), streamed through LDS in
// tiles of BLS_BLOCK keys; every lane searches the tiles of its own set below its own index (secure_first_tile).  gridDim.y
// workgroups share the tiles of a long range (tile k goes to y = k mod gridDim.y) and meet in first (preset to ~0) by atomicMin.
template <int WPK>
__global__ void __launch_bounds__(BLS_BLOCK) k_secure_first(size_t n, const uint64_t* offs, const uint8_t* kb, const uint32_t* sid,
                                                          const uint32_t* flags, uint32_t* first) {
  __shared__ uint32_t tile[BLS_BLOCK * WPK];
  __shared__ unsigned long long range_lo, range_hi;
  const size_t i = (size_t)blockIdx.x * BLS_BLOCK + threadIdx.x, S = gridDim.y;
  const uint32_t* kw = (const uint32_t*)kb;
  bool live = i < n;
  size_t lo = 0;
  uint32_t me[WPK];
  if (threadIdx.x == 0) {
    range_lo = ~0ull;
    range_hi = 0;
  }
  __syncthreads();
  if (live) {
    const uint32_t s = sid[i];
    live = !(flags[s] & SECURE_F_LARGE);
    lo = offs[s];
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < WPK; k++) me[k] = kw[i * WPK + k];
    atomicMin(&range_lo, (unsigned long long)lo);
    atomicMax(&range_hi, (unsigned long long)i);          // a lane looks only at keys below its own
  }
  __syncthreads();
  const size_t rlo = range_lo, rhi = range_hi;
  uint32_t best = (uint32_t)i;                // no live lane: range_hi = 0 and the loop below does not run
  for (size_t t0 = rlo + (size_t)blockIdx.y * BLS_BLOCK; t0 < rhi; t0 += S * BLS_BLOCK) {     // uniform over the workgroup
    const size_t j = t0 + threadIdx.x;
    if (j < rhi) {
#pragma unroll
      for (int k = 0; k < WPK; k++) tile[threadIdx.x * WPK + k] = kw[j * WPK + k];
    }
    __syncthreads();
    if (live) best = secure_first_tile<WPK>(best, tile, t0, rhi - t0 < BLS_BLOCK ? rhi - t0 : BLS_BLOCK, lo, me);
    __syncthreads();
  }
  if (live) atomicMin(&first[i], best);
}
template __global__ void k_secure_first<12>(size_t, const uint64_t*, const uint8_t*, const uint32_t*, const uint32_t*, uint32_t*);
template __global__ void k_secure_first<24>(size_t, const uint64_t*, const uint8_t*, const uint32_t*, const uint32_t*, uint32_t*);
template __global__ void k_secure_rank<12>(size_t, const uint64_t*, size_t, const uint8_t*, const uint32_t*, uint32_t*, uint32_t*);
template __global__ void k_secure_rank<24>(size_t, const uint64_t*, size_t, const uint8_t*, const uint32_t*, uint32_t*, uint32_t*);
#endif

#if BLS_TU_SECURE == 2
// SG: the signature group (the keys live in the other one).  part[part_offs[s]] holds set s's key sum: part_offs is key_offs where
// there is one record per key (k_share_fold, or the large set's MSM result copied there), the strip offsets of the batched multi
// verify where there is one per strip.  With flags (the batched verify_secure) the status before the tail is INVALID_SIGNATURE for
// an empty set (non-OK, so the tail skips it; k_secure_fin decides), INVALID_COEFFICIENT before any verification (:97-100), else
// OK; without flags it is OK and the tail decides everything.
template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK) k_set_out(size_t n_sets, const uint64_t* key_offs, const uint64_t* part_offs, uint32_t* flags,
                                                     const uint8_t* part, const uint8_t* sigs, int fmt, uint8_t* sig_proj, uint8_t* apk,
                                                     int32_t* status) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_sets) return;
  typedef grp<SG> SP;
  typedef grp<3 - SG> KP;
  typename SP::jac_t sg;
  SP::load(sg, sigs, s, fmt);
  SP::store(sig_proj, s, sg);
  const bool empty = key_offs[s + 1] == key_offs[s];
  uint32_t* w = (uint32_t*)(apk + s * KP::PROJ_BYTES);
  if (!empty) {
    const uint32_t* src = (const uint32_t*)(part + part_offs[s] * KP::PROJ_BYTES);
    for (int k = 0; k < KP::PROJ_BYTES / 4; k++) w[k] = src[k];
  } else {
    for (int k = 0; k < KP::PROJ_BYTES / 4; k++) w[k] = 0u;      // no keys: the identity (Z = 0)
  }
  int32_t st = BLS_OK;
  if (flags) {
    uint32_t f = flags[s];
    if (jac_is_inf(sg)) f |= SECURE_F_IDSIG;
    flags[s] = f;
    st = empty ? BLS_ERR_INVALID_SIGNATURE : (f & SECURE_F_ZERO) ? BLS_ERR_INVALID_COEFFICIENT : BLS_OK;
  }
  status[s] = st;
}
// k_share_ladder with a gather: the point of lane i is sigs[first[i]], its scalar the coefficient of key i.  A set that already
// carries a flag (a zero coefficient; a large set, summed by its own MSM) leaves the identity.
template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_secure_ladder(size_t n, const uint8_t* sigs, int fmt, const uint8_t* scal, const uint32_t* first,
                                                           const uint32_t* sid, const uint32_t* flags, uint8_t* part) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  typedef typename grp<G>::F F;
  jac<F> p, acc;
  jac_set_inf(acc);
  if (!flags[sid[i]]) {
    grp<G>::load(p, sigs, first[i], fmt);
    if (!jac_is_inf(p)) {
      aff<F> a;
      jac_to_aff(a, p);
      share_ladder<G>(acc, a, (const uint32_t*)(scal + 32 * i));
    }
  }
  grp<G>::store(part, i, acc);
}
template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_set_sum_out(size_t n_sets, const uint64_t* key_offs, const uint64_t* part_offs, const uint32_t* flags,
                                                         const uint8_t* part, uint8_t* out, int32_t* status) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_sets) return;
  const bool zero_coeff = flags && (flags[s] & SECURE_F_ZERO);
  uint32_t* w = (uint32_t*)(out + s * grp<G>::PROJ_BYTES);
  if (key_offs[s + 1] != key_offs[s] && !zero_coeff) {
    const uint32_t* src = (const uint32_t*)(part + part_offs[s] * grp<G>::PROJ_BYTES);
    for (int k = 0; k < grp<G>::PROJ_BYTES / 4; k++) w[k] = src[k];
  } else {
    for (int k = 0; k < grp<G>::PROJ_BYTES / 4; k++) w[k] = 0u;      // the identity (Z = 0)
  }
  if (status) status[s] = zero_coeff ? BLS_ERR_INVALID_COEFFICIENT : BLS_OK;
}
template __global__ void k_secure_ladder<1>(size_t, const uint8_t*, int, const uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint8_t*);
template __global__ void k_secure_ladder<2>(size_t, const uint8_t*, int, const uint8_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint8_t*);
template __global__ void k_set_sum_out<1>(size_t, const uint64_t*, const uint64_t*, const uint32_t*, const uint8_t*, uint8_t*, int32_t*);
template __global__ void k_set_sum_out<2>(size_t, const uint64_t*, const uint64_t*, const uint32_t*, const uint8_t*, uint8_t*, int32_t*);
template __global__ void k_set_out<1>(size_t, const uint64_t*, const uint64_t*, uint32_t*, const uint8_t*, const uint8_t*, int, uint8_t*, uint8_t*, int32_t*);
template __global__ void k_set_out<2>(size_t, const uint64_t*, const uint64_t*, uint32_t*, const uint8_t*, const uint8_t*, int, uint8_t*, uint8_t*, int32_t*);
#endif
