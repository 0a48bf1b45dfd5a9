// Kernels of the threshold signcryption calls (blsgpu_signcrypt_share_verify_batch, blsgpu_signcrypt_open_batch; signcrypt.cuh),
// included by tu_signcrypt1.hip (BLS_TU_SIGNCRYPT = 1: Bls12381G1Impl's instances and the group-independent kernels) and
// tu_signcrypt2.hip (BLS_TU_SIGNCRYPT = 2: Bls12381G2Impl's instances).
//   k_signcrypt_hash_prefix / k_signcrypt_hash_copy : the messages U.to_bytes() || V of compute_w, one per CIPHERTEXT
//   k_signcrypt_share_pairs  : one share per lane -> the two-pair record (-W', share) (w, pk) and the identity checks
//   k_signcrypt_share_status : verdicts -> BLS_OK / BLS_ERR_INVALID_DECRYPTION_SHARE
//   k_signcrypt_keystream    : one ciphertext per lane: SHAKE128 keystream, xor, prefix parse, status merge
#include "kernels.cuh"
#include "signcrypt.cuh"

template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK) k_signcrypt_hash_prefix(size_t n_ct, const uint8_t* us, int fmt, const uint64_t* v_offs, uint8_t* msgs) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_ct) return;
  typedef grp<3 - SG> PG;
  typename PG::jac_t p;
  typename PG::aff_t a;
  PG::load(p, us, c, fmt);
  jac_to_aff(a, p);
  uint8_t b[PG::COMP_BYTES];
  PG::compress(b, a, false);
  uint8_t* o = msgs + v_offs[c] + c * PG::COMP_BYTES;
  for (int k = 0; k < PG::COMP_BYTES; k++) o[k] = b[k];
}

template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK) k_signcrypt_share_pairs(size_t n, size_t n_ct, const uint64_t* share_offs, const uint8_t* shares,
                                                                   const uint8_t* pks, const uint8_t* ws, int fmt, const uint8_t* wt, uint32_t* pairs,
                                                                   int32_t* status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t c = ragged_set_of(share_offs, n_ct, i);
  typedef grp<3 - SG> PG;
  typedef grp<SG> WG;
  typename PG::jac_t share, pk;
  typename WG::jac_t w, h;
  PG::load(share, shares, i, fmt);
  PG::load(pk, pks, i, fmt);
  WG::load(w, ws, c, fmt);
  WG::load(h, wt, c, 0);
  // the reference's Choice: !share.is_identity() & !pk.is_identity() & !w.is_identity() & pairing.  A hash output is never the
  // identity in practice; if it were, the product would be the single pairing e(w, pk) of two non-identity points, never one.
  if (jac_is_inf(share) || jac_is_inf(pk) || jac_is_inf(w) || jac_is_inf(h)) {
    status[i] = BLS_ERR_INVALID_DECRYPTION_SHARE;
    return;
  }
  g1_aff P[2];
  g2_aff Q[2];
  if constexpr (SG == 1) {       // W', w in G1; share, pk in G2
    g1g2_to_aff(P[0], Q[0], h, share);
    g1g2_to_aff(P[1], Q[1], w, pk);
    fp_neg(P[0].y, P[0].y);
  } else {                       // share, pk in G1; W', w in G2
    g1g2_to_aff(P[0], Q[0], share, h);
    g1g2_to_aff(P[1], Q[1], pk, w);
    fp2_neg(Q[0].y, Q[0].y);
  }
  status[i] = BLS_OK;
  ws_st_pair(pairs, n, i, 0, P[0], Q[0]);
  ws_st_pair(pairs, n, i, 1, P[1], Q[1]);
}

template __global__ void k_signcrypt_hash_prefix<BLS_TU_SIGNCRYPT>(size_t, const uint8_t*, int, const uint64_t*, uint8_t*);
template __global__ void k_signcrypt_share_pairs<BLS_TU_SIGNCRYPT>(size_t, size_t, const uint64_t*, const uint8_t*, const uint8_t*, const uint8_t*, int,
                                                                   const uint8_t*, uint32_t*, int32_t*);

#if BLS_TU_SIGNCRYPT == 1
// byte b of the concatenated v fields moves behind the prefix of its ciphertext: coalesced, one byte per lane
__global__ void __launch_bounds__(BLS_BLOCK) k_signcrypt_hash_copy(size_t total, size_t n_ct, const uint8_t* vs, const uint64_t* v_offs, size_t K,
                                                                 uint8_t* msgs) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= total) return;
  const size_t c = ragged_set_of(v_offs, n_ct, b);
  msgs[b + (c + 1) * K] = vs[b];
}

__global__ void __launch_bounds__(BLS_BLOCK) k_signcrypt_share_status(size_t n, int32_t* status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t st = status[i];
  if (st > 0) status[i] = BLS_ERR_INVALID_DECRYPTION_SHARE;
}

__global__ void __launch_bounds__(BLS_BLOCK) k_signcrypt_keystream(size_t n_ct, const uint64_t* v_offs, const uint8_t* vs, const uint8_t* gbytes, int glen,
                                                                 const uint64_t* share_offs, uint8_t* frames, uint64_t* pt_range, int32_t* status) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_ct) return;
  uint64_t off = 0, plen = 0;
  int32_t st = status[c];
  if (share_offs && share_offs[c + 1] - share_offs[c] < 2) {       // "otherwise why use threshold": nothing is opened
    st = BLS_ERR_VSSS;
  } else {
    const uint64_t lo = v_offs[c], len = v_offs[c + 1] - lo;
    uint8_t* f = frames + lo;
    const uint8_t* g = gbytes + c * (size_t)glen;
    if (glen == 48) signcrypt_keystream_xor<48>(f, vs + lo, len, g);
    else signcrypt_keystream_xor<96>(f, vs + lo, len, g);
    const bool ok = signcrypt_parse_frame(f, len, &off, &plen);      // the lane reads back its own stores
    if (st == BLS_OK && !ok) st = BLS_ERR_BAD_FRAME;
  }
  if (st != BLS_OK) off = plen = 0;
  pt_range[2 * c] = off;
  pt_range[2 * c + 1] = plen;
  status[c] = st;
}
#endif
