// translation unit: the kernels blsgpu_signcrypt_share_verify_indexed_batch adds around those of the by-value call (signcrypt.cuh).
// A unit of its own: the kernels of tu_signcrypt1.hip and tu_signcrypt2.hip stay what they are.
//   k_signcrypt_ct_affine  : Bls12381G2Impl's table plan: -W'_c and w_c of every ciphertext as affine records, the row builder's input
//   k_signcrypt_tab_of     : ... and which two entries of that table a share reads
//   k_signcrypt_swap_pairs : Bls12381G1Impl on the one-wave path: the tabled pair (w, pk) moves to the front of the record
#include "kernels.cuh"
#include "signcrypt.cuh"

__global__ void __launch_bounds__(BLS_BLOCK) k_signcrypt_ct_affine(size_t n_ct, const uint8_t* ws, int fmt, const uint8_t* wt, uint8_t* aff) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_ct) return;
  typedef grp<2> WG;
  typename WG::jac_t w, h;
  typename WG::aff_t a;
  uint32_t* o = (uint32_t*)(aff + c * (size_t)(2 * 192));
  WG::load(h, wt, c, 0);
  jac_to_aff(a, h);                       // the identity: zero coordinates, which the row builder takes for the identity again
  fp2_neg(a.y, a.y);
  fp2_to_raw(o, a.x);
  fp2_to_raw(o + 24, a.y);
  WG::load(w, ws, c, fmt);
  // an identity w decides its shares before any row is read: its slot repeats -W', so that the row builder reports no unusable entry for it
  if (!jac_is_inf(w)) jac_to_aff(a, w);
  fp2_to_raw(o + 48, a.x);
  fp2_to_raw(o + 72, a.y);
}

__global__ void __launch_bounds__(BLS_BLOCK) k_signcrypt_tab_of(size_t n, size_t n_ct, const uint64_t* share_offs, uint32_t* t0, uint32_t* t1) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = (uint32_t)ragged_set_of(share_offs, n_ct, i);
  t0[i] = 2 * c;
  t1[i] = 2 * c + 1;
}

// one lane per word of a pair: word w of pair 0 <-> word w of pair 1 (a record that was never written swaps two unread values)
__global__ void __launch_bounds__(BLS_BLOCK) k_signcrypt_swap_pairs(size_t n, uint32_t* pairs) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * (size_t)WS_PAIR1_WORDS) return;
  const size_t lo = t, hi = t + n * (size_t)WS_PAIR1_WORDS;      // word-major: word w of item i at pairs[w n + i]
  const uint32_t a = pairs[lo], b = pairs[hi];
  pairs[lo] = b;
  pairs[hi] = a;
}
