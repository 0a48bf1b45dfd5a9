// translation unit: HashToScalar and the timestamp proofs of knowledge (hkdf.cuh)
//   k_hash_to_scalar   : HashToScalar::hash_to_scalar(m, salt) per lane, the general (byte-streaming) form
//   k_proof_challenge  : BlsSignatureProof::compute_y(u, t) per lane: one inversion for the affine x, then the fixed-shape hash in
//                        registers (nine sha256_compress_v calls)
//   k_proof_timeout    : the timeout rule of verify_timestamp_proof over the statuses k_prepare_proof wrote
#include "kernels.cuh"
#include "hkdf.cuh"

__global__ void __launch_bounds__(BLS_BLOCK) k_hash_to_scalar(size_t n, const uint8_t* msgs, const uint64_t* offs, const uint8_t* salt,
                                                            uint32_t salt_len, uint8_t* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint8_t y[32];
  hkdf_scalar(y, msgs + offs[i], (uint32_t)(offs[i + 1] - offs[i]), salt, salt_len);
  for (int k = 0; k < 32; k++) out[32 * i + k] = y[k];
}

template <int SG>
__global__ void __launch_bounds__(BLS_BLOCK) k_proof_challenge(size_t n, const uint8_t* commitments, int fmt, const uint64_t* timestamps,
                                                             const int32_t* bad, uint8_t* out_ys) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t y[8];
  if (bad && bad[i] != BLS_OK) {
#pragma unroll
    for (int k = 0; k < 8; k++) y[k] = 0;
  } else {
    typename grp<SG>::jac_t u;
    grp<SG>::load(u, commitments, i, fmt);
    pok_challenge_point(y, u, timestamps[i]);
  }
  uint32_t* o = (uint32_t*)(out_ys + 32 * i);
#pragma unroll
  for (int k = 0; k < 8; k++) o[k] = y[k];
}
template __global__ void k_proof_challenge<1>(size_t, const uint8_t*, int, const uint64_t*, const int32_t*, uint8_t*);
template __global__ void k_proof_challenge<2>(size_t, const uint8_t*, int, const uint64_t*, const int32_t*, uint8_t*);

__global__ void __launch_bounds__(BLS_BLOCK) k_proof_timeout(size_t n, const uint64_t* timestamps, uint64_t now_ms, int64_t timeout_ms,
                                                           const int32_t* dec, int32_t* status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int late = pok_timeout_status(timestamps[i], now_ms, timeout_ms);
  if (late) status[i] = late;
  else if (dec && dec[i] != BLS_OK) status[i] = dec[i];
}
