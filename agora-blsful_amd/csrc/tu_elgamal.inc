// Kernels of the ElGamal proof check and opening (blsgpu_elgamal_proof_verify_batch, blsgpu_elgamal_open_batch; elgamal.cuh),
// included by tu_elgamal1.hip (BLS_TU_ELGAMAL = 1: the key group is G1, Bls12381G2Impl) and tu_elgamal2.hip (= 2: G2).
//   k_elgamal_fixed      : once per call, the small multiples of the group generator and of the message generator
//   k_elgamal_prep       : per proof, the checks that precede the arithmetic; pk, generator, c1, c2 affine (ONE inversion) and compressed
//   k_elgamal_ladder     : per output point (2 n lanes), r1 = (-c) c1 + bp G or r2 = (-c) c2 + mp H + bp pk as one joint ladder
//   k_elgamal_transcript : per proof, r1 and r2 compressed (ONE inversion), Merlin, the 512-bit reduction, the verdict
//   k_elgamal_sub        : per ciphertext, c2 - key
#include "kernels.cuh"
#include "elgamal.cuh"

namespace {
__device__ __forceinline__ void eg_to_raw(uint32_t* w, const fp& a) { fp_to_raw(w, a); }
__device__ __forceinline__ void eg_to_raw(uint32_t* w, const fp2& a) { fp2_to_raw(w, a); }
__device__ __forceinline__ void eg_from_raw(fp& a, const uint32_t* w) { fp_from_raw(a, w); }
__device__ __forceinline__ void eg_from_raw(fp2& a, const uint32_t* w) { fp2_from_raw(a, w); }
__device__ __forceinline__ void eg_generator(g1_aff& a) {
  fp_load(a.x, G1_GEN_X);
  fp_load(a.y, G1_GEN_Y);
  a.inf = false;
}
__device__ __forceinline__ void eg_generator(g2_aff& a) {
  fp2_load(a.x, G2_GEN_X);
  fp2_load(a.y, G2_GEN_Y);
  a.inf = false;
}
template <int G>
struct eg {
  typedef typename grp<G>::F F;
  enum { E = share_ladder_t<G>::E, FW = 12 * G, K = grp<G>::COMP_BYTES };
  // record i of a Z = 1 RAW_PROJ array as an affine point
  __device__ static void load_aff(aff<F>& a, const uint8_t* recs, size_t i) {
    const uint32_t* w = (const uint32_t*)(recs + i * grp<G>::PROJ_BYTES);
    eg_from_raw(a.x, w);
    eg_from_raw(a.y, w + FW);
    a.inf = false;
  }
  __device__ static void store_aff(uint8_t* recs, size_t i, const aff<F>& a) {
    jac<F> q;
    jac_from_aff(q, a);
    grp<G>::store(recs, i, q);
  }
  __device__ static void load_scalar(uint32_t v[8], const uint8_t* s, size_t i) {
    for (int k = 0; k < 8; k++) v[k] = ((const uint32_t*)(s + 32 * i))[k];
  }
};
__device__ __forceinline__ bool eg_words_zero(const uint32_t v[8]) {
  uint32_t o = 0;
  for (int k = 0; k < 8; k++) o |= v[k];
  return o == 0;
}
}  // namespace

template <int G>
__global__ void k_elgamal_fixed(const uint8_t* h, uint32_t* fixed) {
  if (blockIdx.x || threadIdx.x) return;
  typedef typename grp<G>::F F;
  enum { E = eg<G>::E, FW = eg<G>::FW };
  jac<F> hj;
  aff<F> p[2];
  eg_generator(p[0]);
  grp<G>::load(hj, h, 0, 0);
  jac_to_aff(p[1], hj);
  for (int t = 0; t < 2; t++) {
    aff<F> tab[ELGAMAL_TAB];
    elgamal_multiples(tab, p[t]);
    for (int m = 0; m < ELGAMAL_TAB; m++) {
      eg_to_raw(fixed + (size_t)((t * ELGAMAL_TAB + m) * 2) * FW, tab[m].x);
      eg_to_raw(fixed + (size_t)((t * ELGAMAL_TAB + m) * 2 + 1) * FW, tab[m].y);
    }
  }
}

template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_elgamal_prep(size_t n, const uint8_t* pks, size_t n_pks, const uint8_t* gens, const uint8_t* h, const uint8_t* c1s,
                                                          const uint8_t* c2s, int fmt, const uint8_t* mps, const uint8_t* bps, const uint8_t* cs,
                                                          const int32_t* dec, const int32_t* dec_pk, uint8_t* aff_out, uint8_t* comp, int32_t* status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  typedef typename grp<G>::F F;
  enum { K = eg<G>::K };
  uint32_t mp[8], bp[8], ch[8];
  eg<G>::load_scalar(mp, mps, i);
  eg<G>::load_scalar(bp, bps, i);
  eg<G>::load_scalar(ch, cs, i);
  // deserialisation first: a point that did not decode, a scalar that no Scalar can hold
  int32_t st = dec ? dec[i] : BLS_OK;
  if (!st && dec_pk) st = dec_pk[0];
  if (!st && !(fr_words_canonical(mp) && fr_words_canonical(bp) && fr_words_canonical(ch))) st = BLS_ERR_BAD_ENCODING;
  jac<F> p[4];
  if (!st) {
    grp<G>::load(p[0], pks, n_pks == 1 ? 0 : i, fmt);
    if (gens) grp<G>::load(p[1], gens, i, fmt);
    else grp<G>::load(p[1], h, 0, 0);
    grp<G>::load(p[2], c1s, i, fmt);
    grp<G>::load(p[3], c2s, i, fmt);
    if (jac_is_inf(p[0]) || jac_is_inf(p[1]) || jac_is_inf(p[2]) || jac_is_inf(p[3])) st = BLS_ERR_ELGAMAL_IDENTITY;
    else if (eg_words_zero(mp) || eg_words_zero(bp) || eg_words_zero(ch)) st = BLS_ERR_ELGAMAL_ZERO_PROOF;
  }
  status[i] = st;
  if (st) return;
  aff<F> a[4];
  elgamal_to_aff<4>(a, p);
  for (int k = 0; k < 4; k++) {
    eg<G>::store_aff(aff_out, 4 * i + k, a[k]);
    uint8_t b[K];
    grp<G>::compress(b, a[k], false);
    for (int j = 0; j < K; j++) comp[(4 * i + k) * K + j] = b[j];
  }
}

template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_elgamal_ladder(size_t n, int own_gens, const uint8_t* aff_in, const uint32_t* fixed, const uint8_t* mps,
                                                            const uint8_t* bps, const uint8_t* cs, const int32_t* status, uint8_t* rj) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= 2 * n) return;
  typedef typename grp<G>::F F;
  enum { E = eg<G>::E, FW = eg<G>::FW };
  const bool second = lane >= n;
  const size_t i = second ? lane - n : lane;
  jac<F> acc;
  jac_set_inf(acc);
  if (status[i] == BLS_OK) {
    elgamal_terms<G> S;
    uint32_t k[8], nk[8];
    aff<F> a;
    // (-c) c1 or (-c) c2
    eg<G>::load_scalar(k, cs, i);
    elgamal_neg_scalar(nk, k);
    eg<G>::load_aff(a, aff_in, 4 * i + (second ? 3 : 2));
    elgamal_term_point<G>(S, 0, a);
    elgamal_term_scalar<G>(S, 0, nk);
    // bp G, or mp H with H the call's message generator or the proof's own
    eg<G>::load_scalar(k, second ? mps : bps, i);
    elgamal_term_scalar<G>(S, 1, k);
    if (second && own_gens) {
      eg<G>::load_aff(a, aff_in, 4 * i + 1);
      elgamal_term_point<G>(S, 1, a);
    } else {
      const uint32_t* f = fixed + (size_t)((second ? ELGAMAL_TAB : 0) * 2) * FW;
      for (int m = 0; m < ELGAMAL_TAB; m++) {
        eg_from_raw(S.tab[1][m].x, f + (size_t)(2 * m) * FW);
        eg_from_raw(S.tab[1][m].y, f + (size_t)(2 * m + 1) * FW);
        S.tab[1][m].inf = false;
      }
    }
    S.terms = 2;
    if (second) {        // bp pk
      eg<G>::load_scalar(k, bps, i);
      elgamal_term_scalar<G>(S, 2, k);
      eg<G>::load_aff(a, aff_in, 4 * i);
      elgamal_term_point<G>(S, 2, a);
      S.terms = 3;
    }
    elgamal_ladder<G>(acc, S);
  }
  grp<G>::store(rj, lane, acc);
}

template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_elgamal_transcript(size_t n, strobe128 prefix, const uint8_t* comp, const uint8_t* rj, const uint8_t* cs,
                                                                int32_t* status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != BLS_OK) return;
  typedef typename grp<G>::F F;
  enum { K = eg<G>::K };
  jac<F> r[2];
  aff<F> a[2];
  grp<G>::load(r[0], rj, i, 0);
  grp<G>::load(r[1], rj, n + i, 0);
  elgamal_to_aff<2>(a, r);
  uint8_t rs[2 * K], out[64];
  grp<G>::compress(rs, a[0], false);
  grp<G>::compress(rs + K, a[1], false);
  elgamal_transcript(out, prefix, comp + 4 * i * K, rs, K);
  uint32_t v[16], ch[8];
  for (int j = 0; j < 16; j++) v[j] = (uint32_t)out[4 * j] | ((uint32_t)out[4 * j + 1] << 8) | ((uint32_t)out[4 * j + 2] << 16) | ((uint32_t)out[4 * j + 3] << 24);
  fr mine, given;
  fr_from_wide(mine, v);
  eg<G>::load_scalar(ch, cs, i);
  fr_to_mont(given, ch);
  status[i] = fr_eq(mine, given) ? BLS_OK : BLS_ERR_CHALLENGE_MISMATCH;
}

template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_elgamal_sub(size_t n, const uint8_t* c2s, int fmt, const uint8_t* keys, int key_fmt, const int32_t* cst,
                                                         uint8_t* out, int32_t* status) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  typedef typename grp<G>::F F;
  const int32_t st = cst ? cst[s] : BLS_OK;
  status[s] = st;
  jac<F> a, b;
  jac_set_inf(a);
  if (st == BLS_OK) {
    grp<G>::load(a, c2s, s, fmt);
    grp<G>::load(b, keys, s, key_fmt);
    jac_neg(b, b);
    jac_add(a, a, b);
  }
  if (jac_is_inf(a)) {             // the identity leaves as all-zero bytes, as from blsgpu_combine_shares
    uint32_t* w = (uint32_t*)(out + s * grp<G>::PROJ_BYTES);
    for (int k = 0; k < grp<G>::PROJ_BYTES / 4; k++) w[k] = 0;
    return;
  }
  grp<G>::store(out, s, a);
}

template __global__ void k_elgamal_fixed<BLS_TU_ELGAMAL>(const uint8_t*, uint32_t*);
template __global__ void k_elgamal_prep<BLS_TU_ELGAMAL>(size_t, const uint8_t*, size_t, const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, int,
                                                        const uint8_t*, const uint8_t*, const uint8_t*, const int32_t*, const int32_t*, uint8_t*, uint8_t*, int32_t*);
template __global__ void k_elgamal_ladder<BLS_TU_ELGAMAL>(size_t, int, const uint8_t*, const uint32_t*, const uint8_t*, const uint8_t*, const uint8_t*,
                                                          const int32_t*, uint8_t*);
template __global__ void k_elgamal_transcript<BLS_TU_ELGAMAL>(size_t, strobe128, const uint8_t*, const uint8_t*, const uint8_t*, int32_t*);
template __global__ void k_elgamal_sub<BLS_TU_ELGAMAL>(size_t, const uint8_t*, int, const uint8_t*, int, const int32_t*, uint8_t*, int32_t*);
