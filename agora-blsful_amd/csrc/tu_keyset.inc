// Kernels of the registered key sets (blsgpu_keyset_*, the *_indexed_batch entry points; keyset.cuh), included by tu_keyset1.hip
// (BLS_TU_KEYSET = 1: the group-independent kernels and G1 keys, i.e. Bls12381G2Impl) and tu_keyset2.hip (BLS_TU_KEYSET = 2: G2
// keys, i.e. Bls12381G1Impl).
//   k_keyset_seal           : create: the stored affine record and Modern bytes of every entry
//   k_keyset_build          : create: the fixed-base table, one lane per key, ONE inversion per lane
//   k_keyset_lines          : create: the line table of G2 keys, one lane pair per key, ONE inversion per key
//   k_keyset_seal_at, k_keyset_build_at, k_keyset_lines_at : update / append: the same three per-key bodies on the entries a
//                             position list names (lane l: input and workspace row l, entry pos[l])
//   k_keyset_check          : every position's index and entry status, once; the sanitised indices and each set's precedence
//   k_keyset_fin            : the precedence over the statuses of the verification tail
//   k_keyset_fin_aux        : the same over statuses and aux words (the batched aggregate verify)
//   k_keyset_gather         : records by index (affine records, compressed bytes with the Legacy header transcode, statuses)
//   k_keyset_accumulate_seg : the strip sum of the batched multi verify over table[idx[i]], mixed additions only
//   k_keyset_mul            : scalar times entry, from the fixed-base table or by the joint NAF ladder of the threshold recovery
#include "kernels.cuh"
#include "keyset.cuh"

// one coordinate in the internal limb form (Fp: FP_NL words; Fp2: c0 then c1): what the table and the build workspace hold, so
// that a table read needs no radix change
__device__ __forceinline__ void ks_st(uint32_t* e, const fp& a) {
#pragma unroll
  for (int k = 0; k < FP_NL; k++) e[k] = (uint32_t)a.l[k];
}
__device__ __forceinline__ void ks_st(uint32_t* e, const fp2& a) {
  ks_st(e, a.c0);
  ks_st(e + FP_NL, a.c1);
}
__device__ __forceinline__ void ks_ld(fp& r, const uint32_t* e) {
#pragma unroll
  for (int k = 0; k < FP_NL; k++) r.l[k] = (int32_t)e[k];
}
__device__ __forceinline__ void ks_ld(fp2& r, const uint32_t* e) {
  ks_ld(r.c0, e);
  ks_ld(r.c1, e + FP_NL);
}
// one coordinate as the caller formats carry it (blst Montgomery words)
__device__ __forceinline__ void ks_raw(uint32_t* w, const fp& a) { fp_to_raw(w, a); }
__device__ __forceinline__ void ks_raw(uint32_t* w, const fp2& a) { fp2_to_raw(w, a); }
#define KS_CO_WORDS(G) ((G) * FP_NL)                 // words of one coordinate
#define KS_TAB_WORDS(G) (2 * KS_CO_WORDS(G))         // one table record: x, y

#if BLS_TU_KEYSET == 1
__global__ void __launch_bounds__(BLS_BLOCK) k_keyset_check(size_t n, const uint64_t* offs, size_t n_sets, const uint32_t* idx, uint64_t n_keys,
                                                          const int32_t* kstatus, uint32_t* cidx, unsigned long long* pre, const int32_t* nolines,
                                                          uint32_t* walk) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t s = offs ? ragged_set_of(offs, n_sets, i) : i;
  const uint32_t ix = idx[i];
  const bool oob = (uint64_t)ix >= n_keys;
  const int32_t st = oob ? 0 : kstatus[ix];          // nothing outside the table is read
  cidx[i] = oob ? KEYSET_SKIP : ix;
  const uint64_t key = keyset_pre_key(oob, offs ? i - offs[s] : 0, st);
  if (key != KEYSET_PRE_NONE) atomicMin(&pre[s], (unsigned long long)key);
  if (nolines && !oob && nolines[ix] == KEYSET_NOLINES_FINITE) atomicOr(walk, 1u);
}
__global__ void __launch_bounds__(BLS_BLOCK) k_keyset_fin(size_t n_sets, const unsigned long long* pre, int32_t* status) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_sets) return;
  const uint64_t key = pre[s];
  if (key != KEYSET_PRE_NONE) status[s] = keyset_pre_status(key);
}
__global__ void __launch_bounds__(BLS_BLOCK) k_keyset_fin_aux(size_t n_sets, const unsigned long long* pre, int32_t* status, uint64_t* aux) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_sets) return;
  const uint64_t key = pre[s];
  if (key == KEYSET_PRE_NONE) return;
  status[s] = keyset_pre_status(key);
  if (aux) aux[2 * s] = aux[2 * s + 1] = 0;
}
// one lane per 32-bit word of the output
__global__ void __launch_bounds__(BLS_BLOCK) k_keyset_gather(size_t n, size_t words, const uint32_t* cidx, const uint32_t* src, int legacy,
                                                           uint32_t* dst) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * words) return;
  const size_t i = t / words, k = t % words;
  const uint32_t ix = cidx[i];
  uint32_t w = ix == KEYSET_SKIP ? 0u : src[(size_t)ix * words + k];
  if (legacy && k == 0 && ix != KEYSET_SKIP) {
    uint8_t b0 = (uint8_t)w;                       // byte 0 of the record: the header
    header_to_legacy(&b0);
    w = (w & 0xffffff00u) | b0;
  }
  dst[t] = w;
}
#endif

// input key i (any raw format; the identity when status[i] is not OK) -> the stored record and Modern bytes of entry k
template <int G>
__device__ __forceinline__ void keyset_seal_entry(size_t i, size_t k, const uint8_t* pts, int fmt, const int32_t* status, uint8_t* recs, uint8_t* comp) {
  typename grp<G>::jac_t p;
  typename grp<G>::aff_t a;
  if (status[i] != BLS_OK) jac_set_inf(p);
  else grp<G>::load(p, pts, i, fmt);
  jac_to_aff(a, p);
  uint32_t* w = (uint32_t*)(recs + k * (grp<G>::PROJ_BYTES / 3 * 2));
  if (a.inf) {
    for (int j = 0; j < grp<G>::PROJ_BYTES / 6; j++) w[j] = 0u;
  } else {
    ks_raw(w, a.x);
    ks_raw(w + grp<G>::PROJ_BYTES / 12, a.y);
  }
  uint8_t b[grp<G>::COMP_BYTES];
  grp<G>::compress(b, a, false);
  for (int j = 0; j < grp<G>::COMP_BYTES; j++) comp[k * grp<G>::COMP_BYTES + j] = b[j];
}
template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_keyset_seal(size_t n, const uint8_t* pts, int fmt, const int32_t* status, uint8_t* recs, uint8_t* comp) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  keyset_seal_entry<G>(i, i, pts, fmt, status, recs, comp);
}
template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_keyset_seal_at(size_t n, const uint8_t* pts, int fmt, const int32_t* status, const uint32_t* pos, uint8_t* recs,
                                                            uint8_t* comp, int32_t* kstatus) {
  const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n) return;
  const size_t k = pos[l];
  keyset_seal_entry<G>(l, k, pts, fmt, status, recs, comp);
  kstatus[k] = status[l];
}

template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_keyset_to_proj(size_t n, const uint8_t* recs, uint8_t* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  typename grp<G>::jac_t p;
  grp<G>::load(p, recs, i, 1);
  if (jac_is_inf(p)) {             // the identity leaves as all-zero bytes, as from blsgpu_sum_batch
    uint32_t* w = (uint32_t*)(out + i * grp<G>::PROJ_BYTES);
    for (int k = 0; k < grp<G>::PROJ_BYTES / 4; k++) w[k] = 0u;
    return;
  }
  grp<G>::store(out, i, p);
}

// Workspace row `l` serves key `key` (k_keyset_build: k0 + l; k_keyset_build_at: pos[l]).  Its POINTS multiples are computed as
// Jacobian points (per window: B, 2B = dbl, 3B .. 8B by additions of B, then the next window's B = dbl(8B) -- a doubling and seven additions per window), each kept in jac_ws with the
// running product of the Z coordinates in prod_ws; ONE inversion of the last product and a walk back give every 1 / Z.  A key of
// order r has no multiple d 2^(4j) P = identity (d 2^(4j) has the prime factors 2, 3, 5, 7 only); a raw point that is no such key
// may, and then leaves a zero record, which k_keyset_mul skips.
template <int G>
__device__ __forceinline__ void keyset_build_entry(size_t key, size_t l, const uint8_t* recs, uint8_t* jac_ws, uint8_t* prod_ws, uint8_t* table) {
  typedef keyset_shape<G> S;
  typedef typename grp<G>::F F;
  constexpr int C = KS_CO_WORDS(G);
  jac<F> base, m;
  grp<G>::load(base, recs, key, 1);
  if (jac_is_inf(base)) return;               // the identity or an invalid entry: k_keyset_mul never reads its table (stale rows included)
  uint32_t* jw = (uint32_t*)jac_ws + l * (size_t)S::POINTS * 3 * C;
  uint32_t* pw = (uint32_t*)prod_ws + l * (size_t)S::POINTS * C;
  uint32_t* tw = (uint32_t*)table + key * (size_t)S::POINTS * KS_TAB_WORDS(G);
  F run, one;
  fe_one(run);
  fe_one(one);
  int rec = 0;
  for (int j = 0; j <= S::FULL; j++) {
    m = base;
    const int row = j < S::FULL ? KEYSET_ROW : 1;       // the carry window holds 1 B alone
    for (int d = 1; d <= row; d++) {
      if (d == 2) jac_dbl(m, base);
      else if (d > 2) jac_add(m, m, base);
      ks_st(jw + (size_t)rec * 3 * C, m.x);
      ks_st(jw + (size_t)rec * 3 * C + C, m.y);
      ks_st(jw + (size_t)rec * 3 * C + 2 * C, m.z);
      F z = m.z;
      if (fe_is_zero(z)) z = one;
      fe_mul(run, run, z);
      fe_reduce(run, run);
      ks_st(pw + (size_t)rec * C, run);
      rec++;
    }
    if (j < S::FULL) jac_dbl(base, m);                  // 16 B
  }
  F inv;
  fe_inv(inv, run);
  for (rec = S::POINTS - 1; rec >= 0; rec--) {
    ks_ld(m.x, jw + (size_t)rec * 3 * C);
    ks_ld(m.y, jw + (size_t)rec * 3 * C + C);
    ks_ld(m.z, jw + (size_t)rec * 3 * C + 2 * C);
    uint32_t* t = tw + (size_t)rec * KS_TAB_WORDS(G);
    if (fe_is_zero(m.z)) {
      for (int k = 0; k < KS_TAB_WORDS(G); k++) t[k] = 0u;
      continue;
    }
    F zi = inv, zi2;
    if (rec) {
      ks_ld(zi2, pw + (size_t)(rec - 1) * C);
      fe_mul(zi, inv, zi2);
    }
    fe_mul(inv, inv, m.z);
    fe_reduce(inv, inv);
    fe_sqr(zi2, zi);
    fe_mul(m.x, m.x, zi2);
    fe_mul(zi2, zi2, zi);
    fe_mul(m.y, m.y, zi2);
    fe_reduce(m.x, m.x);
    fe_reduce(m.y, m.y);
    ks_st(t, m.x);
    ks_st(t + C, m.y);
  }
}
template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_keyset_build(size_t k0, size_t cnt, const uint8_t* recs, uint8_t* jac_ws, uint8_t* prod_ws, uint8_t* table) {
  const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= cnt) return;
  keyset_build_entry<G>(k0 + l, l, recs, jac_ws, prod_ws, table);
}
template <int G>
__global__ void __launch_bounds__(BLS_BLOCK) k_keyset_build_at(size_t cnt, const uint32_t* pos, const uint8_t* recs, uint8_t* jac_ws, uint8_t* prod_ws,
                                                             uint8_t* table) {
  const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= cnt) return;
  keyset_build_entry<G>(pos[l], l, recs, jac_ws, prod_ws, table);
}

#if BLS_TU_KEYSET == 2
// this lane's half of the rows of entry k, through scratch row l; nolines[k] = 0 or KEYSET_NOLINES_* (an entry that is, or has
// become, the identity or invalid keeps whatever rows it had: nothing reads them)
__device__ __forceinline__ void keyset_lines_pair(size_t k, size_t l, const uint8_t* recs, uint32_t* table, uint32_t* scratch, int32_t* nolines) {
  const size_t lane = lane_hi() ? FP_NL : 0;
  const group_lines_io io = {table + k * (size_t)SHARED_TABLE_WORDS + lane, scratch + l * (size_t)SHARED_TABLE_WORDS + lane};
  const int no = keyset_lines_entry((const uint32_t*)(recs + k * 192), io);
  if (!lane_hi()) nolines[k] = no;
}
__global__ void __launch_bounds__(BLS_BLOCK) k_keyset_lines(size_t k0, size_t cnt, const uint8_t* recs, uint32_t* table, uint32_t* scratch, int32_t* nolines) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t l = t >> 1;                                  // both lanes of a pair are inside or outside: BLS_BLOCK is even
  if (l >= cnt) return;
  keyset_lines_pair(k0 + l, l, recs, table, scratch, nolines);
}
__global__ void __launch_bounds__(BLS_BLOCK) k_keyset_lines_at(size_t cnt, const uint32_t* pos, const uint8_t* recs, uint32_t* table, uint32_t* scratch,
                                                             int32_t* nolines) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t l = t >> 1;
  if (l >= cnt) return;
  keyset_lines_pair(pos[l], l, recs, table, scratch, nolines);
}
#endif

#if BLS_TU_KEYSET == 1
// one lane per strip
template <>
__global__ void __launch_bounds__(BLS_BLOCK) k_keyset_accumulate_seg<1>(size_t n_strips, const uint8_t* recs, const uint32_t* cidx, const uint64_t* key_offs,
                                                                      const uint64_t* strip_offs, const uint32_t* strip_sid, uint8_t* part) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_strips) return;
  const multi_strip st = multi_strip_of(g, key_offs, strip_offs, strip_sid);
  g1_jac acc;
  fp x, y;
  jac_set_inf(acc);
  for (uint64_t i = st.first; i < st.end; i += st.stride) {
    const uint32_t ix = cidx[i];
    if (ix == KEYSET_SKIP) continue;
    const uint32_t* w = (const uint32_t*)(recs + (size_t)ix * 96);
    if (words_all_zero(w, 24)) continue;                  // the identity or an invalid entry adds nothing
    fp_from_raw(x, w);
    fp_from_raw(y, w + 12);
    jac_madd(acc, acc, x, y);
  }
  store_g1_pt(part, g, acc);
}
#else
// one lane pair per strip on the lane-split tower, as k_multi_accumulate_seg<2>
template <>
__global__ void __launch_bounds__(BLS_BLOCK, 2) k_keyset_accumulate_seg<2>(size_t n_strips, const uint8_t* recs, const uint32_t* cidx, const uint64_t* key_offs,
                                                                         const uint64_t* strip_offs, const uint32_t* strip_sid, uint8_t* part) {
  const size_t g = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1;
  if (g >= n_strips) return;
  const multi_strip st = multi_strip_of(g, key_offs, strip_offs, strip_sid);
  jac<hfp2> acc;
  hfp2 x, y;
  jac_set_inf(acc);
  for (uint64_t i = st.first; i < st.end; i += st.stride) {
    const uint32_t ix = cidx[i];
    if (ix == KEYSET_SKIP) continue;
    const uint32_t* w0 = (const uint32_t*)(recs + (size_t)ix * 192);
    if (words_all_zero(w0, 48)) continue;
    const uint32_t* w = w0 + (lane_hi() ? 12 : 0);
    fp_from_raw(x.v, w);
    fp_from_raw(y.v, w + 24);
    jac_madd_body(acc, acc, x, y);                        // the body: the accumulator stays in registers (k_accumulate_g2s)
  }
  st_g2s(part, g, acc);
}
#endif

// image e of a table point with the signs of the decomposition folded in (msm2.cuh: G1 Q1 = -phi; G2 Q1 = -psi, Q2 = psi^2,
// Q3 = -psi^3), negated once more for a negative digit
__device__ __forceinline__ void keyset_image(fp& x, fp& y, int e, bool neg) {
  if (e == 1) {
    fp beta;
    fp_load(beta, G1_BETA);
    fp_mul(x, x, beta);
    neg = !neg;
  }
  if (neg) {
    fp_neg(y, y);
    fp_reduce(y, y);
  }
}
__device__ __forceinline__ void keyset_image(fp2& x, fp2& y, int e, bool neg) {
  if (e >= 2) {
    fp cx2, cy2;
    fp_load(cx2, PSI2_CX);
    fp_load(cy2, PSI2_CY);
    fp2_mul_fp(x, x, cx2);
    fp2_mul_fp(y, y, cy2);
  }
  if (e & 1) {
    fp2 t;
    fp2_conj(t, x);
    fp2_mul_const(x, t, PSI_CX);
    fp2_conj(t, y);
    fp2_mul_const(y, t, PSI_CY);
    neg = !neg;
  }
  if (neg) fp2_neg(y, y);
  fp2_reduce(x, x);
  fp2_reduce(y, y);
}

template <int G, int TAB>
__global__ void __launch_bounds__(BLS_BLOCK) k_keyset_mul(size_t n, const uint8_t* recs, const uint8_t* table, const uint32_t* cidx, const uint8_t* scal,
                                                        const uint32_t* sid, const uint32_t* flags, uint8_t* part) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  typedef keyset_shape<G> S;
  typedef typename grp<G>::F F;
  jac<F> p, acc;
  jac_set_inf(acc);
  const uint32_t ix = cidx[i];
  if (ix != KEYSET_SKIP && !(flags && flags[sid[i]])) {
    grp<G>::load(p, recs, ix, 1);
    if (!jac_is_inf(p)) {
      const uint32_t* lam = (const uint32_t*)(scal + 32 * i);
      if constexpr (TAB) {
        uint64_t a[4];
        share_ladder_t<G>::decompose(a, lam);
        uint32_t carry[S::E];
#pragma unroll
        for (int e = 0; e < S::E; e++) carry[e] = 0;
        const uint32_t* tw = (const uint32_t*)table + (size_t)ix * S::POINTS * KS_TAB_WORDS(G);
        for (int j = 0; j < S::WINDOWS; j++) {
#pragma unroll
          for (int e = 0; e < S::E; e++) {
            const int d = keyset_digit(a + e * S::WORDS, S::WORDS, j, carry[e]);
            if (d == 0) continue;
            const uint32_t* t = tw + (size_t)keyset_record(j, d < 0 ? -d : d) * KS_TAB_WORDS(G);
            F x, y;
            ks_ld(x, t);
            ks_ld(y, t + KS_CO_WORDS(G));
            if (fe_is_zero(x) && fe_is_zero(y)) continue;      // a multiple that is the identity (no key of order r has one)
            keyset_image(x, y, e, d < 0);
            jac_madd(acc, acc, x, y);
          }
        }
      } else {
        aff<F> q;
        q.x = p.x;
        q.y = p.y;
        q.inf = false;
        share_ladder<G>(acc, q, lam);
      }
    }
  }
  grp<G>::store(part, i, acc);
}

template __global__ void k_keyset_seal<BLS_TU_KEYSET>(size_t, const uint8_t*, int, const int32_t*, uint8_t*, uint8_t*);
template __global__ void k_keyset_seal_at<BLS_TU_KEYSET>(size_t, const uint8_t*, int, const int32_t*, const uint32_t*, uint8_t*, uint8_t*, int32_t*);
template __global__ void k_keyset_to_proj<BLS_TU_KEYSET>(size_t, const uint8_t*, uint8_t*);
template __global__ void k_keyset_build<BLS_TU_KEYSET>(size_t, size_t, const uint8_t*, uint8_t*, uint8_t*, uint8_t*);
template __global__ void k_keyset_build_at<BLS_TU_KEYSET>(size_t, const uint32_t*, const uint8_t*, uint8_t*, uint8_t*, uint8_t*);
template __global__ void k_keyset_mul<BLS_TU_KEYSET, 0>(size_t, const uint8_t*, const uint8_t*, const uint32_t*, const uint8_t*, const uint32_t*, const uint32_t*,
                                                        uint8_t*);
template __global__ void k_keyset_mul<BLS_TU_KEYSET, 1>(size_t, const uint8_t*, const uint8_t*, const uint32_t*, const uint8_t*, const uint32_t*, const uint32_t*,
                                                        uint8_t*);
