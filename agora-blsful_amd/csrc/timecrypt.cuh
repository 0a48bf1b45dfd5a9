// Pairing VALUES on the wave-cooperative engine (coop.cuh): blsgpu_pairing_batch, the Gt export that time-lock decryption
// (reference src/traits/time_crypt.rs:76-141: K = e(sig, u), then a hash of K.to_bytes()) is built on.  One 64-lane wave per item:
//   * coop_miller1: the Miller loop of ONE walked pair into S.f -- coop_miller2's rounds with the second owner and the second line
//     multiplication dropped;
//   * coop_final_value (coop.cuh): coop_final_verdict without the comparison, the value in S.t;
//   * coop_gt_bytes: the 576 bytes of Gt::to_bytes() as this library ASSUMES them (include/blsgpu.h), placed by gt_part_offset --
//     the one place that knows the byte order, which the lane-split export (k_finalexp2s_value) shares.
// Device code; tests/hostsim_timecrypt compiles the same functions on the host (one thread per lane pair) under the bound tracker.
#pragma once
#include "fp.cuh"
#define GT_BYTES 576

// ---- Gt::to_bytes(), 576 bytes, AS THIS LIBRARY ASSUMES IT (include/blsgpu.h): the six Fp2 coefficients over
// w^0..w^5 -- in tower terms c0.a0, c1.a0, c0.a1, c1.a1, c0.a2, c1.a2, the order of coop_f12 --, each its real part, then its
// imaginary part, each part 48 bytes big-endian of the canonical residue (not Montgomery).  No reference vector pins this order; if
// it turns out wrong, the fix is a permutation in the two functions below and in tests/timecrypt_ref.py gt_bytes.  They are the ONE
// place on the device that knows the order: both exports -- coop_gt_bytes on the one-wave engine, whose coop_f12 holds the
// coefficients by w-power, and fx_export of k_finalexp2s_value on the lane-split kernels, whose accumulator is in tower order --
// place every part through them.
//   gt_part_offset(k, imag): where the real (imag = false) or imaginary part of the coefficient over w^k starts;
//   gt_tower_wpow(j): the w-power of tower slot j (0..5: c0.a0, c0.a1, c0.a2, c1.a0, c1.a1, c1.a2), since w^2 = v.
BLS_FN int gt_part_offset(int k, bool imag) { return 96 * k + (imag ? 48 : 0); }
BLS_FN int gt_tower_wpow(int j) { return j < 3 ? 2 * j : 2 * (j - 3) + 1; }
// One Fp part: the canonical integer (fp_from_mont) as twelve byte-swapped 32-bit words, assembled in registers.
BLS_FN void coop_gt_put(uint8_t* dst, const fp& a) {
  fp t;
  uint32_t ww[12];
  fp_from_mont(t, a);
  fp_get_words(ww, t);
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const uint32_t w = __builtin_bswap32(ww[11 - i]);
    __builtin_memcpy(dst + 4 * i, &w, 4);           // dst may be any caller address: no alignment is assumed
  }
}

// the engine part: the translation unit of the kernels (BLS_TU_TIMECRYPT, after kernels.cuh) and the host harness
#if defined(BLS_TU_TIMECRYPT) || !defined(__HIPCC__)
#include "coop.cuh"

// Miller loop of the pair (P, Q), Q walked by lane pair 0, into S.f: conj(f_{|x|,Q}(P)) up to a factor in Fp2, which the easy part of
// the final exponentiation removes.  The product rounds are coop_miller2's (fixed_g2 = 0): the job slots of its second pair are
// multiplied along and never read.
__device__ __noinline__ void coop_miller1(coop_shared& S, const g1_aff& P, const aff<hfp2>& Q) {
  const int me = coop_pair();
  const bool owner = me == 0;
  hfp2 xp2, yp2;                                 // (xP, 0), (yP, 0): Fp scalings as Fp2 products, so that all jobs are alike
#if defined(__HIPCC__)
  {
    fp z;
    fp_zero(z);
    fp_sel(xp2.v, lane_hi(), z, P.x);
    fp_sel(yp2.v, lane_hi(), z, P.y);
  }
#else
  fp2_from_fp(xp2, P.x);
  fp2_from_fp(yp2, P.y);
#endif
  g2_hom_t<hfp2> T;
  T.x = Q.x;
  T.y = Q.y;
  fp2_one(T.z);
  if (me < 6) {                                  // f = 1
    hfp2 x;
    if (me == 0) fp2_one(x);
    else fp2_zero(x);
    coop_st(S.f.c[me], x);
  }
  __syncthreads();
  hfp2 l0, l2, l3, t;
  for (int i = 62; i >= 0; i--) {
    // ---- doubling step, exactly coop_miller2's general pair (miller_dbl_step cut into two product rounds; same bounds)
    hfp2 a, b, c, e, f, h, g, s;
    if (owner) {
      fp2_add(h, T.y, T.z);
      fp2_norm(h, h);
      coop_job_put(S, 0, 0, T.x, T.y);
      coop_job_put(S, 0, 1, T.y, T.y);
      coop_job_put(S, 0, 2, T.z, T.z);
      coop_job_put(S, 0, 3, T.x, T.x);
      coop_job_put(S, 0, 4, h, h);
    }
    if (i != 62) coop_sqr_with_jobs(S, S.f);
    else coop_jobs(S, 5);
    if (owner) {
      coop_ld(a, S.res[0][0]);       // XY
      coop_ld(b, S.res[0][1]);       // B = Y^2
      coop_ld(c, S.res[0][2]);       // C = Z^2
      coop_ld(s, S.res[0][3]);       // X^2
      coop_ld(h, S.res[0][4]);       // (Y + Z)^2
      fp2_mul_xi(e, c);
      fp2_dbl(g, e);
      fp2_add(e, g, e);
      fp2_reduce(e, e);
      fp2_dbl(e, e);
      fp2_dbl(e, e);
      fp2_norm(e, e);                 // E = 3b'C
      fp2_dbl(f, e);
      fp2_add(f, f, e);               // F = 3E
      fp2_sub(h, h, b);
      fp2_sub(h, h, c);
      fp2_norm(h, h);                 // H = 2YZ
      fp2_sub(l0, b, e);
      fp2_norm(l0, l0);
      fp2_dbl(g, s);
      fp2_add(g, g, s);
      fp2_neg(g, g);
      fp2_norm(g, g);                 // -3X^2
      fp2_sub(t, b, f);
      fp2_norm(t, t);
      coop_job_put(S, 0, 0, a, t);   // XY (B - F)
      fp2_add(t, b, f);
      fp2_norm(t, t);
      coop_job_put(S, 0, 1, t, t);   // (B + F)^2
      coop_job_put(S, 0, 2, e, e);   // E^2
      coop_job_put(S, 0, 3, b, h);   // BH
      coop_job_put(S, 0, 4, g, xp2); // l2
      coop_job_put(S, 0, 5, h, yp2); // l3
    }
    coop_jobs(S, 6);
    if (owner) {
      coop_ld(g, S.res[0][0]);
      fp2_dbl(g, g);
      fp2_reduce(T.x, g);             // X3 = 2XY(B - F)
      coop_ld(g, S.res[0][1]);
      coop_ld(s, S.res[0][2]);
      fp2_dbl(a, s);
      fp2_add(a, a, s);
      fp2_norm(a, a);
      fp2_dbl(a, a);
      fp2_dbl(a, a);                  // 12E^2
      fp2_sub(g, g, a);
      fp2_reduce(T.y, g);             // Y3 = (B + F)^2 - 12E^2
      coop_ld(g, S.res[0][3]);
      fp2_dbl(g, g);
      fp2_dbl(g, g);
      fp2_reduce(T.z, g);             // Z3 = 4BH
      coop_ld(l2, S.res[0][4]);
      coop_ld(l3, S.res[0][5]);
      coop_st(S.line[0][0], l0);
      coop_st(S.line[0][1], l2);
      coop_st(S.line[0][2], l3);
    }
    __syncthreads();
    coop_mul_line(S, S.f, 0);
    // ---- addition step (set bits of |x|)
    if ((BLS_X_ABS >> i) & 1) {
      if (owner) {
        miller_add_step(T, l0, l2, l3, Q.x, Q.y, P.x, P.y);
        coop_st(S.line[0][0], l0);
        coop_st(S.line[0][1], l2);
        coop_st(S.line[0][2], l3);
      }
      __syncthreads();
      coop_mul_line(S, S.f, 0);
    }
  }
  coop_conj(S.f, S.f);
}

// the value a (reduced coefficients, as every coop_* function leaves them) -> out[0, 576): lane pair k < 6 writes coefficient k, the
// even lane its real part and the odd lane its imaginary part, 48 bytes each
__device__ __forceinline__ void coop_gt_bytes(uint8_t* out, const coop_f12& a) {
  const int k = coop_pair();
  if (k < 6) {
    hfp2 x;
    coop_ld(x, a.c[k]);
#if defined(__HIPCC__)
    coop_gt_put(out + gt_part_offset(k, lane_hi()), x.v);
#else
    coop_gt_put(out + gt_part_offset(k, false), x.c[0]);
    coop_gt_put(out + gt_part_offset(k, true), x.c[1]);
#endif
  }
}

#if defined(__HIPCC__)
// Gt one: 00..01 in the first 48 bytes, then zeros (all 64 lanes of the wave store 32-bit words); zero = true: 576 zero bytes
__device__ __forceinline__ void coop_gt_const(uint8_t* out, bool zero) {
  for (int w = threadIdx.x; w < GT_BYTES / 4; w += BLS_BLOCK) {
    const uint32_t v = (w == 11 && !zero) ? 0x01000000u : 0u;      // byte 47 = 1
    __builtin_memcpy(out + 4 * w, &v, 4);
  }
}
#endif

// ---- the time-lock tail (reference src/traits/time_crypt.rs:86-115), one item per lane after the pairing.  Public inputs only:
// nothing here is constant time.  Also compiles as plain C++ (tests/hostsim_timecrypt).
#include "hkdf.cuh"
#include "signcrypt.cuh"
#include "shares.cuh"
#define TIMECRYPT_SALT "TIMELOCK_BLS12381_XOF:HKDF-SHA2-256_"   // src/traits/time_crypt.rs:13
#define TIMECRYPT_SALT_LEN 36
// alpha = SHA-256(K.to_bytes()) xor v (compute_v, :119-127): the 576 bytes are nine whole blocks, the tenth is the padding alone --
// every block in sixteen registers, as the fixed shapes of hkdf.cuh
BLS_FN void timecrypt_alpha(uint8_t* alpha, const uint8_t* gt, const uint8_t* v) {
  hk_h h = hk_iv();
  hk_w w;
  for (int b = 0; b < GT_BYTES / 64; b++) {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      uint32_t x;
      __builtin_memcpy(&x, gt + 64 * b + 4 * j, 4);
      w[j] = __builtin_bswap32(x);
    }
    h = hk_compress(h, w);
  }
  w[0] = 0x80000000u;
  hk_tail(w, 1, GT_BYTES - 64);                  // the bit length of 576 bytes
  h = hk_compress(h, w);
#pragma unroll
  for (int j = 0; j < 8; j++)
    for (int k = 0; k < 4; k++) alpha[4 * j + k] = (uint8_t)(h[j] >> (24 - 8 * k)) ^ v[4 * j + k];
}
// One item from its pairing value to the scalar of the check: frame[0, len) = SHAKE128(alpha) xor w (compute_w, :130-141), the length
// prefix -- a failed `peek` leaves the message EMPTY and the check goes on, a length beyond the frame is None (:89-102) --, then
// r = hash_to_scalar(alpha || SHA-256(message)) as eight little-endian words (zero stays zero, as blsgpu_hash_to_scalar writes it).
// Returns BLS_OK with *pt_off, *pt_len and r set, or BLS_ERR_BAD_FRAME.  len is below 2^29 (the host checks it).
BLS_FN int timecrypt_open_frame(uint8_t* frame, const uint8_t* w, uint64_t len, const uint8_t* gt, const uint8_t* v, uint64_t* pt_off, uint64_t* pt_len,
                                uint32_t* r) {
  uint8_t ikm[64];                               // alpha || SHA-256(message)
  timecrypt_alpha(ikm, gt, v);
  signcrypt_keystream_xor<32>(frame, w, len, ikm);
  uint64_t off = 0, plen = 0;
  const int kind = signcrypt_parse_frame_kind(frame, len, &off, &plen);
  if (kind == SIGNCRYPT_FRAME_BEYOND) return BLS_ERR_BAD_FRAME;
  if (kind == SIGNCRYPT_FRAME_NO_PREFIX) off = plen = 0;
  sha256_ctx c;
  sha256_init(c);
  sha256_update(c, frame + off, (uint32_t)plen);
  sha256_final(c, ikm + 32);
  uint8_t rb[32];
  hkdf_scalar(rb, ikm, 64, (const uint8_t*)TIMECRYPT_SALT, TIMECRYPT_SALT_LEN);
  for (int j = 0; j < 8; j++) r[j] = (uint32_t)rb[4 * j] | ((uint32_t)rb[4 * j + 1] << 8) | ((uint32_t)rb[4 * j + 2] << 16) | ((uint32_t)rb[4 * j + 3] << 24);
  *pt_off = off;
  *pt_len = plen;
  return BLS_OK;
}
// g r == u, projectively: (g r) - u is the identity (:112-115).  g: the generator of u's group G, affine; g r by the joint NAF ladder
// of the threshold recovery (shares.cuh share_ladder: 128 doublings in G1, 64 in G2 over the endomorphism split of r)
template <int G, class F>
BLS_FN bool timecrypt_check(const aff<F>& g, const uint32_t* r, const jac<F>& u) {
  jac<F> gr, nu, d;
  share_ladder<G>(gr, g, r);
  jac_neg(nu, u);
  jac_add(d, gr, nu);
  return jac_is_inf(d);
}
#endif  // the engine part

#if defined(__HIPCC__)
#define PV_RUN 0        // flag values of k_pairing_value_prepare: walk the pair
#define PV_ONE 1        // a member is the identity: the value is Gt one (multi_miller_loop skips such a pair)
#define PV_ZERO 2       // a member did not decode: 576 zero bytes
// pair i of caller-format points -> the one-pair affine workspace (word-major, stride n, slot 0) and flag[i].  status == nullptr:
// raw formats, nothing to check.  Otherwise status[i] holds the decode status of the pair (the points are then RAW_PROJ from
// k_decompress; a point that did not decode is never read).
__global__ void k_pairing_value_prepare(size_t n, const uint8_t* g1s, const uint8_t* g2s, int fmt, const int32_t* status, uint32_t* pairs, int32_t* flag);
// items first .. first + count - 1, one wave each: coop_miller1, coop_final_value, coop_gt_bytes -> out_gt[576 i ..)
__global__ void k_pairing_value(size_t n, size_t first, size_t count, const uint32_t* pairs, const int32_t* flag, uint8_t* out_gt);
// The same value on the lane-split kernels (tu_finalexp2_value.hip), two lanes per item: the final exponentiation of items
// [first, first + count) of the Fp12 workspace fws (stride n; conj(f) as k_millerfp3 / k_millerf_rows1 leave it) with k_finalexp2s's
// operations and value store vp, ended as a VALUE -- t f^3 -- whose 576 bytes go to out_gt[576 i ..).  An item whose flag is not PV_RUN
// reads nothing and gets k_pairing_value's constants, written by its lane pair.
__global__ void k_finalexp2s_value(size_t n, size_t first, size_t count, const uint32_t* fws, uint32_t* vp, size_t lanes, const int32_t* flag, uint8_t* out_gt);
// blsgpu_timecrypt_open_batch, one lane per item.  Item i belongs to the group g with item_offs[g] <= i < item_offs[g + 1] (found by
// bisection; empty groups own nothing).  status[i] = the first that applies of: the decode status of u_i (dec_u), of sig_g (dec_sig;
// both null for the raw formats), BLS_ERR_INVALID_SCHEME (ct_schemes[i] != sig_schemes[g]), BLS_ERR_SIG_IDENTITY, BLS_ERR_PK_IDENTITY,
// BLS_OK.  An OK item gets its pair (the G1 member first: (sig, u) for SG = 1, (u, sig) for SG = 2) in the one-pair workspace and
// flag PV_RUN; every other item flag PV_ZERO, so that k_pairing_value walks nothing for it.
template <int SG>
__global__ void k_timecrypt_prepare(size_t n, size_t n_groups, const uint64_t* item_offs, const uint8_t* us, const uint8_t* sigs, int fmt,
                                    const uint8_t* sig_schemes, const uint8_t* ct_schemes, const int32_t* dec_u, const int32_t* dec_sig, uint32_t* pairs,
                                    int32_t* flag, int32_t* status);
// the tail of an item whose status is OK on entry (timecrypt_open_frame, timecrypt_check): its frame, pt_range and final status --
// BLS_ERR_BAD_FRAME, BLS_ERR_INVALID_SIGNATURE or BLS_OK.  Every other item: pt_range (0, 0), nothing else is touched.
template <int SG>
__global__ void k_timecrypt_open(size_t n, const uint8_t* gt, const uint8_t* us, int fmt, const uint8_t* vs, const uint8_t* ws, const uint64_t* w_offs,
                                 uint8_t* frames, uint64_t* pt_range, int32_t* status);
#endif
