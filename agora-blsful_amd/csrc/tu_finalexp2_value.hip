// translation unit: k_finalexp2s_value, the final exponentiation of the lane-split batch path ended as a VALUE with its Gt bytes
// (timecrypt.cuh) -- the pairing values of blsgpu_pairing_batch, blsgpu_timecrypt_open_batch and the two calls over a signature set
// from BLSGPU_VALUE_SPLIT_MIN items up.  The operations are the fx_* functions of kernels.cuh's BLS_TU_FINALEXP2 section, compiled
// here a second time: a unit of its own, so that k_finalexp2s and k_finalexp_seg (tu_finalexp2.hip) stay what they are.
#define BLS_TU_FINALEXP2_VALUE 1
#pragma clang diagnostic ignored "-Wunused-function"   // the verdict's comparisons (fx_is_one, fx_eq_conj) and the six-power finish have no caller here
#include "kernels.cuh"
#include "timecrypt.cuh"

// Gt one or 576 zero bytes (coop_gt_const's bytes) by the item's own lane pair: 144 32-bit words, every other one per lane
__device__ __forceinline__ void fx_gt_const(uint8_t* out, bool zero) {
  for (int w = (int)(threadIdx.x & 1u); w < GT_BYTES / 4; w += 2) {
    const uint32_t v = (w == 11 && !zero) ? 0x01000000u : 0u;      // byte 47 = 1
    __builtin_memcpy(out + 4 * w, &v, 4);
  }
}
// out[0, 576) <- A.  The packed accumulator is in tower order and holds reduced coefficients; tower slot j is the coefficient over
// w^gt_tower_wpow(j), the even lane holds its real part and the odd lane its imaginary part: each lane converts its six Fp out of
// Montgomery form and stores 48 consecutive bytes per coefficient as twelve byte-swapped words (coop_gt_put), from registers.
static __device__ __noinline__ void fx_export(lds_u32* sh, uint8_t* out) {
  const bool hi = lane_hi();
#pragma nounroll
  for (int j = 0; j < 6; j++) {
    fp x;
    sh_ld_fp(x, sh, 13 * j);
    coop_gt_put(out + gt_part_offset(gt_tower_wpow(j), hi), x);
  }
}

// k_finalexp2s's body and launch shape; the ending multiplies by f once more and exports
__global__ void __launch_bounds__(BLS_BLOCK, BLS_SPLIT_WAVES) __attribute__((disable_tail_calls))
k_finalexp2s_value(size_t n, size_t first, size_t count, const uint32_t* fws, uint32_t* vp, size_t lanes, const int32_t* flag, uint8_t* out_gt) {
  const uint32_t t = blockIdx.x * BLS_BLOCK + threadIdx.x;
  const size_t j = t >> 1;
  if (j >= count) return;
  const size_t i = first + j;
  uint8_t* out = out_gt + (size_t)GT_BYTES * i;
  const int fl = flag[i];
  if (fl != PV_RUN) {
    fx_gt_const(out, fl == PV_ZERO);
    return;
  }
  __shared__ uint32_t ash[F12_SH_WORDS * BLS_BLOCK];
  lds_u32* sh = lds_column(ash);
  {
    fp12_t<hfp2> f;
    ws_ld_hfp12(f, fws, n, i);
    fp12_reduce(f, f);       // the Miller kernel's conjugate carries negated limbs
    sh_st_f12(sh, f);
  }
  // easy part: f^((p^6 - 1)(p^2 + 1))
  fx_store(sh, vp, lanes, t, 1);                 // fin
  fx_inv(sh);
  fx_store(sh, vp, lanes, t, 0);                 // t = 1 / fin
  fx_load(sh, vp, lanes, t, 1, FX_CONJ);
  fx_mul(sh, vp, lanes, t, 0, FX_PLAIN);         // f = conj(fin) / fin
  fx_store(sh, vp, lanes, t, 1);
  fx_frob2(sh);
  fx_mul(sh, vp, lanes, t, 1, FX_PLAIN);         // f = f^(p^2) f
  fx_store(sh, vp, lanes, t, 1);                 // slot 1: f for the rest of the kernel
  // hard part: (x-1)^2 (x+p) (x^2+p^2-1) + 3
  fx_pow_x(sh, vp, lanes, t);
  fx_mul(sh, vp, lanes, t, 1, FX_CONJ);          // t = f^(x-1)
  fx_store(sh, vp, lanes, t, 0);
  fx_pow_x(sh, vp, lanes, t);
  fx_mul(sh, vp, lanes, t, 0, FX_CONJ);          // t = t^(x-1)
  fx_store(sh, vp, lanes, t, 0);
  fx_pow_x(sh, vp, lanes, t);
  fx_mul(sh, vp, lanes, t, 0, FX_FROB1);         // t = t^(x+p)
  fx_store(sh, vp, lanes, t, 0);
  fx_pow_x(sh, vp, lanes, t);
  fx_pow_x(sh, vp, lanes, t);                    // t^(x^2)
  fx_mul(sh, vp, lanes, t, 0, FX_FROB2);
  fx_mul(sh, vp, lanes, t, 0, FX_CONJ);          // t = t^(x^2+p^2-1)
  fx_store(sh, vp, lanes, t, 0);
  fx_load(sh, vp, lanes, t, 1, FX_PLAIN);
  fx_cyc_sqr(sh);
  fx_mul(sh, vp, lanes, t, 0, FX_PLAIN);         // t f^2
  fx_mul(sh, vp, lanes, t, 1, FX_PLAIN);         // t f^3: the value
  fx_export(sh, out);
}
