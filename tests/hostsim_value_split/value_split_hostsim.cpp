// TEST-ONLY harness for tests/test_hostsim_value_split.py: what the host build can run of the pairing values on the lane-split
// kernels (agora-blsful_amd/csrc/tu_finalexp2_value.hip, tu_millerf_rows1.hip), as plain host C++ with the bound tracker on.
//   * the value ending and the byte export of k_finalexp2s_value: pairing.cuh final_exp_parts -- the chain the kernel's fx_* operations
//     follow operation for operation (kernels.cuh) -- on the lane-split Fp2 of tower_split.cuh, then the kernel's own ending (f^2 by
//     the cyclotomic squaring, times t, times f once more) and fx_export's placement: every tower slot through gt_tower_wpow,
//     gt_part_offset and coop_gt_put (timecrypt.cuh), the even lane's part and the odd lane's;
//   * the per-entry loop of k_millerf_rows1: a squaring on every non-addition entry after the first, then the row's line
//     n0 + (c xP) w^2 + (yP, 0) w^3 (pairing.cuh miller_line3_row, the rows read with fp2_load as a table's are) multiplied in by
//     tower.cuh fp12_mul_by_line_body, whose sequence f12_sh_mul_line3 follows; conj(f) leaves as the kernel leaves it.
// Not run here, because they exist on the device only: the packed LDS accumulator and the functions that stream through it
// (sh_ld_fp / sh_st_fp, fx_load / fx_store / fx_mul, f12_sh_mul_line3, the value store in global memory).
// The wave model and hs_in_fp are those of tests/hostsim_coop, whose source this file includes as it is.  Never linked into libblsgpu.so.
#include "../hostsim_coop/coop_hostsim.cpp"

#define __device__ static
#define __forceinline__ inline
#define __noinline__ __attribute__((noinline))
#include "../../agora-blsful_amd/csrc/timecrypt.cuh"
#undef __device__
#undef __forceinline__
#undef __noinline__

// fx_export for both lanes of the pair: v in tower order, reduced coefficients
static void hs_export(uint8_t* out, const fp12_t<hfp2>& v) {
  const hfp2* co[6] = {&v.c0.a0, &v.c0.a1, &v.c0.a2, &v.c1.a0, &v.c1.a1, &v.c1.a2};
  for (int j = 0; j < 6; j++)
    for (int hi = 0; hi < 2; hi++) coop_gt_put(out + gt_part_offset(gt_tower_wpow(j), hi != 0), co[j]->c[hi]);
}
// fin (what the Miller kernel left, reduced as the kernel reduces it on entry) -> the 576 bytes of t f^3
static void hs_value(uint8_t* out, const fp12_t<hfp2>& fin) {
  fp12_t<hfp2> f, t, u;
  final_exp_parts(t, f, fin);
  fp12_cyclotomic_sqr(u, f);
  fp12_mul(u, u, t);             // t f^2, where k_finalexp2s stops
  fp12_mul(u, u, f);             // t f^3: the value
  fp12_reduce(u, u);
  hs_export(out, u);
}

extern "C" {
// in: twelve limb vectors, an Fp12 in tower order (c0.a0.c0, c0.a0.c1, c0.a1.c0, ...), declared reduced; out = 576 bytes
int hs_finalexp_value(const int32_t* in, uint8_t* out) {
  fp12_t<hfp2> fin;
  hfp2* co[6] = {&fin.c0.a0, &fin.c0.a1, &fin.c0.a2, &fin.c1.a0, &fin.c1.a1, &fin.c1.a2};
  for (int j = 0; j < 6; j++) {
    hs_in_fp(co[j]->c[0], in, 2 * j);
    hs_in_fp(co[j]->c[1], in, 2 * j + 1);
  }
  hs_value(out, fin);
  return 0;
}
// xy: the limb vectors of P = (xP, yP), declared reduced; rows: 68 rows of 4 FP_NL words (n0.c0, n0.c1, c.c0, c.c1), the *_LINES_N
// layout.  out_f = the export of conj(f) as the kernel stores it, out_value = the 576 bytes of its final exponentiation.
int hs_rows1(const int32_t* xy, const uint32_t* rows, uint8_t* out_f, uint8_t* out_value) {
  fp x, y;
  hs_in_fp(x, xy, 0);
  hs_in_fp(y, xy, 1);
  fp12_t<hfp2> f, r;
  fp12_one(f);
  for (int e = 0; e < MILLER_ENTRIES; e++) {
    if (e > 0 && !miller_entry_is_add(e)) {
      fp12_sqr_body(r, f);
      f = r;
    }
    hfp2 n0, c, l0, l2, l3;
    fp2_load(n0, rows + (size_t)e * 4 * FP_NL);
    fp2_load(c, rows + (size_t)e * 4 * FP_NL + 2 * FP_NL);
    miller_line3_row(l0, l2, l3, n0, c, x, y);
    fp12_mul_by_line_body(f, l0, l2, l3);
  }
  fp12_conj(r, f);
  fp12_reduce(r, r);
  hs_export(out_f, r);
  hs_value(out_value, r);
  return 0;
}
}
