// translation unit: k_millerf_rows1, the lane-split Miller accumulator of ONE TABLED pair per item (sigset.cuh) -- the pairing values
// of a Bls12381G2Impl signature set with rows, from BLSGPU_VALUE_SPLIT_MIN items up.  A unit of its own: the kernels of tu_millerf.hip
// and tu_lines.hip stay what they are.
#define BLS_TU_MILLERF_ROWS1 1
#include "kernels.cuh"
#include "timecrypt.cuh"
#include "sigset.cuh"

// The two operations of the kernel are functions whose arguments are scalars, as k_millerfp3's (kernels.cuh): each fits the register
// file on its own and nothing travels by reference.
static __device__ __noinline__ void rows1_sqr_fn(lds_u32* sh) {
  fp12_t<hfp2> a, r;
  sh_ld_f12(a, sh);
  fp12_sqr_body(r, a);
  sh_st_f12(sh, r);
}
// A <- A * (n0 + (c xP) w^2 + (yP, 0) w^3) with (n0, c) this lane's components of row e of the item's entry (off: the entry's word
// offset in the table plus FP_NL on the odd lane, 32 bits; the base is wave-uniform) and P = (xP, yP) item i of the one-pair
// workspace, read again per entry: held across the squaring it would travel through scratch.  The operands are those k_linesp_keyed
// stores (pairing.cuh miller_line3_row) and f12_sh_mul_line3_fn consumes.
static __device__ __noinline__ void rows1_mul_fn(lds_u32* sh, const uint32_t* table, uint32_t off, const uint32_t* pairs, size_t stride, uint32_t i, int e) {
  hfp2 n0, c, l0, l2, l3;
  fp x, y;
  {
    gc_u32* tr = uni_global(table);
    const uint32_t o = off + uni_u32((uint32_t)e) * (4 * FP_NL);
#pragma unroll
    for (int k = 0; k < FP_NL; k++) {
      n0.v.l[k] = (int32_t)g_ld(tr, o + k);
      c.v.l[k] = (int32_t)g_ld(tr, o + 2 * FP_NL + k);
    }
  }
  {
    stride = uni_sz(stride);
    gc_u32* row = uni_global(pairs);
#pragma unroll
    for (int k = 0; k < FP_NL; k++) {
      x.l[k] = (int32_t)g_ld(row, i);
      y.l[k] = (int32_t)g_ld(row + (size_t)W1 * stride, i);
      row += stride;
    }
  }
  miller_line3_row(l0, l2, l3, n0, c, x, y);
  f12_sh_mul_line3(sh, l0, l2, l3);
}

// One lane pair per item; the host keeps n below 2^30 (the item's 32-bit byte offset in a workspace row) and the table below 2^32 bytes.
__global__ void __launch_bounds__(BLS_BLOCK, BLS_SPLIT_WAVES) __attribute__((disable_tail_calls))
k_millerf_rows1(size_t n, size_t first, size_t count, const uint32_t* pairs, const int32_t* flag, const uint32_t* table, const uint32_t* ent, uint32_t* fws) {
  const uint32_t t = blockIdx.x * BLS_BLOCK + threadIdx.x;
  const size_t j = t >> 1;
  if (j >= count) return;
  const size_t i = first + j;                          // the item's index in the BATCH: flag, ent, the pairs and fws are indexed by it
  if (flag[i] != PV_RUN) return;                       // before any table read: only a PV_RUN item has an entry with usable rows
  __shared__ uint32_t fsh[F12_SH_WORDS * BLS_BLOCK];   // the accumulator, packed (tower_split.cuh)
  f12_sh acc = {lds_column(fsh)};
  acc_one(acc);
  const uint32_t off = ent[i] * (uint32_t)(MILLER_ENTRIES * 4 * FP_NL) + (lane_hi() ? FP_NL : 0);
  for (int e = 0; e < MILLER_ENTRIES; e++) {
    if (e > 0 && !miller_entry_is_add(e)) rows1_sqr_fn(acc.sh);
    rows1_mul_fn(acc.sh, table, off, pairs, n, (uint32_t)i, e);
  }
  fp12_t<hfp2> f;
  sh_ld_f12(f, acc.sh);
  fp12_conj(f, f);
  ws_st_hfp12(fws, n, i, f);
}
