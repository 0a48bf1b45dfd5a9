// translation unit: self-test kernel of blsgpu_debug_field_op (debug_ops.h) for the wave-cooperative pairing engine (coop.cuh):
// one item per 64-lane workgroup, the functions of coop.cuh called on a coop_shared that is first overwritten with the record's
// `fill` word, so that nothing an operation returns can depend on what LDS held.
#include "debug_ops_io.cuh"
#include "coop.cuh"

// record order is the tower order c0.a0, c0.a1, c0.a2, c1.a0, c1.a1, c1.a2 -> powers of w 0, 2, 4, 1, 3, 5 (as k_finalexp_coop)
static __device__ __forceinline__ int dbg_coop_pw(int k) { return (k < 3) ? 2 * k : 2 * (k - 3) + 1; }
// Fp12 at Fp2 numbers k0 .. k0 + 5 of a record <-> a coop_f12, lane pair k moving coefficient k
static __device__ __forceinline__ void dbg_coop_ld12(coop_f12& f, const int32_t* rec, int k0) {
  const int k = coop_pair();
  if (k < 6) {
    hfp2 x;
    dbg_ld2(x, rec, k0 + k);
    coop_st(f.c[dbg_coop_pw(k)], x);
  }
}
static __device__ __forceinline__ void dbg_coop_st12(int32_t* rec, const coop_f12& f) {
  const int k = coop_pair();
  if (k < 6) {
    hfp2 x;
    coop_ld(x, f.c[dbg_coop_pw(k)]);
    dbg_st2(rec, k, x);
  }
}
// the staged jobs S.job[k][0 .. per - 1][0 .. 1] (k = 0, 1) from Fp2 number k0 on, and their results to Fp2 number k0 on
static __device__ __forceinline__ void dbg_coop_ld_jobs(coop_shared& S, const int32_t* rec, int k0, int per) {
  for (int t = coop_pair(); t < 4 * per; t += BLS_BLOCK / 2) {
    hfp2 x;
    dbg_ld2(x, rec, k0 + t);
    coop_st(S.job[t / (2 * per)][(t / 2) % per][t & 1], x);
  }
}
static __device__ __forceinline__ void dbg_coop_st_res(int32_t* rec, int k0, const coop_shared& S, int per) {
  const int t = coop_pair();
  if (t < 2 * per) {
    hfp2 x;
    coop_ld(x, S.res[t / per][t % per]);
    dbg_st2(rec, k0 + t, x);
  }
}

__global__ void __launch_bounds__(BLS_BLOCK, 2) k_dbg_coop(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out) {
  __shared__ coop_shared S;
  const size_t j = blockIdx.x;
  if (j >= n) return;
  const int32_t* x = in + j * (size_t)rec_in;
  int32_t* y = out + j * (size_t)rec_out;
  const int par = x[rec_in - 2];                 // alias / set / njobs of the rows that have one (the word before `fill`)
  const uint32_t fill = (uint32_t)x[rec_in - 1];
  for (int w = threadIdx.x; w < (int)(sizeof(coop_shared) / 4); w += BLS_BLOCK) ((uint32_t*)&S)[w] = fill;
  __syncthreads();
  const int me = coop_pair();
  const coop_f12* res = &S.f;
  if (op != DBG_COOP_JOBS) dbg_coop_ld12(S.f, x, 0);
  switch (op) {
    case DBG_COOP_MUL: {             // a = S.f, b = S.u; alias 0: dst = S.t, 1: dst = a, 2: dst = b (S.v keeps b for the chain)
      dbg_coop_ld12(S.u, x, 6);
      dbg_coop_ld12(S.v, x, 6);
      __syncthreads();
      coop_f12& dst = par == 1 ? S.f : par == 2 ? S.u : S.t;
      for (int k = 0; k < reps; k++) {
        coop_mul(S, dst, S.f, S.u);
        if (k + 1 < reps) {
          if (par != 1) coop_copy(S.f, dst);
          if (par == 2) coop_copy(S.u, S.v);
        }
      }
      res = &dst;
      break;
    }
    case DBG_COOP_SQR:
      __syncthreads();
      for (int k = 0; k < reps; k++) {
        coop_sqr(S, S.u, S.f);
        if (k + 1 < reps) coop_copy(S.f, S.u);
      }
      res = &S.u;
      break;
    case DBG_COOP_MUL_LINE:          // the line in set `par`; the other set holds the same coefficients rotated by one place
      if (me < 3) {
        hfp2 l;
        dbg_ld2(l, x, 6 + me);
        coop_st(S.line[par & 1][me], l);
        coop_st(S.line[1 - (par & 1)][(me + 2) % 3], l);
      }
      __syncthreads();
      for (int k = 0; k < reps; k++) coop_mul_line(S, S.f, par & 1);
      break;
    case DBG_COOP_CYC_SQR: {         // alias 0: dst = S.t, 1: dst = a
      __syncthreads();
      coop_f12& dst = par == 1 ? S.f : S.t;
      for (int k = 0; k < reps; k++) {
        coop_cyc_sqr(S, dst, S.f);
        if (k + 1 < reps && par != 1) coop_copy(S.f, dst);
      }
      res = &dst;
      break;
    }
    case DBG_COOP_POW_X:
      __syncthreads();
      coop_pow_x(S, S.t, S.f);
      res = &S.t;
      break;
    case DBG_COOP_CONJ:
      __syncthreads();
      coop_conj(S.u, S.f);
      res = &S.u;
      break;
    case DBG_COOP_FROB1:
      __syncthreads();
      coop_frob<1>(S.v, S.f);
      res = &S.v;
      break;
    case DBG_COOP_FROB2:
      __syncthreads();
      coop_frob<2>(S.v, S.f);
      res = &S.v;
      break;
    case DBG_COOP_FINAL_EASY:
      __syncthreads();
      coop_final_easy(S);
      break;
    default:
      break;
  }
  if (op == DBG_COOP_JOBS) {         // twelve operand pairs in, the twelve result slots out (an uncomputed one still holds `fill`)
    dbg_coop_ld_jobs(S, x, 0, 6);
    coop_jobs(S, par);
    dbg_coop_st_res(y, 0, S, 6);
    return;
  }
  if (op == DBG_COOP_SQR_MUL_JOBS) {
    dbg_coop_ld_jobs(S, x, 6, 5);
    coop_sqr_with_jobs(S, S.f);
    dbg_coop_st12(y, S.f);
    dbg_coop_st_res(y, 6, S, 5);
    return;
  }
  if (op == DBG_COOP_LINE_MUL_JOBS) {
    if (me < 3) {
      hfp2 l;
      dbg_ld2(l, x, 6 + me);
      coop_st(S.line[par & 1][me], l);
      coop_st(S.line[1 - (par & 1)][(me + 2) % 3], l);
    }
    dbg_coop_ld_jobs(S, x, 9, 6);
    coop_mul_line_with_jobs(S, S.f, par & 1);
    dbg_coop_st12(y, S.f);
    dbg_coop_st_res(y, 6, S, 6);
    return;
  }
  if (op == DBG_COOP_FINAL_VERDICT) {
    __syncthreads();
    const int st = coop_final_verdict(S);
    if (threadIdx.x < FP_NL) y[threadIdx.x] = threadIdx.x == 0 ? st : 0;
    return;
  }
  __syncthreads();
  dbg_coop_st12(y, *res);
}
