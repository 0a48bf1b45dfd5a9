// TEST-ONLY harness for tests/test_hostsim_coop.py and tests/test_field_cases.py: the wave-cooperative pairing engine
// (agora-blsful_amd/csrc/coop.cuh) compiled as plain host C++ with the bound tracker on.  A wave runs as 32 threads, one per lane
// pair (threadIdx.x = 2 * lane pair; the host hfp2 holds both halves), __syncthreads is a barrier, and the LDS block is a static
// buffer with one tracker record per Fp slot, so that an element keeps its tracked bounds on its way through LDS and a read of a
// slot nobody wrote aborts.  The round functions are the source text the device compiles.  Never linked into libblsgpu.so.
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>
#include "../../agora-blsful_amd/csrc/verify.cuh"
#include "../../agora-blsful_amd/csrc/tower_split.cuh"
#include "../../agora-blsful_amd/csrc/debug_ops.h"

#ifndef BLS_TRACK_BOUNDS
#error "build with -DBLS_TRACK_BOUNDS"
#endif

#define BLS_BLOCK 64
#define COOP_PAIRS (BLS_BLOCK / 2)
struct hs_dim3 {
  unsigned x;
};
static thread_local hs_dim3 threadIdx;
static pthread_barrier_t g_barrier;
static inline void __syncthreads() { pthread_barrier_wait(&g_barrier); }

// the LDS block and its tracker records (one per FP_NL words); 16 Ki words hold a coop_shared (checked below)
#define HS_LDS_WORDS 16384
struct hs_trk {
  double lb, vb;
  bool nn, written;
};
alignas(64) static uint32_t g_lds[HS_LDS_WORDS];
static hs_trk g_trk[HS_LDS_WORDS / FP_NL + 1];
static bool g_strict = true;
static hs_trk& hs_trk_of(const uint32_t* p) {
  const ptrdiff_t w = p - g_lds;
  if (w < 0 || w + FP_NL > HS_LDS_WORDS || w % FP_NL) {
    fprintf(stderr, "coop_hostsim: an Fp slot outside the LDS block or off the %d-word grid (word %ld)\n", FP_NL, (long)w);
    abort();
  }
  return g_trk[w / FP_NL];
}
static inline void coop_trk_ld(fp& r, const uint32_t* p) {
  const hs_trk& t = hs_trk_of(p);
  if (!t.written) {
    // coop_miller2 lets the product rounds multiply job slots of the table pair that nobody staged (their results are not read): the
    // pairing export tolerates that and tracks such a value as nothing; a row of the operation table must not read what nobody wrote
    if (!g_strict) {
      r.lb = r.vb = 0;
      r.nn = false;
      return;
    }
    fprintf(stderr, "coop_hostsim: lane pair %u reads LDS word %ld, which nobody wrote\n", threadIdx.x >> 1, (long)(p - g_lds));
    abort();
  }
  r.lb = t.lb;
  r.vb = t.vb;
  r.nn = t.nn;
}
static inline void coop_trk_st(const uint32_t* p, const fp& a) {
  hs_trk& t = hs_trk_of(p);
  t.lb = a.lb;
  t.vb = a.vb;
  t.nn = a.nn;
  t.written = true;
}

#define __device__ static
#define __forceinline__ inline
#define __noinline__ __attribute__((noinline))
#include "../../agora-blsful_amd/csrc/coop.cuh"
#undef __device__
#undef __forceinline__
#undef __noinline__

static_assert(sizeof(coop_shared) <= sizeof(g_lds), "the LDS block holds a coop_shared");
static_assert(offsetof(coop_shared, flag) % (4 * FP_NL) == 0 && sizeof(coop_f12) % (4 * FP_NL) == 0, "every Fp slot lies on the FP_NL-word grid");

// ---- one record of the operation table on one wave, as k_dbg_coop (csrc/tu_debug_ops4.hip) runs it
struct hs_args {
  int op, reps;
  const int32_t* in;
  const double *lb, *vb;
  const int32_t *nn, *par;
  int32_t* out;
};
static void hs_ld2(hfp2& h, const hs_args& A, int k) {
  for (int c = 0; c < 2; c++) {
    fp& r = h.c[c];
    const int v = 2 * k + c;
    for (int i = 0; i < FP_NL; i++) r.l[i] = A.in[v * FP_NL + i];
    r.lb = A.lb[v];
    r.vb = A.vb[v];
    r.nn = A.nn[v] != 0;
  }
}
static void hs_st2(int32_t* out, int k, const hfp2& h) {
  for (int c = 0; c < 2; c++)
    for (int i = 0; i < FP_NL; i++) out[(2 * k + c) * FP_NL + i] = h.c[c].l[i];
}
static int hs_pw(int k) { return (k < 3) ? 2 * k : 2 * (k - 3) + 1; }
static void hs_ld12(coop_f12& f, const hs_args& A, int k0) {
  const int k = coop_pair();
  if (k < 6) {
    hfp2 x;
    hs_ld2(x, A, k0 + k);
    coop_st(f.c[hs_pw(k)], x);
  }
}
static void hs_st12(int32_t* out, const coop_f12& f) {
  const int k = coop_pair();
  if (k < 6) {
    hfp2 x;
    coop_ld(x, f.c[hs_pw(k)]);
    hs_st2(out, k, x);
  }
}
static void hs_ld_jobs(coop_shared& S, const hs_args& A, int k0, int per) {
  for (int t = coop_pair(); t < 4 * per; t += COOP_PAIRS) {
    hfp2 x;
    hs_ld2(x, A, k0 + t);
    coop_st(S.job[t / (2 * per)][(t / 2) % per][t & 1], x);
  }
}
// results to Fp2 number k0 on; a slot nobody wrote comes back as the words LDS holds (the fill)
static void hs_st_res(int32_t* out, int k0, const coop_shared& S, int per) {
  const int t = coop_pair();
  if (t < 2 * per) {
    const uint32_t* slot = S.res[t / per][t % per];
    for (int i = 0; i < 2 * FP_NL; i++) out[(k0 + t) * 2 * FP_NL + i] = (int32_t)slot[i];
    if (hs_trk_of(slot).written) {       // (a computed result also passes the tracked load)
      hfp2 x;
      coop_ld(x, slot);
    }
  }
}
static void hs_put_line(coop_shared& S, const hs_args& A, int set) {
  const int me = coop_pair();
  if (me < 3) {
    hfp2 l;
    hs_ld2(l, A, 6 + me);
    coop_st(S.line[set & 1][me], l);
    coop_st(S.line[1 - (set & 1)][(me + 2) % 3], l);
  }
}

static void hs_wave(const hs_args& A, int pair) {
  threadIdx.x = 2 * pair;
  coop_shared& S = *(coop_shared*)g_lds;
  const int op = A.op, reps = A.reps, par = A.par[0];
  const coop_f12* res = &S.f;
  if (op != DBG_COOP_JOBS) hs_ld12(S.f, A, 0);
  switch (op) {
    case DBG_COOP_MUL: {
      hs_ld12(S.u, A, 6);
      hs_ld12(S.v, A, 6);
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
    case DBG_COOP_MUL_LINE:
      hs_put_line(S, A, par);
      __syncthreads();
      for (int k = 0; k < reps; k++) coop_mul_line(S, S.f, par & 1);
      break;
    case DBG_COOP_CYC_SQR: {
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
    case DBG_COOP_JOBS:
      hs_ld_jobs(S, A, 0, 6);
      coop_jobs(S, par);
      hs_st_res(A.out, 0, S, 6);
      return;
    case DBG_COOP_SQR_MUL_JOBS:
      hs_ld_jobs(S, A, 6, 5);
      coop_sqr_with_jobs(S, S.f);
      hs_st12(A.out, S.f);
      hs_st_res(A.out, 6, S, 5);
      return;
    case DBG_COOP_LINE_MUL_JOBS:
      hs_put_line(S, A, par);
      hs_ld_jobs(S, A, 9, 6);
      coop_mul_line_with_jobs(S, S.f, par & 1);
      hs_st12(A.out, S.f);
      hs_st_res(A.out, 6, S, 6);
      return;
    case DBG_COOP_FINAL_VERDICT: {
      __syncthreads();
      const int st = coop_final_verdict(S);
      if (pair == 0) {
        for (int i = 0; i < FP_NL; i++) A.out[i] = 0;
        A.out[0] = st;
      }
      return;
    }
    default:
      break;
  }
  __syncthreads();
  hs_st12(A.out, *res);
}

static void hs_reset_lds(uint32_t fill) {
  for (int w = 0; w < HS_LDS_WORDS; w++) g_lds[w] = fill;
  memset(g_trk, 0, sizeof(g_trk));
}
template <class F>
static void hs_run_wave(F body) {
  pthread_barrier_init(&g_barrier, nullptr, COOP_PAIRS);
  std::vector<std::thread> th;
  for (int p = 0; p < COOP_PAIRS; p++) th.emplace_back([=] { body(p); });
  for (auto& t : th) t.join();
  pthread_barrier_destroy(&g_barrier);
}

extern "C" {
// the signature of tests/hostsim hs_field_op; the last parameter of every row is the fill word.  Returns 0, or -1 for an operation
// that is not a row of the wave-cooperative engine.
int hs_coop_op(int op, const int32_t* in, const double* lb, const double* vb, const int32_t* nn, const int32_t* par, int reps, int32_t* out) {
  int n_par = -1;
#define X(name, id, lanes, nin, nout, npar, chain) if (op == id && lanes == 64) n_par = npar;
  BLS_DEBUG_OPS(X)
#undef X
  if (n_par < 1) return -1;
  hs_reset_lds((uint32_t)par[n_par - 1]);
  g_strict = true;
  const hs_args A = {op, reps, in, lb, vb, nn, par, out};
  hs_run_wave([&](int p) { hs_wave(A, p); });
  return 0;
}

// the body of k_pairing_coop_easy (mode 0) / k_pairing_coop (mode 1) on one item: twelve limb vectors (P.x, P.y, Q.x.c0, Q.x.c1, Q.y.c0,
// Q.y.c1 per pair), declared reduced (|value| <= 0.52 p, limbs below 2^28).  mode 0: out = the easy-part value, twelve limb vectors
// in tower order; returns 0.  mode 1: returns the status.
static int g_status;
static void hs_in_fp(fp& r, const int32_t* in, int v) {
  bool nn = true;
  for (int i = 0; i < FP_NL; i++) {
    r.l[i] = in[v * FP_NL + i];
    if (i < FP_NL - 1 && r.l[i] < 0) nn = false;
  }
  r.lb = FP_LB_N;
  r.vb = 0.52;
  r.nn = nn;
}
int hs_coop_pairing(int mode, int fixed_g2, const int32_t* in, int32_t* out) {
  hs_reset_lds(0x7fffffffu);
  g_strict = false;
  g1_aff P[2];
  aff<hfp2> Q[2];
  for (int k = 0; k < 2; k++) {
    hs_in_fp(P[k].x, in, 6 * k);
    hs_in_fp(P[k].y, in, 6 * k + 1);
    hs_in_fp(Q[k].x.c[0], in, 6 * k + 2);
    hs_in_fp(Q[k].x.c[1], in, 6 * k + 3);
    hs_in_fp(Q[k].y.c[0], in, 6 * k + 4);
    hs_in_fp(Q[k].y.c[1], in, 6 * k + 5);
    P[k].inf = false;
    Q[k].inf = false;
  }
  g_status = -1;
  hs_run_wave([&](int p) {
    threadIdx.x = 2 * p;
    coop_shared& S = *(coop_shared*)g_lds;
    coop_miller2(S, P, Q, fixed_g2);
    if (mode == 0) {
      coop_final_easy(S);
      hs_st12(out, S.f);
    } else {
      const int st = coop_final_verdict(S);
      if (p == 0) g_status = st;
    }
  });
  return mode == 0 ? 0 : g_status;
}
}
