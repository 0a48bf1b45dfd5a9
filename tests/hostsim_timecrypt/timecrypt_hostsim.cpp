// TEST-ONLY harness for tests/test_hostsim_timecrypt.py: the pairing-value functions of agora-blsful_amd/csrc/timecrypt.cuh --
// coop_miller1, coop_final_value (coop.cuh), coop_gt_bytes -- and the time-lock tail (timecrypt_open_frame, timecrypt_check) compiled
// as plain host C++ with the bound tracker on.  The wave model
// (32 threads, one per lane pair, a tracked LDS block) is the one of tests/hostsim_coop, whose source this file includes as it is;
// the functions under test are the source text the device compiles.  Never linked into libblsgpu.so.
#include "../hostsim_coop/coop_hostsim.cpp"

#define __device__ static
#define __forceinline__ inline
#define __noinline__ __attribute__((noinline))
#include "../../agora-blsful_amd/csrc/timecrypt.cuh"
#undef __device__
#undef __forceinline__
#undef __noinline__

extern "C" {
// the body of k_pairing_value on one item: six limb vectors (P.x, P.y, Q.x.c0, Q.x.c1, Q.y.c0, Q.y.c1), declared reduced as
// hs_coop_pairing declares them; out = the 576 Gt bytes.  A tracked-bound violation aborts.
int hs_pairing_value(const int32_t* in, uint8_t* out) {
  hs_reset_lds(0x7fffffffu);
  g_strict = false;              // the product rounds multiply the second pair's job slots, which nobody stages (as coop_miller2's table pair)
  g1_aff P;
  aff<hfp2> Q;
  hs_in_fp(P.x, in, 0);
  hs_in_fp(P.y, in, 1);
  hs_in_fp(Q.x.c[0], in, 2);
  hs_in_fp(Q.x.c[1], in, 3);
  hs_in_fp(Q.y.c[0], in, 4);
  hs_in_fp(Q.y.c[1], in, 5);
  P.inf = false;
  Q.inf = false;
  hs_run_wave([&](int p) {
    threadIdx.x = 2 * p;
    coop_shared& S = *(coop_shared*)g_lds;
    coop_miller1(S, P, Q);
    coop_final_value(S);
    coop_gt_bytes(out, S.t);
  });
  return 0;
}
// what a lane of k_timecrypt_open does for an item whose status is OK on entry: gt = the 576 bytes of K, v = 32 bytes, w[0, len), u = a
// RAW_PROJ point of the key group of sg (blst words).  frame receives len bytes, range = (offset, length); returns the status.
int hs_timecrypt_open(int sg, const uint8_t* gt, const uint8_t* v, const uint8_t* w, uint64_t len, const uint32_t* u, uint8_t* frame, uint64_t* range) {
  uint32_t r[8];
  range[0] = range[1] = 0;
  uint64_t off = 0, plen = 0;
  int st = timecrypt_open_frame(frame, w, len, gt, v, &off, &plen, r);
  if (st != BLS_OK) return st;
  bool ok;
  if (sg == 1) {
    g2_jac a;
    g2_aff ga;
    fp_from_raw(a.x.c0, u); fp_from_raw(a.x.c1, u + 12); fp_from_raw(a.y.c0, u + 24); fp_from_raw(a.y.c1, u + 36);
    fp_from_raw(a.z.c0, u + 48); fp_from_raw(a.z.c1, u + 60);
    fp2_load(ga.x, G2_GEN_X);
    fp2_load(ga.y, G2_GEN_Y);
    ga.inf = false;
    ok = timecrypt_check<2>(ga, r, a);
  } else {
    g1_jac a;
    g1_aff ga;
    fp_from_raw(a.x, u); fp_from_raw(a.y, u + 12); fp_from_raw(a.z, u + 24);
    fp_load(ga.x, G1_GEN_X);
    fp_load(ga.y, G1_GEN_Y);
    ga.inf = false;
    ok = timecrypt_check<1>(ga, r, a);
  }
  if (!ok) return BLS_ERR_INVALID_SIGNATURE;
  range[0] = off;
  range[1] = plen;
  return BLS_OK;
}
// coop_gt_bytes alone on an Fp12 given as twelve reduced limb vectors in the order of coop_f12 (w^0 .. w^5, real then imaginary)
int hs_gt_bytes(const int32_t* in, uint8_t* out) {
  hs_reset_lds(0x7fffffffu);
  g_strict = true;
  hs_run_wave([&](int p) {
    threadIdx.x = 2 * p;
    coop_shared& S = *(coop_shared*)g_lds;
    if (p < 6) {
      hfp2 x;
      hs_in_fp(x.c[0], in, 2 * p);
      hs_in_fp(x.c[1], in, 2 * p + 1);
      coop_st(S.t.c[p], x);
    }
    __syncthreads();
    coop_gt_bytes(out, S.t);
  });
  return 0;
}
}
