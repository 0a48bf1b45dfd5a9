// TEST-ONLY harness for tests/test_hostsim_pairing_doors.py: the per-item bodies of k_prepare_hashed and k_prepare_proof
// (agora-blsful_amd/csrc/verify.cuh prepare_hashed_item, prepare_proof_item) and a restatement of k_pairs2_to_affine's as plain host
// C++ with the bound tracker on, followed by the host Miller loop and final verdict -- with the plain -g2 line table (G2NEG_LINES, what
// k_miller2s and the wave-cooperative kernel read for fixed_g2 = 1) on the one-lane tower and with its merged form (G2NEG_LINES_N,
// what k_lines2s reads) on the lane-split tower.  Never linked into libblsgpu.so.
#include <string.h>
#include "../../agora-blsful_amd/csrc/verify.cuh"
#include "../../agora-blsful_amd/csrc/tower_split.cuh"

static void raw_fp2(fp2& r, const uint32_t* w) { fp_from_raw(r.c0, w); fp_from_raw(r.c1, w + 12); }
static void load_g1_jac(g1_jac& p, const uint32_t* w) { fp_from_raw(p.x, w); fp_from_raw(p.y, w + 12); fp_from_raw(p.z, w + 24); }
static void load_g2_jac(g2_jac& p, const uint32_t* w) { raw_fp2(p.x, w); raw_fp2(p.y, w + 24); raw_fp2(p.z, w + 48); }
static void to_split(aff<hfp2>& r, const g2_aff& q) { r.x.c[0] = q.x.c0; r.x.c[1] = q.x.c1; r.y.c[0] = q.y.c0; r.y.c[1] = q.y.c1; r.inf = false; }

// what run_pairing2 computes from an item's pair slots: fixed_g2 = 1 (pair 1's G2 member is -g2, lines from the tables) or 0 (two
// general pairs).  The slots hold coordinates only (ws_st_pair / ws_ld_pair drop the `inf` flag), so it is cleared here too.
// Returns the verdict when the one-lane loop over the plain table and the lane-split loop over the merged one agree,
// -100 - (the lane-split verdict) otherwise.
static int verdict2(int fixed_g2, g1_aff* P, g2_aff* Q) {
  P[0].inf = P[1].inf = false;
  Q[0].inf = Q[1].inf = false;
  aff<hfp2> QQ[2];
  to_split(QQ[0], Q[0]);
  to_split(QQ[1], Q[1]);
  fp12 f;
  fp12_t<hfp2> fs;
  if (fixed_g2) {
    miller_loop_fixed_g2(f, P[0], Q[0], P[1], G2NEG_LINES);
    miller_loop_fixed_g2_merged(fs, P[0], QQ[0], P[1], G2NEG_LINES_N);
  } else {
    miller_loop<2>(f, P, Q);
    miller_loop2_merged(fs, P, QQ);
  }
  const int v = pairing_verdict(f), vs = pairing_verdict(fs);
  return v == vs ? v : -100 - vs;
}

// The body of k_pairs2_to_affine (csrc/kernels.cuh) RESTATED: hoisting it out of the kernel changed the kernel's register and
// scratch figures, so the kernel keeps its text and this copy must be kept in step with it by hand.  Both pairs to affine; with both
// pairs trivial the fixed product e(g1, -g2) * e(-g1, -g2), which is one; with exactly one trivial pair BLS_ERR_INVALID_SIGNATURE
// and no pairs.
static int pairs2_item(g1_aff* P, g2_aff* Q, const g1_jac& a1, const g2_jac& a2, const g1_jac& b1, const g2_jac& b2) {
  const bool ta = jac_is_inf(a1) || jac_is_inf(a2), tb = jac_is_inf(b1) || jac_is_inf(b2);
  if (ta != tb) return BLS_ERR_INVALID_SIGNATURE;
  if (ta) {
    fp_load(P[0].x, G1_GEN_X);
    fp_load(P[0].y, G1_GEN_Y);
    P[0].inf = false;
    g1_neg_gen(P[1]);
    g2_neg_gen(Q[0]);
    g2_neg_gen(Q[1]);
  } else {
    g1g2_to_aff(P[0], Q[0], a1, a2);
    g1g2_to_aff(P[1], Q[1], b1, b2);
  }
  return BLS_OK;
}

extern "C" {
// blsgpu_core_verify_hashed on one item: RAW_PROJ points
int hs_door_hashed(int sig_group, const uint32_t* pk, const uint32_t* sig, const uint32_t* h) {
  g1_aff P[2];
  g2_aff Q[2];
  int st;
  if (sig_group == 1) {
    g2_jac k; g1_jac s, hh;
    load_g2_jac(k, pk); load_g1_jac(s, sig); load_g1_jac(hh, h);
    st = prepare_hashed_item(P, Q, k, s, hh);
  } else {
    g1_jac k; g2_jac s, hh;
    load_g1_jac(k, pk); load_g2_jac(s, sig); load_g2_jac(hh, h);
    st = prepare_hashed_item(P, Q, k, s, hh);
  }
  return st != BLS_OK ? st : verdict2(sig_group == 1 ? 1 : 0, P, Q);
}
// blsgpu_sig_proof_verify_batch on one item: RAW_PROJ points, y as 8 little-endian words
int hs_door_proof(int sig_group, const uint32_t* u, const uint32_t* v, const uint32_t* pk, const uint32_t* y, const uint8_t* msg,
                  uint32_t len, const uint8_t* dst, uint32_t dlen) {
  g1_aff P[2];
  g2_aff Q[2];
  int st;
  if (sig_group == 1) {
    g1_jac uu, vv; g2_jac k;
    load_g1_jac(uu, u); load_g1_jac(vv, v); load_g2_jac(k, pk);
    st = prepare_proof_item(P, Q, uu, vv, k, y, msg, len, dst, dlen);
  } else {
    g2_jac uu, vv; g1_jac k;
    load_g2_jac(uu, u); load_g2_jac(vv, v); load_g1_jac(k, pk);
    st = prepare_proof_item(P, Q, uu, vv, k, y, msg, len, dst, dlen);
  }
  return st != BLS_OK ? st : verdict2(sig_group == 1 ? 1 : 0, P, Q);
}
// blsgpu_pairing2_check_batch on one item: the status before k_status_to_flag (0 <=> the product is one)
int hs_door_pairs2(const uint32_t* g1a, const uint32_t* g2a, const uint32_t* g1b, const uint32_t* g2b) {
  g1_aff P[2];
  g2_aff Q[2];
  g1_jac a1, b1; g2_jac a2, b2;
  load_g1_jac(a1, g1a); load_g2_jac(a2, g2a); load_g1_jac(b1, g1b); load_g2_jac(b2, g2b);
  const int st = pairs2_item(P, Q, a1, a2, b1, b2);
  return st != BLS_OK ? st : verdict2(0, P, Q);
}
}
