// TEST-ONLY harness for tests/test_hostsim_keyset_lines.py: compiles the host side of the per-key line tables of the registered key
// sets (agora-blsful_amd/csrc/keyset.cuh: keyset_lines_entry, keyset_lines_fit; tower.cuh: lines_merge_yy; pairing.cuh:
// miller_loop_tables_merged) as plain host C++ with the bound tracker on, on the host emulation of the lane-split tower
// (tower_split.cuh), and runs the Miller loop fed from TWO tables -- a key's built rows and G2NEGC_LINES_N, what k_lines2s_keyed +
// k_millerf2s compute -- beside the general two-pair loop.  Built twice: as a shared object driven from Python, and -- with
// KEYSET_LINES_HOSTSIM_MAIN -- as a stand-alone program under the address and undefined-behaviour sanitizers that walks the same
// functions over its own inputs.  Never linked into libblsgpu.so.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../agora-blsful_amd/csrc/keyset.cuh"

static void raw_fp2(fp2& r, const uint32_t* w) { fp_from_raw(r.c0, w); fp_from_raw(r.c1, w + 12); }
static void load_g1_jac(g1_jac& p, const uint32_t* w) { fp_from_raw(p.x, w); fp_from_raw(p.y, w + 12); fp_from_raw(p.z, w + 24); }
static void load_g2_jac(g2_jac& p, const uint32_t* w) { raw_fp2(p.x, w); raw_fp2(p.y, w + 24); raw_fp2(p.z, w + 48); }
static void to_split(hfp2& r, const fp2& a) { r.c[0] = a.c0; r.c[1] = a.c1; }
static void to_split(aff<hfp2>& r, const g2_aff& q) { to_split(r.x, q.x); to_split(r.y, q.y); r.inf = false; }

// an entry's table and scratch rows on the host: both lanes' components side by side, as the device's two lanes leave them
struct host_io {
  uint32_t* table;
  uint32_t* scratch;
  uint32_t* at(int e, int slot) const { return (slot < 2 ? table : scratch) + (size_t)e * SHARED_ROW_WORDS + (slot & 1) * (2 * FP_NL); }
  void st(int e, int slot, const hfp2& v) const { fp_store(at(e, slot), v.c[0]); fp_store(at(e, slot) + FP_NL, v.c[1]); }
  void ld(hfp2& v, int e, int slot) const { fp_load(v.c[0], at(e, slot)); fp_load(v.c[1], at(e, slot) + FP_NL); }
  void st_canon(int e, int slot, const hfp2& v) const {
    fp t;
    fp_canon(t, v.c[0]);
    fp_store(at(e, slot), t);
    fp_canon(t, v.c[1]);
    fp_store(at(e, slot) + FP_NL, t);
  }
};
// the key-set build path: the stored record (RAW_AFFINE G2, 48 words) -> rows; returns 0 or KEYSET_NOLINES_*
static int build_rows(uint32_t* table, const uint32_t* rec) {
  std::vector<uint32_t> scratch(SHARED_TABLE_WORDS);
  const host_io io = {table, scratch.data()};
  return keyset_lines_entry(rec, io);
}
// rows that differ, as field elements, between a built table and a constant one, plus the words that are not canonical (limbs
// below 2^28, the value below p: the line kernel loads them as they are)
static int rows_differ(const uint32_t* table, const uint32_t (*rows)[4 * FP_NL]) {
  int bad = 0;
  for (int e = 0; e < MILLER_ENTRIES; e++) {
    bool same = true;
    for (int k = 0; k < 4; k++) {
      fp a, b, t;
      const uint32_t* w = table + (size_t)e * SHARED_ROW_WORDS + k * FP_NL;
      fp_load(a, w);
      fp_load(b, rows[e] + k * FP_NL);
      same = same && fp_eq(a, b);
      fp_canon(t, a);
      for (int j = 0; j < FP_NL; j++) bad += w[j] >> 28 != 0 || (uint32_t)t.l[j] != w[j];
    }
    bad += !same;
  }
  return bad;
}

// lines_merge_yy against lines_merge with ya, yb embedded in Fp2; in: ten Fp in RAW words (a0, a2, b0, b2 as Fp2, then ya, yb).
// Returns the coefficients that differ, over both tower instantiations.
template <class F2>
static int merge_differs(const fp2& a0, const fp2& a2, const fp2& b0, const fp2& b2, const fp& ya, const fp& yb);
static bool coeff_eq(const fp2& a, const fp2& b) { return fp2_eq(a, b); }
static bool coeff_eq(const hfp2& a, const hfp2& b) { return fp2_eq(a, b); }
static void conv(fp2& r, const fp2& a) { r = a; }
static void conv(hfp2& r, const fp2& a) { to_split(r, a); }
template <class F2>
static int merge_differs(const fp2& a0_, const fp2& a2_, const fp2& b0_, const fp2& b2_, const fp& ya, const fp& yb) {
  F2 a0, a2, b0, b2, a3, b3;
  conv(a0, a0_);
  conv(a2, a2_);
  conv(b0, b0_);
  conv(b2, b2_);
  fp2_from_fp(a3, ya);
  fp2_from_fp(b3, yb);
  line5_t<F2> L, M;
  lines_merge_yy(L, a0, a2, ya, b0, b2, yb);
  lines_merge(M, a0, a2, a3, b0, b2, b3);
  return !coeff_eq(L.c0, M.c0) + !coeff_eq(L.c2, M.c2) + !coeff_eq(L.c4, M.c4) + !coeff_eq(L.c3, M.c3) + !coeff_eq(L.c5, M.c5);
}

// the two verdicts of one Bls12381G1Impl item: pk the key (Jacobian, and `rec` its stored RAW_AFFINE record), sig the signature, h the
// UNCLEARED message point.  out[0]: the loop fed from the key's BUILT rows and G2NEGC_LINES_N on prepare_shared_item's record;
// out[1]: the general two-pair loop on the same four points; -1 in out[0]: the rows were refused
static void verdicts(int* out, const g2_jac& pk, const uint32_t* rec, const g1_jac& sig, const g1_aff& h) {
  g1_aff P[2];
  g2_aff Q[2];
  out[0] = out[1] = prepare_shared_item(P, Q, pk, sig, h);
  if (out[0] != BLS_OK) return;
  std::vector<uint32_t> table(SHARED_TABLE_WORDS);
  if (build_rows(table.data(), rec) != 0) {
    out[0] = -1;
  } else {
    fp12_t<hfp2> fs;
    miller_loop_tables_merged<hfp2>(fs, P[0], table.data(), P[1], G2NEGC_LINES_N);
    out[0] = pairing_verdict(fs);
  }
  P[0].inf = P[1].inf = Q[0].inf = Q[1].inf = false;
  aff<hfp2> QQ[2];
  to_split(QQ[0], Q[0]);
  to_split(QQ[1], Q[1]);
  fp12_t<hfp2> f;
  miller_loop2_merged(f, P, QQ);
  out[1] = pairing_verdict(f);
}

extern "C" {
// in: 10 x 12 RAW words -- a0.c0, a0.c1, a2.c0, a2.c1, b0.c0, b0.c1, b2.c0, b2.c1, ya, yb
int hs_merge_yy_differs(const uint32_t* in) {
  fp v[10];
  for (int k = 0; k < 10; k++) fp_from_raw(v[k], in + 12 * k);
  const fp2 a0 = {v[0], v[1]}, a2 = {v[2], v[3]}, b0 = {v[4], v[5]}, b2 = {v[6], v[7]};
  return merge_differs<fp2>(a0, a2, b0, b2, v[8], v[9]) + merge_differs<hfp2>(a0, a2, b0, b2, v[8], v[9]);
}
// rec: a stored record (RAW_AFFINE G2, 48 words; all-zero: the identity or an invalid entry); table: SHARED_TABLE_WORDS words out;
// returns 0 (usable rows) or KEYSET_NOLINES_*
int hs_build_rows(const uint32_t* rec, uint32_t* table) { return build_rows(table, rec); }
// rec: the record of -[c] g2; the rows that differ from G2NEGC_LINES_N + the words that are not canonical, or -1 when refused
int hs_rows_of_negc(const uint32_t* rec) {
  std::vector<uint32_t> table(SHARED_TABLE_WORDS);
  if (build_rows(table.data(), rec) != 0) return -1;
  return rows_differ(table.data(), G2NEGC_LINES_N);
}
// pk: RAW_PROJ G2 and rec: the same key's RAW_AFFINE record; sig: RAW_PROJ G1; h_aff: the uncleared message point, RAW_AFFINE G1
void hs_verdicts(const uint32_t* pk, const uint32_t* rec, const uint32_t* sig, const uint32_t* h_aff, int* out) {
  g2_jac k;
  g1_jac s;
  g1_aff h;
  load_g2_jac(k, pk);
  load_g1_jac(s, sig);
  fp_from_raw(h.x, h_aff);
  fp_from_raw(h.y, h_aff + 12);
  h.inf = false;
  verdicts(out, k, rec, s, h);
}
int hs_lines_fit(uint64_t n_keys, uint64_t other_bytes, uint64_t cap_mib) { return keyset_lines_fit(n_keys, other_bytes, cap_mib) ? 1 : 0; }
}

#ifdef KEYSET_LINES_HOSTSIM_MAIN
static void aff_record(uint32_t* rec, const g2_aff& q) {
  fp_to_raw(rec, q.x.c0);
  fp_to_raw(rec + 12, q.x.c1);
  fp_to_raw(rec + 24, q.y.c0);
  fp_to_raw(rec + 36, q.y.c1);
}
int main() {
  long bad = 0, seen = 0;
  uint32_t p_minus_1[12], one_raw[12], zero_raw[12] = {0};
  {
    fp one, m;
    fp_one(one);
    fp_to_raw(one_raw, one);
    fp_neg(m, one);
    fp_reduce(m, m);
    fp_to_raw(p_minus_1, m);
  }
  // lines_merge_yy against lines_merge: pseudo-random slots, and every slot in turn at 0, 1 and p - 1
  {
    uint64_t x = 0x9e3779b97f4a7c15ull;
    uint32_t in[120];
    auto fill = [&]() {                     // a word string below p is a field element in Montgomery form
      for (int j = 0; j < 120; j++) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        in[j] = j % 12 == 11 ? (uint32_t)x & 0x0fffffffu : (uint32_t)x;
      }
    };
    for (int t = 0; t < 20; t++) {
      fill();
      bad += hs_merge_yy_differs(in);
      seen++;
    }
    const uint32_t* edges[3] = {zero_raw, one_raw, p_minus_1};
    for (int slot = 0; slot <= 10; slot++)      // slot 10: every slot at once
      for (int ed = 0; ed < 3; ed++) {
        fill();
        for (int k = 0; k < 10; k++)
          if (slot == 10 || k == slot) memcpy(in + 12 * k, edges[ed], 48);
        bad += hs_merge_yy_differs(in);
        seen++;
      }
  }
  // the rows of -[c] g2 through the key-set build path are the generated table; the identity record and a point with y = 0 (its
  // first tangent is vertical: h = 2 Y Z = 0) are flagged as what they are
  std::vector<uint32_t> table(SHARED_TABLE_WORDS);
  {
    g2_aff q;
    g2_negc_gen(q);
    uint32_t rec[48];
    aff_record(rec, q);
    bad += hs_rows_of_negc(rec) != 0;
    uint32_t zero[48] = {0};
    bad += build_rows(table.data(), zero) != KEYSET_NOLINES_EMPTY;
    memset(rec + 24, 0, 96);
    bad += build_rows(table.data(), rec) != KEYSET_NOLINES_FINITE;
    seen += 3;
  }
  // an item signed with k under the message point H' = g1 (any point of E1 serves): pk = k g2, sig = k (1 - x) H' verifies in both
  // forms against (sig, -[c] g2), sig + H' in neither; identities are decided before any pairing
  {
    g1_aff g1;
    fp_load(g1.x, G1_GEN_X);
    fp_load(g1.y, G1_GEN_Y);
    g1.inf = false;
    g2_aff g2;
    fp2_load(g2.x, G2_GEN_X);
    fp2_load(g2.y, G2_GEN_Y);
    g2.inf = false;
    g1_jac gj, sig, t;
    g2_jac qj, pk;
    jac_from_aff(gj, g1);
    jac_from_aff(qj, g2);
    const uint32_t k[8] = {0x12345679u, 0x9abcdef0u, 0x0fedcba9u, 0x7, 0, 0, 0, 0};
    const uint32_t heff[8] = {0x00010001u, 0xd2010000u, 0, 0, 0, 0, 0, 0};      // 1 - x
    jac_mul_scalar(pk, qj, k);
    jac_mul_scalar(t, gj, k);
    jac_mul_scalar(sig, t, heff);
    g2_aff pka;
    jac_to_aff(pka, pk);
    uint32_t rec[48];
    aff_record(rec, pka);
    int v[2];
    verdicts(v, pk, rec, sig, g1);
    bad += v[0] != BLS_OK || v[1] != BLS_OK;
    g1_jac sig2;
    jac_add(sig2, sig, gj);
    verdicts(v, pk, rec, sig2, g1);
    bad += v[0] != BLS_ERR_INVALID_SIGNATURE || v[1] != BLS_ERR_INVALID_SIGNATURE;
    g1_jac inf1;
    jac_set_inf(inf1);
    verdicts(v, pk, rec, inf1, g1);
    bad += v[0] != BLS_ERR_SIG_IDENTITY;
    g2_jac inf2;
    jac_set_inf(inf2);
    verdicts(v, inf2, rec, sig, g1);
    bad += v[0] != BLS_ERR_PK_IDENTITY;
    seen += 4;
  }
  // the size rule: the 32-bit offset of the line kernel, and the cap shared with the fixed-base tables
  bad += !keyset_lines_fit(281970, 0, 4096) + keyset_lines_fit(281971, 0, 1ull << 20) + keyset_lines_fit(0, 0, 4096) + keyset_lines_fit(320, 0, 1) +
         !keyset_lines_fit(320, 0, 5) + keyset_lines_fit(320, 1u << 20, 5);
  seen += 6;
  printf("keyset_lines_hostsim: %ld checks, %ld bad\n", seen, bad);
  return bad ? 1 : 0;
}
#endif
