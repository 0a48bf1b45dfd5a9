// TEST-ONLY harness for tests/test_hostsim_verify_shared.py: compiles the per-item functions of the shared-message verify calls
// (agora-blsful_amd/csrc/verify_shared.cuh: shared_group_of, shared_expand_src, prepare_shared_item, group_lines_build) as plain
// host C++ with the bound tracker on, the line-table routine on the host emulation of the lane-split tower (tower_split.cuh), and
// runs the host Miller loop over the built table (miller_loop_fixed_g2_merged, what k_lines2s_shared + k_millerf2s compute) beside
// the general two-pair loop.  Built twice: as a shared object driven from Python, and -- with VERIFY_SHARED_HOSTSIM_MAIN -- as a
// stand-alone program under the address and undefined-behaviour sanitizers that walks the same functions over its own inputs.
// Never linked into libblsgpu.so.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../agora-blsful_amd/csrc/verify_shared.cuh"

static void raw_fp2(fp2& r, const uint32_t* w) { fp_from_raw(r.c0, w); fp_from_raw(r.c1, w + 12); }
static void load_g1_jac(g1_jac& p, const uint32_t* w) { fp_from_raw(p.x, w); fp_from_raw(p.y, w + 12); fp_from_raw(p.z, w + 24); }
static void load_g2_jac(g2_jac& p, const uint32_t* w) { raw_fp2(p.x, w); raw_fp2(p.y, w + 24); raw_fp2(p.z, w + 48); }
static void to_split(hfp2& r, const fp2& a) { r.c[0] = a.c0; r.c[1] = a.c1; }
static void to_split(aff<hfp2>& r, const g2_aff& q) { to_split(r.x, q.x); to_split(r.y, q.y); r.inf = false; }

// a group's table and scratch rows on the host: both lanes' components side by side, as the device's two lanes leave them
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
static bool build_table(uint32_t* table, const g2_aff& q) {
  std::vector<uint32_t> scratch(SHARED_TABLE_WORDS);
  aff<hfp2> qs;
  to_split(qs, q);
  const host_io io = {table, scratch.data()};
  return group_lines_build(qs.x, qs.y, q.inf, io);
}
// rows that differ, as field elements, between a built table and a constant one
static int rows_differ(const uint32_t* table, const uint32_t (*rows)[4 * FP_NL]) {
  int bad = 0;
  for (int e = 0; e < MILLER_ENTRIES; e++) {
    bool same = true;
    for (int k = 0; k < 4; k++) {
      fp a, b;
      fp_load(a, table + (size_t)e * SHARED_ROW_WORDS + k * FP_NL);
      fp_load(b, rows[e] + k * FP_NL);
      same = same && fp_eq(a, b);
    }
    bad += !same;
  }
  return bad;
}
// the stored words are canonical: limbs below 2^28 and the value below p (the consumer loads them as they are)
static int rows_not_canonical(const uint32_t* table) {
  int bad = 0;
  for (size_t w = 0; w < (size_t)SHARED_TABLE_WORDS; w += FP_NL) {
    fp a, t;
    fp_load(a, table + w);
    fp_canon(t, a);
    for (int k = 0; k < FP_NL; k++) bad += table[w + k] >> 28 != 0 || (uint32_t)t.l[k] != table[w + k];
  }
  return bad;
}
// the two verdicts of one Bls12381G2Impl item whose group point is h: the Miller loop fed from the group's BUILT table on the
// swapped record (what the table form computes) and the general two-pair loop on the plain record; -1: the table was refused
static void verdicts(int* out, const g1_jac& pk, const g2_jac& sig, const g2_aff& h) {
  g1_aff P[2];
  g2_aff Q[2];
  out[0] = out[1] = prepare_shared_item(P, Q, pk, sig, h, true);
  if (out[0] != BLS_OK) return;
  std::vector<uint32_t> table(SHARED_TABLE_WORDS);
  if (!build_table(table.data(), h)) {
    out[0] = -1;
  } else {
    aff<hfp2> q0;
    to_split(q0, Q[0]);                    // the signature: the walked point
    fp12_t<hfp2> fs;
    miller_loop_fixed_g2_merged(fs, P[0], q0, P[1], (const uint32_t (*)[4 * FP_NL])table.data());
    out[0] = pairing_verdict(fs);
  }
  prepare_shared_item(P, Q, pk, sig, h, false);
  P[0].inf = P[1].inf = Q[0].inf = Q[1].inf = false;
  aff<hfp2> QQ[2];
  to_split(QQ[0], Q[0]);
  to_split(QQ[1], Q[1]);
  fp12_t<hfp2> f;
  miller_loop2_merged(f, P, QQ);
  out[1] = pairing_verdict(f);
}

extern "C" {
uint64_t hs_group_of(const uint64_t* offs, uint64_t n_groups, uint64_t i) { return shared_group_of(offs, (size_t)n_groups, i); }
uint64_t hs_expand_src(const uint64_t* x_offs, uint64_t n_items, const uint64_t* item_offs, uint64_t n_groups, const uint64_t* msg_offs, uint64_t b) {
  return shared_expand_src(x_offs, (size_t)n_items, item_offs, (size_t)n_groups, msg_offs, b);
}
// which: 1 = -g2 against G2NEG_LINES_N, 2 = -[c] g2 against G2NEGC_LINES_N; returns the rows that differ + the words that are not
// canonical, or -1 when the routine refused the point
int hs_table_of_constant(int which) {
  g2_aff q;
  if (which == 1) g2_neg_gen(q);
  else g2_negc_gen(q);
  std::vector<uint32_t> table(SHARED_TABLE_WORDS);
  if (!build_table(table.data(), q)) return -1;
  return rows_differ(table.data(), which == 1 ? G2NEG_LINES_N : G2NEGC_LINES_N) + rows_not_canonical(table.data());
}
// q: a RAW_AFFINE G2 record (48 words; all-zero: the identity); table: SHARED_TABLE_WORDS words out; returns 1 when the rows are usable
int hs_build_table(const uint32_t* q, uint32_t* table) {
  g2_aff a;
  a.inf = true;
  for (int k = 0; k < 48; k++) a.inf = a.inf && q[k] == 0;
  raw_fp2(a.x, q);
  raw_fp2(a.y, q + 24);
  return build_table(table, a) ? 1 : 0;
}
// pk: RAW_PROJ G1, sig: RAW_PROJ G2, h: RAW_AFFINE G2 (the group's point); out[0] = the table form's verdict, out[1] = the general one
void hs_verdicts(const uint32_t* pk, const uint32_t* sig, const uint32_t* h, int* out) {
  g1_jac k;
  g2_jac s;
  g2_aff a;
  load_g1_jac(k, pk);
  load_g2_jac(s, sig);
  raw_fp2(a.x, h);
  raw_fp2(a.y, h + 24);
  a.inf = false;
  verdicts(out, k, s, a);
}
// Bls12381G1Impl: the record of prepare_shared_item against prepare_hashed_item's on the same points (h: RAW_PROJ G1 with Z = 1 is
// the affine point); returns the status, or -10 when a coordinate differs
int hs_prepare_g1impl(const uint32_t* pk, const uint32_t* sig, const uint32_t* h_aff) {
  g2_jac k;
  g1_jac s, hj;
  load_g2_jac(k, pk);
  load_g1_jac(s, sig);
  fp_from_raw(hj.x, h_aff);
  fp_from_raw(hj.y, h_aff + 12);
  fp_one(hj.z);
  g1_aff h = {hj.x, hj.y, false}, P[2], P2[2];
  g2_aff Q[2], Q2[2];
  const int st = prepare_shared_item(P, Q, k, s, h), st2 = prepare_hashed_item(P2, Q2, k, s, hj);
  if (st != st2) return -11;
  if (st != BLS_OK) return st;
  g2_aff nc;
  g2_negc_gen(nc);
  const bool same = fp_eq(P[0].x, P2[0].x) && fp_eq(P[0].y, P2[0].y) && fp_eq(P[1].x, P2[1].x) && fp_eq(P[1].y, P2[1].y) && fp2_eq(Q[0].x, Q2[0].x) &&
                    fp2_eq(Q[0].y, Q2[0].y) && fp2_eq(Q[1].x, nc.x) && fp2_eq(Q[1].y, nc.y);
  return same ? st : -10;
}
}

#ifdef VERIFY_SHARED_HOSTSIM_MAIN
static size_t linear_group_of(const std::vector<uint64_t>& offs, uint64_t i) {
  size_t g = 0;
  for (size_t s = 0; s + 1 < offs.size(); s++)
    if (offs[s] <= i) g = s;
  return g;
}
int main() {
  long bad = 0, seen = 0;
  // the group lookup against a linear scan: runs of empty groups first, in the middle and last, groups of one, one group alone
  uint64_t x = 0x9e3779b97f4a7c15ull;
  for (int t = 0; t < 300; t++) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    const size_t ng = 1 + (size_t)(x % 40);
    std::vector<uint64_t> offs(ng + 1, 0);
    uint64_t y = x;
    for (size_t g = 0; g < ng; g++) {
      y ^= y << 13, y ^= y >> 7, y ^= y << 17;
      const uint64_t size = (y & 3) < 2 ? 0 : (y >> 8) % 5;          // half the groups are empty
      offs[g + 1] = offs[g] + size;
    }
    for (uint64_t i = 0; i < offs[ng]; i++) {
      const size_t g = shared_group_of(offs.data(), ng, i);
      bad += g != linear_group_of(offs, i) || !(offs[g] <= i && i < offs[g + 1]);
      seen++;
    }
  }
  // the byte gather of the MessageAugmentation path: every byte of the per-item buffer comes from its item's group's message
  {
    const uint64_t ioffs[6] = {0, 0, 2, 2, 5, 5}, moffs[6] = {0, 3, 7, 9, 9, 12};       // groups 1 (4-byte message) and 3 (empty message) own items
    uint64_t xoffs[6] = {0, 4, 8, 8, 8, 8};
    for (uint64_t b = 0; b < 8; b++) bad += shared_expand_src(xoffs, 5, ioffs, 5, moffs, b) != 3 + (b & 3);
    seen += 8;
  }
  // the line tables of the two constant points reproduce the generated ones row for row
  std::vector<uint32_t> table(SHARED_TABLE_WORDS), scratch(SHARED_TABLE_WORDS);
  for (int which = 1; which <= 2; which++) {
    const int r = hs_table_of_constant(which);
    bad += r != 0;
    seen++;
  }
  // the flag: the identity, and a point with y = 0 (its first tangent is vertical: h = 2 Y Z = 0)
  {
    g2_aff q;
    g2_neg_gen(q);
    q.inf = true;
    bad += build_table(table.data(), q);
    q.inf = false;
    fp2_zero(q.y);
    bad += build_table(table.data(), q);
    uint32_t zero[48] = {0};
    bad += hs_build_table(zero, table.data()) != 0;
    seen += 3;
  }
  // an item signed with k under the group point H = -[c] g2 (any G2 point serves): pk = k g1, sig = k H verifies in both forms,
  // sig = (k + 1) H in neither; identities are decided before any pairing
  {
    g2_aff h;
    g2_negc_gen(h);
    g1_aff g1;
    fp_load(g1.x, G1_GEN_X);
    fp_load(g1.y, G1_GEN_Y);
    g1.inf = false;
    g1_jac gj, pk;
    g2_jac hj, sig;
    jac_from_aff(gj, g1);
    jac_from_aff(hj, h);
    uint32_t k[8] = {0x12345679u, 0x9abcdef0u, 0x0fedcba9u, 0x7, 0, 0, 0, 0};
    jac_mul_scalar(pk, gj, k);
    jac_mul_scalar(sig, hj, k);
    int v[2];
    verdicts(v, pk, sig, h);
    bad += v[0] != BLS_OK || v[1] != BLS_OK;
    k[0]++;
    jac_mul_scalar(sig, hj, k);
    verdicts(v, pk, sig, h);
    bad += v[0] != BLS_ERR_INVALID_SIGNATURE || v[1] != BLS_ERR_INVALID_SIGNATURE;
    g2_jac inf2;
    jac_set_inf(inf2);
    verdicts(v, pk, inf2, h);
    bad += v[0] != BLS_ERR_SIG_IDENTITY;
    g1_jac inf1;
    jac_set_inf(inf1);
    verdicts(v, inf1, inf2, h);
    bad += v[0] != BLS_ERR_SIG_IDENTITY;
    verdicts(v, inf1, sig, h);
    bad += v[0] != BLS_ERR_PK_IDENTITY;
    seen += 5;
  }
  printf("verify_shared_hostsim: %ld checks, %ld bad\n", seen, bad);
  return bad ? 1 : 0;
}
#endif
