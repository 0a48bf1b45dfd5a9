// TEST-ONLY harness for tests/test_hostsim_agg_keyed.py: compiles the host side of the keyed line kernel of the batched aggregate
// verify over a registered key set (agora-blsful_amd/csrc/pairing.cuh miller_line3_row -- the per-entry value k_linesp_keyed stores --
// keyset.cuh keyset_lines_entry, agg_batch.cuh agg_batch_plan / agg_flat_pair / agg_flat_key) as plain host C++ with the bound
// tracker on, on the host emulation of the lane-split tower.  Every item is ONE pair whose G2 member is given as 68 normalised
// rows: its value goes through the one-pair Miller accumulation (acc_sqr, acc_mul_line, acc_finish: what k_millerfp3 does with
// the stored lines), the items' values are multiplied and the product takes the final exponentiation.  Built twice: as a shared
// object driven from Python, and -- with AGG_KEYED_HOSTSIM_MAIN -- as a stand-alone program under the address and
// undefined-behaviour sanitizers that walks the same functions over its own inputs.  Never linked into libblsgpu.so.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../agora-blsful_amd/csrc/keyset.cuh"
#include "../../agora-blsful_amd/csrc/agg_batch.cuh"

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
static int build_rows(uint32_t* table, const uint32_t* rec) {
  std::vector<uint32_t> scratch(SHARED_TABLE_WORDS);
  const host_io io = {table, scratch.data()};
  return keyset_lines_entry(rec, io);
}
// the Miller value of ONE item from its rows (68 x 4 FP_NL words) at the G1 point (x, y): per entry the keyed kernel's value, then
// k_millerfp3's accumulation
static void item_value(fp12_t<hfp2>& f, const uint32_t* rows, const fp& x, const fp& y) {
  acc_one(f);
  for (int e = 0; e < MILLER_ENTRIES; e++) {
    const uint32_t* r = rows + (size_t)e * (4 * FP_NL);
    hfp2 n0, c, l0, l2, l3;
    fp2_load(n0, r);
    fp2_load(c, r + 2 * FP_NL);
    miller_line3_row(l0, l2, l3, n0, c, x, y);
    if (e != 0 && !miller_entry_is_add(e)) acc_sqr(f);
    acc_mul_line(f, l0, l2, l3);
  }
  acc_finish(f);
}

extern "C" {
// The verdict of a product of n pair items times the signature item, every line value from rows.  recs: n stored key records
// (RAW_AFFINE G2, 48 words each); pts: n uncleared message points and then the signature (RAW_AFFINE G1, 24 words each); negc_rec:
// the record of -[c] g2, whose rows are BUILT here when it is given, else (null) the generated table G2NEGC_LINES_N is read.
// Returns BLS_OK / BLS_ERR_INVALID_SIGNATURE, or -1 when some rows were refused.
int hs_product_verdict(const uint32_t* recs, const uint32_t* pts, size_t n, const uint32_t* negc_rec) {
  std::vector<uint32_t> table(SHARED_TABLE_WORDS);
  fp12_t<hfp2> prod, f;
  fp12_one(prod);
  for (size_t i = 0; i <= n; i++) {
    fp x, y;
    fp_from_raw(x, pts + 24 * i);
    fp_from_raw(y, pts + 24 * i + 12);
    const uint32_t* rows = table.data();
    if (i < n || negc_rec) {
      if (build_rows(table.data(), i < n ? recs + 48 * i : negc_rec) != 0) return -1;
    } else {
      rows = &G2NEGC_LINES_N[0][0];
    }
    item_value(f, rows, x, y);
    fp12_mul(prod, prod, f);
  }
  return pairing_verdict(prod);
}
// The flat list of a call, integers only.  sizes: n_sets set sizes; a set of max_small pairs or more is large.  cidx: one entry per
// caller position (T = sum of sizes).  The line kernel runs in rounds of per_round items (the library: hs_round_size).  Out, per
// flat item i (M = T_b + n_b of them): key[i] = the entry lane pair (first, j) with first + j = i resolves to (0xfffffffe for a
// signature item), src[i] = its caller position (a signature item: its set), first_of[i] = the `first` of the round that took it.
// Returns M, or -1 when an item was taken by no round or by two.
long hs_flat_map(const uint64_t* sizes, size_t n_sets, uint64_t max_small, size_t per_round, const uint32_t* cidx, uint32_t* key, uint32_t* src_out,
                 uint64_t* first_of) {
  std::vector<uint64_t> offs(n_sets + 1, 0), boffs, bsrc;
  for (size_t s = 0; s < n_sets; s++) offs[s + 1] = offs[s] + sizes[s];
  std::vector<uint32_t> bset;
  std::vector<size_t> large;
  uint64_t tmax_large = 0;
  agg_batch_plan(offs.data(), n_sets, max_small, boffs, bsrc, bset, large, &tmax_large);
  const size_t n_b = bset.size(), T_b = (size_t)boffs.back(), M = n_b ? T_b + n_b : 0;
  // k_prepare_agg_seg's map, k_agg_flat_keys
  std::vector<uint32_t> src(T_b ? T_b : 1), key_of(T_b ? T_b : 1);
  for (size_t i = 0; i < T_b; i++) {
    uint32_t b = 0;
    while (boffs[b + 1] <= i) b++;                       // ragged_set_of: the last set with boffs[b] <= i among the non-empty ones
    src[i] = (uint32_t)agg_flat_pair(boffs.data(), bsrc.data(), b, i);
  }
  for (size_t i = 0; i < T_b; i++) key_of[i] = agg_flat_key(src.data(), cidx, i);
  // the rounds of the line kernel: lane pair j of the round at `first` is flat item first + j
  std::vector<int> taken(M ? M : 1, 0);
  if (M && !per_round) return -1;
  for (size_t first = 0; first < M; first += per_round) {
    const size_t cnt = M - first < per_round ? M - first : per_round;
    for (size_t j = 0; j < cnt; j++) {
      const size_t i = first + j;
      taken[i]++;
      first_of[i] = first;
      if (i >= T_b) {
        key[i] = 0xfffffffeu;
        src_out[i] = bset[i - T_b];
      } else {
        key[i] = key_of[i];
        src_out[i] = src[i];
      }
    }
  }
  for (size_t i = 0; i < M; i++)
    if (taken[i] != 1) return -1;
  return (long)M;
}
size_t hs_round_size(size_t M, size_t round) { return agg_round_size(M, round); }
}

#ifdef AGG_KEYED_HOSTSIM_MAIN
static void aff_record(uint32_t* rec, const g2_aff& q) {
  fp_to_raw(rec, q.x.c0);
  fp_to_raw(rec + 12, q.x.c1);
  fp_to_raw(rec + 24, q.y.c0);
  fp_to_raw(rec + 36, q.y.c1);
}
static void aff_point(uint32_t* w, const g1_jac& p) {
  g1_aff a;
  jac_to_aff(a, p);
  fp_to_raw(w, a.x);
  fp_to_raw(w + 12, a.y);
}
int main() {
  long bad = 0, seen = 0;
  // three signers k_i under the "message points" H'_i = m_i g1 (any points of E1 serve): pk_i = k_i g2, sig = sum k_i (1 - x) H'_i
  // verifies against (sig, -[c] g2) in products of 1, 2 and 3 pairs; with a message point or a key swapped it does not
  g1_aff g1;
  fp_load(g1.x, G1_GEN_X);
  fp_load(g1.y, G1_GEN_Y);
  g1.inf = false;
  g2_aff g2;
  fp2_load(g2.x, G2_GEN_X);
  fp2_load(g2.y, G2_GEN_Y);
  g2.inf = false;
  g1_jac gj;
  g2_jac qj;
  jac_from_aff(gj, g1);
  jac_from_aff(qj, g2);
  const uint32_t ks[3][8] = {{0x12345679u, 0x9abcdef0u, 0x0fedcba9u, 0x7, 0, 0, 0, 0}, {0x0badcafeu, 0x31415926u, 0x5, 0, 0, 0, 0, 0}, {0x27182818u, 0x28459045u, 0x23536028u, 0x1, 0, 0, 0, 0}};
  const uint32_t ms[3][8] = {{3, 0, 0, 0, 0, 0, 0, 0}, {0x10001u, 7, 0, 0, 0, 0, 0, 0}, {0xdeadbeefu, 0, 1, 0, 0, 0, 0, 0}};
  const uint32_t heff[8] = {0x00010001u, 0xd2010000u, 0, 0, 0, 0, 0, 0};      // 1 - x
  uint32_t recs[3 * 48], pts[4 * 24], negc[48];
  g1_jac h[3], part[3];
  for (int i = 0; i < 3; i++) {
    g2_jac pk;
    g2_aff pka;
    jac_mul_scalar(pk, qj, ks[i]);
    jac_to_aff(pka, pk);
    aff_record(recs + 48 * i, pka);
    jac_mul_scalar(h[i], gj, ms[i]);
    g1_jac t;
    jac_mul_scalar(t, h[i], ks[i]);
    jac_mul_scalar(part[i], t, heff);
  }
  {
    g2_aff q;
    g2_negc_gen(q);
    aff_record(negc, q);
  }
  for (int n = 1; n <= 3; n++) {
    g1_jac sig = part[0];
    for (int i = 1; i < n; i++) {
      g1_jac t;
      jac_add(t, sig, part[i]);
      sig = t;
    }
    for (int i = 0; i < n; i++) aff_point(pts + 24 * i, h[i]);
    aff_point(pts + 24 * n, sig);
    bad += hs_product_verdict(recs, pts, n, nullptr) != BLS_OK;
    bad += hs_product_verdict(recs, pts, n, negc) != BLS_OK;                 // the built rows of -[c] g2 serve as the generated ones do
    aff_point(pts + 24 * (n - 1), h[n % 3]);                                 // one message point changed
    bad += hs_product_verdict(recs, pts, n, nullptr) != BLS_ERR_INVALID_SIGNATURE;
    aff_point(pts + 24 * (n - 1), h[n - 1]);
    uint32_t swapped[3 * 48];
    memcpy(swapped, recs, sizeof swapped);
    memcpy(swapped + 48 * (n - 1), recs + 48 * (n % 3), 192);                // one key swapped
    bad += hs_product_verdict(swapped, pts, n, nullptr) != BLS_ERR_INVALID_SIGNATURE;
    seen += 4;
  }
  {
    uint32_t zero[48] = {0};
    memcpy(recs, zero, 192);                                                 // the identity record has no rows: refused, never evaluated
    bad += hs_product_verdict(recs, pts, 1, nullptr) != -1;
    seen++;
  }
  // the flat list of sets 0, 3, 9 (large), 1, 0, 2 in rounds of 4 items: every item once, pair items at their own positions
  {
    const uint64_t sizes[6] = {0, 3, 9, 1, 0, 2};
    uint32_t cidx[15], key[16], src[16];
    uint64_t first_of[16];
    for (int p = 0; p < 15; p++) cidx[p] = 1000 + p;
    const long M = hs_flat_map(sizes, 6, 5, 4, cidx, key, src, first_of);
    bad += M != 6 + 5;
    const uint32_t want_src[11] = {0, 1, 2, 12, 13, 14, 0, 1, 3, 4, 5};
    for (long i = 0; i < 11 && M == 11; i++) bad += src[i] != want_src[i] || key[i] != (i < 6 ? 1000 + want_src[i] : 0xfffffffeu) || first_of[i] != (uint64_t)(i / 4 * 4);
    seen += 2;
  }
  printf("agg_keyed_hostsim: %ld checks, %ld bad\n", seen, bad);
  return bad ? 1 : 0;
}
#endif
