// TEST-ONLY harness for tests/test_hostsim_coop_keyed.py: the Miller loop of two TABLED pairs of the wave-cooperative engine
// (agora-blsful_amd/csrc/coop.cuh coop_miller2_tables, what k_pairing_coop_keyed runs) as plain host C++ with the bound tracker on.
// The wave, its barrier, the LDS block and the tracker records that carry an element's bounds through its slot are those of
// tests/hostsim_coop, whose source this file includes as it stands; pair 0's rows are built by the key-set build path
// (keyset.cuh keyset_lines_entry), pair 1's are the generated table G2NEGC_LINES_N.  Reads of a slot nobody wrote abort: the
// tabled loop, unlike coop_miller2, multiplies nothing it has not staged.  Never linked into libblsgpu.so.
#include "../hostsim_coop/coop_hostsim.cpp"
#include "../../agora-blsful_amd/csrc/keyset.cuh"

// an entry's table and scratch rows on the host, as tests/hostsim_keyset_lines keeps them
struct tl_host_io {
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
// Fp2 number k of a limb-vector list with declared bounds
static void tl_ld2(hfp2& h, const int32_t* in, const double* lb, const double* vb, int k) {
  for (int c = 0; c < 2; c++) {
    fp& r = h.c[c];
    const int v = 2 * k + c;
    for (int i = 0; i < FP_NL; i++) r.l[i] = in[v * FP_NL + i];
    r.lb = lb[v];
    r.vb = vb[v];
    r.nn = false;
  }
}
static void tl_ld1(hfp2& h, const int32_t* in, const double* lb, const double* vb, int v) {   // an Fp as (k, 0)
  fp k;
  for (int i = 0; i < FP_NL; i++) k.l[i] = in[v * FP_NL + i];
  k.lb = lb[v];
  k.vb = vb[v];
  k.nn = false;
  fp2_from_fp(h, k);
}

extern "C" {
// The body of k_pairing_coop_keyed on one item.  in: the twelve limb vectors of hs_coop_pairing (the record's Q members are not
// read); rec: pair 0's G2 member as a stored RAW_AFFINE record (48 words).  mode 0: out = the easy-part value, twelve limb vectors
// in tower order, returns 0; mode 1: returns the status.  -2: the rows were refused.
int hs_coop_pairing_keyed(int mode, const int32_t* in, const uint32_t* rec, int32_t* out) {
  std::vector<uint32_t> table(SHARED_TABLE_WORDS), scratch(SHARED_TABLE_WORDS);
  const tl_host_io io = {table.data(), scratch.data()};
  if (keyset_lines_entry(rec, io) != 0) return -2;
  hs_reset_lds(0x7fffffffu);
  g_strict = true;
  g1_aff P[2];
  for (int k = 0; k < 2; k++) {
    hs_in_fp(P[k].x, in, 6 * k);
    hs_in_fp(P[k].y, in, 6 * k + 1);
    P[k].inf = false;
  }
  g_status = -1;
  hs_run_wave([&](int p) {
    threadIdx.x = 2 * p;
    coop_shared& S = *(coop_shared*)g_lds;
    coop_miller2_tables(S, P, table.data(), G2NEGC_LINES_N);
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
// coop_reduce_line5 on its own.  in: the 30 staged products f_i L_j (product 5 i + j, j over w^0, w^2, w^3, w^4, w^5) as 60 limb
// vectors with declared bounds; out: the six coefficients at w^0 .. w^5, twelve limb vectors.
void hs_coop_reduce_line5(const int32_t* in, const double* lb, const double* vb, int32_t* out) {
  hs_reset_lds(0x7fffffffu);
  g_strict = true;
  hs_run_wave([&](int p) {
    threadIdx.x = 2 * p;
    coop_shared& S = *(coop_shared*)g_lds;
    if (p < 30) {
      hfp2 x;
      tl_ld2(x, in, lb, vb, p);
      coop_st(S.prod[p], x);
    }
    __syncthreads();
    coop_reduce_line5(S, S.t);
    if (p < 6) {
      hfp2 x;
      coop_ld(x, S.t.c[p]);
      hs_st2(out, p, x);
    }
  });
}
// The merge round on its own (no squaring rides along), after the round that forms xi ya yb.  in: a0, a2, b0, b2 (Fp2: eight limb
// vectors), then ya, yb (Fp) with declared bounds; the sums a0 + a2, b0 + b2 are staged unnormalised, as the multiply round leaves
// them.  out: c0, c2, c3, c4, c5, ten limb vectors.
void hs_coop_merge_round(const int32_t* in, const double* lb, const double* vb, int32_t* out) {
  hs_reset_lds(0x7fffffffu);
  g_strict = true;
  hs_run_wave([&](int p) {
    threadIdx.x = 2 * p;
    coop_shared& S = *(coop_shared*)g_lds;
    if (p < 2) {
      hfp2 n0, n2, s;
      tl_ld2(n0, in, lb, vb, 2 * p);
      tl_ld2(n2, in, lb, vb, 2 * p + 1);
      fp2_add(s, n0, n2);
      coop_st(S.line[p][0], n0);
      coop_st(S.line[p][1], n2);
      coop_st(S.line[p][2], s);
    } else if (p < 4) {
      hfp2 y;
      tl_ld1(y, in, lb, vb, 8 + (p - 2));
      coop_st(S.v.c[p - 2], y);
    }
    __syncthreads();
    coop_tl_mul_round(S, 0, false);
    coop_tl_merge_round(S, false, nullptr);
    if (p < 5) {
      hfp2 x;
      coop_ld(x, S.u.c[p]);
      hs_st2(out, p, x);
    }
  });
}
}
