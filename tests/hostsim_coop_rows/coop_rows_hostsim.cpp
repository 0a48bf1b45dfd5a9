// TEST-ONLY harness for tests/test_hostsim_coop_rows.py: the Miller loop of one TABLED and one WALKED pair of the wave-cooperative
// engine (agora-blsful_amd/csrc/coop_rows.cuh coop_miller2_rows, what k_pairing_coop_rows runs) as plain host C++ with the bound
// tracker on and STRICT: a read of an LDS slot nobody wrote aborts, so the loop multiplies nothing it has not staged.  The wave, its
// barrier, the LDS block and the tracker records that carry an element's bounds through its slot are those of tests/hostsim_coop,
// whose source this file includes as it stands; pair 0's rows are built by group_lines_build (through keyset_lines_entry, the path
// that builds a message set's rows).  Never linked into libblsgpu.so.
#include "../hostsim_coop/coop_hostsim.cpp"
#include "../../agora-blsful_amd/csrc/keyset.cuh"

#define __device__ static
#define __forceinline__ inline
#define __noinline__ __attribute__((noinline))
#include "../../agora-blsful_amd/csrc/coop_rows.cuh"
#undef __device__
#undef __forceinline__
#undef __noinline__

// an entry's table and scratch rows on the host, as tests/hostsim_keyset_lines keeps them
struct rows_host_io {
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

extern "C" {
// The body of k_pairing_coop_rows on one item.  in: the twelve limb vectors of hs_coop_pairing (pair 0's Q is not read); rec: pair 0's
// G2 member as a stored RAW_AFFINE record (48 words).  mode 0: out = the easy-part value, twelve limb vectors in tower order,
// returns 0; mode 1: returns the status.  -2: the rows were refused.
int hs_coop_pairing_rows(int mode, const int32_t* in, const uint32_t* rec, int32_t* out) {
  std::vector<uint32_t> table(SHARED_TABLE_WORDS), scratch(SHARED_TABLE_WORDS);
  const rows_host_io io = {table.data(), scratch.data()};
  if (keyset_lines_entry(rec, io) != 0) return -2;
  hs_reset_lds(0x7fffffffu);
  g_strict = true;
  g1_aff P[2];
  aff<hfp2> Q1;
  for (int k = 0; k < 2; k++) {
    hs_in_fp(P[k].x, in, 6 * k);
    hs_in_fp(P[k].y, in, 6 * k + 1);
    P[k].inf = false;
  }
  hs_in_fp(Q1.x.c[0], in, 8);
  hs_in_fp(Q1.x.c[1], in, 9);
  hs_in_fp(Q1.y.c[0], in, 10);
  hs_in_fp(Q1.y.c[1], in, 11);
  Q1.inf = false;
  g_status = -1;
  hs_run_wave([&](int p) {
    threadIdx.x = 2 * p;
    coop_shared& S = *(coop_shared*)g_lds;
    coop_miller2_rows(S, P, Q1, table.data());
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
