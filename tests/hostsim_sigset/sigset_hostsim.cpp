// TEST-ONLY harness for tests/test_hostsim_sigset.py: the body of k_pairing_value_rows -- coop_miller1_rows
// (agora-blsful_amd/csrc/coop_row1.cuh), coop_final_value (coop.cuh) and coop_gt_bytes (timecrypt.cuh) -- as plain host C++ with the
// bound tracker on and STRICT: a read of an LDS slot nobody wrote aborts, so the loop multiplies nothing it has not staged.  The wave,
// its barrier, the LDS block, the tracker records and the rows' host io (rows_host_io; the rows are built by group_lines_build through
// keyset_lines_entry, the path that builds a signature set's rows) are those of tests/hostsim_coop and tests/hostsim_coop_rows, whose
// sources this file includes as they stand.  Built with -DCOOP_ROW1_TEST_SKIP_ROW0 the loop leaves the first row's n0 unstaged: the
// test uses that build to see the harness abort.  Never linked into libblsgpu.so.
#include "../hostsim_coop_rows/coop_rows_hostsim.cpp"

#define __device__ static
#define __forceinline__ inline
#define __noinline__ __attribute__((noinline))
#include "../../agora-blsful_amd/csrc/timecrypt.cuh"
#include "../../agora-blsful_amd/csrc/coop_row1.cuh"
#undef __device__
#undef __forceinline__
#undef __noinline__

extern "C" {
// in: the limb vectors P.x, P.y, declared reduced as hs_coop_pairing declares them; rec: Q as a stored RAW_AFFINE record (48 words);
// out = the 576 Gt bytes.  Returns 0; -2: the rows were refused.  A tracked-bound violation or an unstaged slot aborts.
int hs_pairing_value_rows(const int32_t* in, const uint32_t* rec, uint8_t* out) {
  std::vector<uint32_t> table(SHARED_TABLE_WORDS), scratch(SHARED_TABLE_WORDS);
  const rows_host_io io = {table.data(), scratch.data()};
  if (keyset_lines_entry(rec, io) != 0) return -2;
  hs_reset_lds(0x7fffffffu);
  g_strict = true;
  g1_aff P;
  hs_in_fp(P.x, in, 0);
  hs_in_fp(P.y, in, 1);
  P.inf = false;
  hs_run_wave([&](int p) {
    threadIdx.x = 2 * p;
    coop_shared& S = *(coop_shared*)g_lds;
    coop_miller1_rows(S, P, table.data());
    coop_final_value(S);
    coop_gt_bytes(out, S.t);
  });
  return 0;
}
// the body of k_pairing_value on the same pair, Q walked: six limb vectors (P.x, P.y, Q.x.c0, Q.x.c1, Q.y.c0, Q.y.c1)
int hs_pairing_value_walked(const int32_t* in, uint8_t* out) {
  hs_reset_lds(0x7fffffffu);
  g_strict = false;              // coop_miller1's product rounds multiply the second pair's job slots, which nobody stages
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
}
