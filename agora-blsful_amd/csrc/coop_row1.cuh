// Wave-cooperative Miller loop of ONE TABLED pair and nothing walked (k_pairing_value_rows; sigset.cuh): Bls12381G2Impl over a
// registered signature.  The pair is (u, sig) with sig's 68 normalised rows (verify_shared.cuh group_lines_build, the *_LINES_N layout)
// read from the signature set.  The line of entry e is n0_e + (c_e xP) w^2 + yP w^3: it depends on neither f nor a walk, so no lane
// pair owns a point, there are no job slots, and between two product rounds nothing runs but the reduction of f.
// The two line sets of coop_shared take the entries in turn, entry e in set e & 1, so that entry e + 1's line is built while entry e's
// is multiplied:
//   doubling   round 1  lane pairs 0..20 the squaring of f
//              round 2  0..17 f * line (e & 1); the scaler forms c_{e+1} xP into set (e + 1) & 1; after the products the loader reads
//                       row e + 2 and, after the reduction, stages its n0 into set e & 1 and its c beside (xP, 0)
//   addition   round 2 alone
// Two product rounds per doubling entry, one per addition entry (entry 0, where f = 1, has no squaring): 63 + 68 - 1 = 130 rounds
// against the 63 * 3 + 5 = 194 of coop_miller1 (timecrypt.cuh), none of which waits for an owner.  An addition entry's c xP is
// ready before its single round because EVERY line round scales the next entry's, one entry ahead; the row loads -- the only memory
// reads of the loop -- are issued two entries ahead, after a round's products, and staged after the reduction that follows.  No lane
// pair multiplies a slot that nobody staged.
// Slots, all inside coop_shared as coop.cuh declares it:
//   S.line[s][0..2]   n0, c xP, (yP, 0) of the entry whose turn set s has      S.job[0][0][0..1]   c of the staged row, (xP, 0)
// Device code; tests/hostsim_sigset compiles the same functions on the host (one thread per lane pair) under the bound tracker.
#pragma once
#include "coop.cuh"

#define COOP_ROW1_SCALER 30               // the lane pair that scales c xP
#define COOP_ROW1_LOADER 31               // the lane pair that reads the rows
// f <- f^2: the 21 products and their reduction (coop_sqr's, on S.f in place)
__device__ __noinline__ void coop_row1_sqr_round(coop_shared& S) {
  __syncthreads();                 // the loader's stores of the round before are in place
  const int q = coop_pair();
  if (q < 21) {
    int i, j, w;
    coop_sqr_idx(q, i, j, w);
    hfp2 x, y, p;
    coop_ld(x, S.f.c[i]);
    coop_ld(y, S.f.c[j]);
    fp2_mul(p, x, y);
    coop_st(S.prod[q], p);
  }
  __syncthreads();
  coop_reduce<1>(S, S.f);
}
// f *= line `set`.  scale: the scaler turns the staged c into the w^2 coefficient of the OTHER set (the next entry's line); next: the
// row the loader reads for the entry after that (or null), whose n0 goes into `set` once its products are done.
__device__ __noinline__ void coop_row1_line_round(coop_shared& S, int set, bool scale, const uint32_t* next) {
  __syncthreads();                 // line `set` and the staged c are in place
  const int q = coop_pair();
  const uint32_t *pa = nullptr, *pb = nullptr;
  uint32_t* pd = nullptr;
  if (q < 18) {
    pa = S.f.c[q / 3];
    pb = S.line[set][q % 3];
    pd = S.prod[q];
  } else if (q == COOP_ROW1_SCALER && scale) {
    pa = S.job[0][0][0];
    pb = S.job[0][0][1];
    pd = S.line[set ^ 1][1];
  }
  if (pd) {
    hfp2 x, y, p;
    coop_ld(x, pa);
    coop_ld(y, pb);
    fp2_mul(p, x, y);
    coop_st(pd, p);
  }
  __syncthreads();
  hfp2 n0, c;
  const bool stage = q == COOP_ROW1_LOADER && next;
  if (stage) {                     // issued here, consumed after the reduction
    fp2_load(n0, next);
    fp2_load(c, next + 2 * FP_NL);
  }
  coop_reduce<2>(S, S.f);
  if (stage) {                     // nobody reads line `set` or the staged c between this round's products and the next round's barrier
    coop_st(S.line[set][0], n0);
    coop_st(S.job[0][0][0], c);
  }
}

// f ends as conj(f_{|x|,Q}(P)) up to a factor in Fp2 (the rows are normalised), which the easy part of the final exponentiation
// removes; Q is the point whose rows are `rows`: 68 rows of 4 FP_NL words.
__device__ __noinline__ void coop_miller1_rows(coop_shared& S, const g1_aff& P, const uint32_t* rows) {
  const int me = coop_pair();
  {  // f = 1, the constant parts of both line sets, rows 0 and 1
    hfp2 x;
    if (me < 6) {
      if (me == 0) fp2_one(x);
      else fp2_zero(x);
      coop_st(S.f.c[me], x);
    } else if (me == 6 || me == 7) {
      fp2_from_fp(x, P.y);
      coop_st(S.line[me - 6][2], x);
    } else if (me == 8) {
      fp2_from_fp(x, P.x);
      coop_st(S.job[0][0][1], x);
    } else if (me == COOP_ROW1_SCALER) {             // row 0: its line whole, c_0 xP by this lane pair's own product
      hfp2 c, xp, p;
#if !defined(COOP_ROW1_TEST_SKIP_ROW0)               // test only (tests/hostsim_sigset): the strict harness must notice the missing slot
      fp2_load(x, rows);
      coop_st(S.line[0][0], x);
#endif
      fp2_load(c, rows + 2 * FP_NL);
      fp2_from_fp(xp, P.x);
      fp2_mul(p, c, xp);
      coop_st(S.line[0][1], p);
    } else if (me == COOP_ROW1_LOADER) {             // row 1: n0 in place, c staged for the scaler of entry 0's line round
      hfp2 c;
      fp2_load(x, rows + 4 * FP_NL);
      fp2_load(c, rows + 4 * FP_NL + 2 * FP_NL);
      coop_st(S.line[1][0], x);
      coop_st(S.job[0][0][0], c);
    }
  }
  int row = 0;
  for (int i = 62; i >= 0; i--) {
    if (i != 62) coop_row1_sqr_round(S);
    coop_row1_line_round(S, row & 1, row + 1 < MILLER_ENTRIES, row + 2 < MILLER_ENTRIES ? rows + (row + 2) * (4 * FP_NL) : nullptr);
    row++;
    if ((BLS_X_ABS >> i) & 1) {      // addition entry (set bits of |x|)
      coop_row1_line_round(S, row & 1, row + 1 < MILLER_ENTRIES, row + 2 < MILLER_ENTRIES ? rows + (row + 2) * (4 * FP_NL) : nullptr);
      row++;
    }
  }
  coop_conj(S.f, S.f);
}
