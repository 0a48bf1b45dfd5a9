// Wave-cooperative Miller loop of one TABLED and one WALKED pair (k_pairing_coop_rows; msgset.cuh): Bls12381G2Impl over a registered
// message.  Pair 0 is (pk, H(m)) with H(m)'s 68 normalised rows (verify_shared.cuh group_lines_build, the *_LINES_N layout) read from
// the message set; pair 1 is (-g1, sig), whose G2 member lane pair 1 walks exactly as coop_miller2 (coop.cuh) walks a general pair:
// the same two job rounds per doubling, the same glue, the same bounds.
// The tabled line of entry e is n0_e + (c_e xP0) w^2 + yP0 w^3.  It does not depend on f or on the walk, so it is whole BEFORE its entry
// begins and multiplies f in the round that carries the walked pair's second job set -- three product rounds per doubling entry
// (coop_miller2 with fixed_g2 != 0), two per addition entry:
//   doubling   round 1  lane pairs 0..20 the squaring of f, 21..25 the walked pair's five jobs
//              round 2  0..17 f * line 0 (tabled), 18..23 the walked pair's six jobs; lane pair 31 loads row e + 1
//              round 3  0..17 f * line 1 (walked); lane pair 30 scales c_{e+1} xP0
//   addition   round A  0..17 f * line 0; lane pair 31 loads row e + 1         (the walked pair's addition step stays on its owner)
//              round B  0..17 f * line 1; lane pair 30 scales c_{e+1} xP0
// A row load is issued after the round's products and staged to LDS after the reduction that follows -- the only memory reads of
// the loop -- and no value is held across a call.  No lane pair multiplies a slot that nobody staged.
// Slots, all inside coop_shared as coop.cuh declares it:
//   S.line[0][0..2]   n0, c xP0, (yP0, 0): the tabled line          S.job[0][0][0..1]   c of the staged row, (xP0, 0)
//   S.line[1][0..2]   the walked line                               S.job[1][j], S.res[1][j]   the walked pair's jobs
// Device code; tests/hostsim_coop_rows compiles the same functions on the host (one thread per lane pair) under the bound tracker.
#pragma once
#include "coop.cuh"

#define COOP_ROWS_SCALER 30               // the lane pair that scales c xP0
#define COOP_ROWS_LOADER 31               // the lane pair that reads the rows
// One product round.  kind 1: f <- f^2 (21 products);  2: f *= line `set` (18 products);  0: no product of f.  The next njobs lane pairs
// multiply the walked pair's staged jobs; scale: the scaler turns the staged row into the tabled line's w^2 coefficient; next: the row the
// loader reads (or null).
__device__ __forceinline__ void coop_rows_round(coop_shared& S, int kind, int set, int njobs, bool scale, const uint32_t* next) {
  __syncthreads();                 // lines, job operands and the staged row are in place
  const int q = coop_pair();
  const int nf = kind == 1 ? 21 : kind == 2 ? 18 : 0;
  const uint32_t *pa = nullptr, *pb = nullptr;
  uint32_t* pd = nullptr;
  if (q < nf) {
    if (kind == 1) {
      int i, j, w;
      coop_sqr_idx(q, i, j, w);
      pa = S.f.c[i];
      pb = S.f.c[j];
    } else {
      pa = S.f.c[q / 3];
      pb = S.line[set][q % 3];
    }
    pd = S.prod[q];
  } else if (q < nf + njobs) {
    const int j = q - nf;
    pa = S.job[1][j][0];
    pb = S.job[1][j][1];
    pd = S.res[1][j];
  } else if (q == COOP_ROWS_SCALER && scale) {
    pa = S.job[0][0][0];
    pb = S.job[0][0][1];
    pd = S.line[0][1];
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
  const bool stage = q == COOP_ROWS_LOADER && next;
  if (stage) {                     // issued here, consumed after the reduction
    fp2_load(n0, next);
    fp2_load(c, next + 2 * FP_NL);
  }
  if (kind == 1) coop_reduce<1>(S, S.f);
  else if (kind == 2) coop_reduce<2>(S, S.f);
  if (stage) {                     // nobody reads line 0 between its multiplication and the next round's barrier
    coop_st(S.line[0][0], n0);
    coop_st(S.job[0][0][0], c);
  }
}
__device__ __noinline__ void coop_rows_sqr_round(coop_shared& S, bool sqr, bool scale) { coop_rows_round(S, sqr ? 1 : 0, 0, 5, scale, nullptr); }
__device__ __noinline__ void coop_rows_line_round(coop_shared& S, int set, int njobs, bool scale, const uint32_t* next) {
  coop_rows_round(S, 2, set, njobs, scale, next);
}

// f ends as conj(f_{|x|,Q0}(P0) f_{|x|,Q1}(P1)) up to a factor in Fp2 (the rows are normalised), Q0 being the point whose rows are
// `rows`: 68 rows of 4 FP_NL words.
__device__ __noinline__ void coop_miller2_rows(coop_shared& S, const g1_aff* P, const aff<hfp2>& Q1, const uint32_t* rows) {
  const int me = coop_pair();
  const bool owner = me == 1;                    // of the walked pair
  hfp2 xp2, yp2;                                 // (xP1, 0), (yP1, 0): Fp scalings as Fp2 products, so that all jobs are alike
  fp2_from_fp(xp2, P[1].x);
  fp2_from_fp(yp2, P[1].y);
  g2_hom_t<hfp2> T;
  T.x = Q1.x;
  T.y = Q1.y;
  fp2_one(T.z);
  {  // f = 1, the constant parts of the tabled line, row 0
    hfp2 x;
    if (me < 6) {
      if (me == 0) fp2_one(x);
      else fp2_zero(x);
      coop_st(S.f.c[me], x);
    } else if (me == 6) {
      fp2_from_fp(x, P[0].y);
      coop_st(S.line[0][2], x);
    } else if (me == 7) {
      fp2_from_fp(x, P[0].x);
      coop_st(S.job[0][0][1], x);
    } else if (me == COOP_ROWS_LOADER) {
      hfp2 c;
      fp2_load(x, rows);
      fp2_load(c, rows + 2 * FP_NL);
      coop_st(S.line[0][0], x);
      coop_st(S.job[0][0][0], c);
    }
  }
  hfp2 l0, l2, l3, t;
  int row = 0;
  for (int i = 62; i >= 0; i--) {
    // ---- doubling step of the walked pair (coop_miller2's, on lane pair 1)
    hfp2 a, b, c, e, f, h, g, s;
    if (owner) {
      fp2_add(h, T.y, T.z);
      fp2_norm(h, h);
      coop_job_put(S, 1, 0, T.x, T.y);
      coop_job_put(S, 1, 1, T.y, T.y);
      coop_job_put(S, 1, 2, T.z, T.z);
      coop_job_put(S, 1, 3, T.x, T.x);
      coop_job_put(S, 1, 4, h, h);
    }
    coop_rows_sqr_round(S, i != 62, i == 62);
    if (owner) {
      coop_ld(a, S.res[1][0]);        // XY
      coop_ld(b, S.res[1][1]);        // B = Y^2
      coop_ld(c, S.res[1][2]);        // C = Z^2
      coop_ld(s, S.res[1][3]);        // X^2
      coop_ld(h, S.res[1][4]);        // (Y + Z)^2
      fp2_mul_xi(e, c);
      fp2_dbl(g, e);
      fp2_add(e, g, e);
      fp2_reduce(e, e);
      fp2_dbl(e, e);
      fp2_dbl(e, e);
      fp2_norm(e, e);                 // E = 3b'C
      fp2_dbl(f, e);
      fp2_add(f, f, e);               // F = 3E
      fp2_sub(h, h, b);
      fp2_sub(h, h, c);
      fp2_norm(h, h);                 // H = 2YZ
      fp2_sub(l0, b, e);
      fp2_norm(l0, l0);
      fp2_dbl(g, s);
      fp2_add(g, g, s);
      fp2_neg(g, g);
      fp2_norm(g, g);                 // -3X^2
      fp2_sub(t, b, f);
      fp2_norm(t, t);
      coop_job_put(S, 1, 0, a, t);    // XY (B - F)
      fp2_add(t, b, f);
      fp2_norm(t, t);
      coop_job_put(S, 1, 1, t, t);    // (B + F)^2
      coop_job_put(S, 1, 2, e, e);    // E^2
      coop_job_put(S, 1, 3, b, h);    // BH
      coop_job_put(S, 1, 4, g, xp2);  // l2
      coop_job_put(S, 1, 5, h, yp2);  // l3
    }
    bool more = row + 1 < MILLER_ENTRIES;
    coop_rows_line_round(S, 0, 6, false, more ? rows + (row + 1) * (4 * FP_NL) : nullptr);
    if (owner) {
      coop_ld(g, S.res[1][0]);
      fp2_dbl(g, g);
      fp2_reduce(T.x, g);             // X3 = 2XY(B - F)
      coop_ld(g, S.res[1][1]);
      coop_ld(s, S.res[1][2]);
      fp2_dbl(a, s);
      fp2_add(a, a, s);
      fp2_norm(a, a);
      fp2_dbl(a, a);
      fp2_dbl(a, a);                  // 12E^2
      fp2_sub(g, g, a);
      fp2_reduce(T.y, g);             // Y3 = (B + F)^2 - 12E^2
      coop_ld(g, S.res[1][3]);
      fp2_dbl(g, g);
      fp2_dbl(g, g);
      fp2_reduce(T.z, g);             // Z3 = 4BH
      coop_ld(l2, S.res[1][4]);
      coop_ld(l3, S.res[1][5]);
      coop_st(S.line[1][0], l0);
      coop_st(S.line[1][1], l2);
      coop_st(S.line[1][2], l3);
    }
    coop_rows_line_round(S, 1, 0, more, nullptr);
    row++;
    // ---- addition step (set bits of |x|)
    if ((BLS_X_ABS >> i) & 1) {
      if (owner) {
        miller_add_step(T, l0, l2, l3, Q1.x, Q1.y, P[1].x, P[1].y);
        coop_st(S.line[1][0], l0);
        coop_st(S.line[1][1], l2);
        coop_st(S.line[1][2], l3);
      }
      more = row + 1 < MILLER_ENTRIES;
      coop_rows_line_round(S, 0, 0, false, more ? rows + (row + 1) * (4 * FP_NL) : nullptr);
      coop_rows_line_round(S, 1, 0, more, nullptr);
      row++;
    }
  }
  coop_conj(S.f, S.f);
}
