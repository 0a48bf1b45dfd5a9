// Operation table of the field / tower self-test door (blsgpu_debug_field_op, include/blsgpu.h): ONE list that the device
// kernels (tu_debug_ops*.hip), the host entry (blsgpu.hip) and, through blsgpu_debug_field_op_shape, the Python binding read.
// Elements cross the door in the internal form: fourteen signed 32-bit limbs of 28 bits (fp.cuh), R = 2^392.
//     X(name, id, lanes, n_in, n_out, n_par, chain)
// lanes: 1 = one item per lane (the code of k_prepare, the MSM and the point kernels), 2 = one item per lane pair (hfp2: item j
// on lanes 2j and 2j + 1, 32 items per workgroup), 64 = one item per 64-lane workgroup (the wave-cooperative engine of coop.cuh on a
// __shared__ coop_shared, launched with BLS_BLOCK threads as k_pairing_coop is).  n_in / n_out: Fp limb vectors per record; an Fp2 is two of them (c0, c1), an
// Fp12 twelve, in tower order (c0.a0, c0.a1, c0.a2, c1.a0, c1.a1, c1.a2).  n_par: small integers after the input vectors.
// chain: reps > 1 is allowed and feeds the output back as the first operand.
// lanes = 4: one item per four adjacent lanes (item j on lanes 4j .. 4j + 3, 16 items per workgroup): both lane pairs are loaded with
// the same lane-split point, as k_msm_chunk_g2q holds it, and each pair writes the point it ends with.
// Point records: a Jacobian point is its coordinates X, Y, Z in that order -- three limb vectors over Fp, six over Fp2 (c0 then c1 of
// each); an affine operand is (x, y); outputs likewise.  A scalar crosses in the parameter slots as little-endian 32-bit words (a word
// of 2^31 or more as the negative int32 with the same bits).  The identity is any point with Z = 0 mod p.
// The last parameter of every lanes = 64 row is `fill`: the word the kernel writes over the whole coop_shared before it stages the
// operands.  An Fp12 crosses the door in tower order there too; the kernel maps it to the w-power slots of coop_f12 as k_finalexp_coop does.
#pragma once

#define BLS_DEBUG_OPS(X)                                                                                            \
  /* ---- one lane per item */                                                                                      \
  X(FP_NORM, 0, 1, 1, 1, 0, 0)         /* fp_norm */                                                                 \
  X(FP_REDUCE, 1, 1, 1, 1, 0, 0)       /* fp_reduce */                                                               \
  X(FP_CANON, 2, 1, 1, 2, 0, 0)        /* out0 = fp_canon; out1 = [fp_is_zero, fp_to_raw words 0..11, 0] */          \
  X(FP_REDUCE_LIN2, 3, 1, 2, 1, 2, 0)  /* fp_reduce_lin2(a, ka, b, kb) */                                            \
  X(FP_MUL, 4, 1, 2, 1, 0, 1)          /* fp_mul */                                                                  \
  X(FP_SQR, 5, 1, 1, 1, 0, 1)          /* fp_sqr */                                                                  \
  X(FP_INV, 6, 1, 1, 1, 0, 0)          /* fp_inv (constant-time safegcd) */                                          \
  X(FP_INV_VAR, 7, 1, 1, 1, 0, 0)      /* fp_inv_var */                                                              \
  X(FP_SQRT, 8, 1, 1, 2, 0, 0)         /* out0 = fp_sqrt root; out1 = [fp_sqrt flag, fp_is_square, 0..] */           \
  X(FP_FROM_RAW, 9, 1, 1, 1, 0, 0)     /* in0 = [raw words 0..11, 0, 0]; out = fp_from_raw */                        \
  X(FP2_KARA_PRODUCTS, 10, 1, 4, 2, 0, 0) /* fp2_kara_products(a0, a1, b0, b1) -> c0, c0 + c1 */                     \
  X(FP2_KARA_DIFFS, 11, 1, 4, 2, 0, 0)    /* fp2_kara_diffs */                                                       \
  X(FP2L_MUL, 12, 1, 4, 2, 0, 0)       /* one-lane fp2_mul (tower.cuh fp2) */                                        \
  X(FP2L_SQR, 13, 1, 2, 2, 0, 0)       /* one-lane fp2_sqr */                                                        \
  X(FP2L_INV, 14, 1, 2, 2, 0, 0)       /* one-lane fp2_inv */                                                        \
  /* ---- two lanes per item: lane-split Fp2 */                                                                     \
  X(FP2_MUL, 20, 2, 4, 2, 0, 1)        /* fp2_mul (fp2_mul_split_leaf) */                                            \
  X(FP2_SQR, 21, 2, 2, 2, 0, 1)        /* fp2_sqr */                                                                 \
  X(FP2_MUL_XI, 22, 2, 2, 2, 0, 0)     /* fp2_mul_xi */                                                              \
  X(FP2_MUL_FP, 23, 2, 3, 2, 0, 0)     /* fp2_mul_fp(a, k): in = a.c0, a.c1, k */                                    \
  X(FP2_CONJ, 24, 2, 2, 2, 0, 0)       /* fp2_conj */                                                                \
  X(FP2_INV, 25, 2, 2, 2, 0, 0)        /* fp2_inv (fp_inv_pair) */                                                   \
  X(F12_PACK, 26, 2, 12, 12, 0, 0)     /* sh_st_f12 then sh_ld_f12 */                                                \
  /* ---- two lanes per item: the accumulator in LDS */                                                             \
  X(F12_SH_SQR, 30, 2, 12, 12, 0, 1)        /* f12_sh_sqr */                                                         \
  X(F12_SH_MUL, 31, 2, 24, 12, 0, 1)        /* f12_sh_mul(acc, b) */                                                 \
  X(F12_SH_MUL_LINE, 32, 2, 18, 12, 0, 1)   /* f12_sh_mul_line(acc, l0, l2, l3) */                                   \
  X(F12_SH_MUL_2LINES, 33, 2, 24, 12, 0, 1) /* f12_sh_mul_2lines(acc, a0, a2, a3, b0, b2, b3) */                     \
  X(F12_SH_MUL_LINE5, 34, 2, 22, 12, 0, 1)  /* f12_sh_mul_line5(acc, c0, c2, c4, c3, c5) */                          \
  X(F12_SH_CYC_SQR, 35, 2, 12, 12, 0, 1)    /* f12_sh_cyclotomic_sqr */                                              \
  /* ---- two lanes per item: compressed squarings on (z2, z3, z4, z5) */                                           \
  X(CYC_C_SQR, 40, 2, 8, 8, 0, 1)           /* f12_sh_cyc_c_sqr_body (packed slots) */                               \
  X(CYC_C_SQR_UNPACKED, 41, 2, 8, 8, 0, 1)  /* f12_sh_cyc_c_sqr_unpacked_body */                                     \
  X(CYC_C_SQR_KARA, 42, 2, 8, 8, 0, 1)      /* cyck_from_split, f12_sh_cyc_c_sqr_kara_body, cyck_to_split */         \
  /* ---- two lanes per item: other Fp12 operations on fp12_t<hfp2> */                                              \
  X(F12_POW_X, 50, 2, 12, 12, 0, 0)    /* fp12_pow_x */                                                              \
  X(F12_INV, 51, 2, 12, 12, 0, 0)      /* fp12_inv */                                                                \
  X(F12_FROB1, 52, 2, 12, 12, 0, 0)    /* fp12_frob<1> */                                                            \
  X(F12_FROB2, 53, 2, 12, 12, 0, 0)    /* fp12_frob<2> */                                                            \
  /* ---- one 64-lane workgroup per item: coop.cuh */                                                               \
  X(COOP_MUL, 60, 64, 24, 12, 2, 1)    /* coop_mul(S, dst, a, b); par = alias (0: own dst, 1: dst = a, 2: dst = b), fill */ \
  X(COOP_SQR, 61, 64, 12, 12, 1, 1)    /* coop_sqr; par = fill */                                                    \
  X(COOP_MUL_LINE, 62, 64, 18, 12, 2, 1) /* coop_mul_line(S, f, set): in = f, l0, l2, l3; par = set, fill (the other set: the line rotated) */ \
  X(COOP_CYC_SQR, 63, 64, 12, 12, 2, 1)  /* coop_cyc_sqr; par = alias (0: own dst, 1: dst = a), fill */              \
  X(COOP_POW_X, 64, 64, 12, 12, 1, 0)    /* coop_pow_x */                                                            \
  X(COOP_CONJ, 65, 64, 12, 12, 1, 0)     /* coop_conj */                                                             \
  X(COOP_FROB1, 66, 64, 12, 12, 1, 0)    /* coop_frob<1> */                                                          \
  X(COOP_FROB2, 67, 64, 12, 12, 1, 0)    /* coop_frob<2> */                                                          \
  X(COOP_JOBS, 68, 64, 48, 24, 2, 0)     /* coop_jobs(S, njobs): in = job[k][j][0], job[k][j][1] for k < 2, j < 6; out = res[k][j] (fill where not computed); par = njobs, fill */ \
  X(COOP_SQR_MUL_JOBS, 69, 64, 52, 32, 1, 0)  /* coop_sqr_with_jobs: in = f, job[k][j][0..1] for j < 5; out = f^2, res[k][j] */ \
  X(COOP_LINE_MUL_JOBS, 70, 64, 66, 36, 2, 0) /* coop_mul_line_with_jobs: in = f, l0, l2, l3, job[k][j][0..1] for j < 6; out = f * line, res[k][j]; par = set, fill */ \
  X(COOP_FINAL_EASY, 71, 64, 12, 12, 1, 0)    /* coop_final_easy on S.f */                                           \
  X(COOP_FINAL_VERDICT, 72, 64, 12, 1, 1, 0)  /* coop_final_verdict on S.f: out limb 0 = the status */                \
  /* ---- one lane per item: the curve layer on jac<fp> (curve.cuh, msm2.cuh) */                                    \
  X(G1_DBL, 80, 1, 3, 3, 1, 1)         /* jac_dbl (par = form: 0 the non-inlined function, 1 jac_dbl_body) */        \
  X(G1_ADD, 81, 1, 6, 3, 1, 1)         /* jac_add / jac_add_body(p, q); chain: p <- p + q */                         \
  X(G1_MADD, 82, 1, 5, 3, 1, 1)        /* jac_madd / jac_madd_body(p, x2, y2); chain: p <- p + (x2, y2) */           \
  X(G1_TO_AFF, 83, 1, 3, 3, 0, 0)      /* jac_to_aff: out = x, y, [inf, 0..] */                                      \
  X(G1_MUL_U64, 84, 1, 3, 3, 2, 0)     /* jac_mul_u64; par = k as two 32-bit words */                                \
  X(G1_MUL_SCALAR, 85, 1, 3, 3, 8, 0)  /* jac_mul_scalar; par = k as eight 32-bit words */                           \
  X(G1_IN_SUBGROUP, 86, 1, 2, 1, 1, 0) /* g1_in_subgroup(x, y; par = inf): out limb 0 = the verdict */               \
  /* ---- one lane per item: the curve layer on jac<fp2> */                                                         \
  X(G2L_DBL, 90, 1, 6, 6, 1, 1)        /* jac_dbl / jac_dbl_body */                                                  \
  X(G2L_ADD, 91, 1, 12, 6, 1, 1)       /* jac_add / jac_add_body */                                                  \
  X(G2L_MADD, 92, 1, 10, 6, 1, 1)      /* jac_madd / jac_madd_body */                                                \
  X(G2L_TO_AFF, 93, 1, 6, 5, 0, 0)     /* jac_to_aff: out = x, y, [inf, 0..] */                                      \
  X(G2L_MUL_U64, 94, 1, 6, 6, 2, 0)    /* jac_mul_u64 */                                                             \
  X(G2L_MUL_SCALAR, 95, 1, 6, 6, 8, 0) /* jac_mul_scalar */                                                          \
  X(G2L_IN_SUBGROUP, 96, 1, 4, 1, 1, 0) /* g2_in_subgroup */                                                         \
  X(G2L_PSI, 97, 1, 6, 6, 0, 0)        /* g2_psi */                                                                  \
  X(G2L_PSI2, 98, 1, 6, 6, 0, 0)       /* g2_psi2 */                                                                 \
  X(G2L_CLEAR, 99, 1, 6, 6, 0, 0)      /* g2_clear_cofactor<fp2> */                                                  \
  /* ---- two lanes per item: the curve layer on jac<hfp2> */                                                       \
  X(G2S_DBL, 100, 2, 6, 6, 1, 1)       /* jac_dbl / jac_dbl_body */                                                  \
  X(G2S_ADD, 101, 2, 12, 6, 1, 1)      /* jac_add / jac_add_body */                                                  \
  X(G2S_MADD, 102, 2, 10, 6, 1, 1)     /* jac_madd / jac_madd_body */                                                \
  X(G2S_PSI, 103, 2, 6, 6, 0, 0)       /* g2_psi */                                                                  \
  X(G2S_PSI2, 104, 2, 6, 6, 0, 0)      /* g2_psi2 */                                                                 \
  X(G2S_CLEAR, 105, 2, 6, 6, 0, 0)     /* g2_clear_cofactor<hfp2> */                                                 \
  /* ---- four lanes per item: jac_dbl_quad (curve_quad.cuh) */                                                     \
  X(G2Q_DBL, 110, 4, 6, 12, 0, 1)      /* out = the point as lane pair 0 holds it, then as lane pair 1 holds it */ \
  /* ---- the Miller steps (pairing.cuh) on g2_hom_t<fp2>, one lane per item: in = T (X, Y, Z), [xq, yq,] xp, yp; out = T', l0, l2, l3; */ \
  /* par = form (0: the non-inlined miller_*_step, 1: miller_*_step_at inlined through miller_regs); chain: T feeds back */ \
  X(MILLER1_DBL, 111, 1, 8, 12, 1, 1)  /* miller_dbl_step */                                                          \
  X(MILLER1_ADD, 112, 1, 12, 12, 1, 1) /* miller_add_step */                                                          \
  /* ---- ... and on g2_hom_t<hfp2>, two lanes per item: the same records and forms */                               \
  X(MILLER2_DBL, 113, 2, 8, 12, 1, 1)  /* miller_dbl_step */                                                          \
  X(MILLER2_ADD, 114, 2, 12, 12, 1, 1) /* miller_add_step */                                                          \
  /* ---- two lanes per item: merged line values (tower.cuh) and the row evaluation; out = c0, c2, c4, c3, c5 */      \
  X(LINES_MERGE, 115, 2, 12, 10, 0, 0)    /* lines_merge(a0, a2, a3, b0, b2, b3) */                                   \
  X(LINES_MERGE_Y, 116, 2, 11, 10, 0, 0)  /* lines_merge_y(a0, a2, a3, b0, b2, y): y one vector over Fp */            \
  X(LINES_MERGE_YY, 117, 2, 10, 10, 0, 0) /* lines_merge_yy(a0, a2, ya, b0, b2, yb): in = a0, a2, ya, b0, b2, yb */   \
  X(LINE3_ROW, 118, 2, 6, 6, 0, 0)        /* miller_line3_row(n0, c, x, y): in = n0, c, x, y; out = l0, l2, l3 */

enum {
#define X(name, id, lanes, nin, nout, npar, chain) DBG_##name = id,
  BLS_DEBUG_OPS(X)
#undef X
};

#define DBG_NL 14   // limbs per Fp (FP_NL)

#if defined(__HIPCC__)
#ifndef BLS_BLOCK
#define BLS_BLOCK 64
#endif
#ifndef BLS_SPLIT_WAVES
#define BLS_SPLIT_WAVES 2
#endif
// in: n records of rec_in 32-bit words (the input vectors, then the parameters), out: n records of rec_out words
__global__ void k_dbg_fp1(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out);
__global__ void k_dbg_fp2s(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out);
__global__ void k_dbg_f12acc(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out);
__global__ void k_dbg_cyc(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out);
__global__ void k_dbg_f12misc(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out);
__global__ void k_dbg_coop(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out);
__global__ void k_dbg_pt1(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out);
__global__ void k_dbg_pt2s(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out);
__global__ void k_dbg_g2q(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out);
__global__ void k_dbg_miller1(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out);
__global__ void k_dbg_miller2s(int op, size_t n, int reps, const int32_t* in, int rec_in, int32_t* out, int rec_out);
// blsgpu_debug_map_to_curve: the G1 point at WREC_P0 of n cut-check records (engine values, Jacobian) -> RAW_PROJ
__global__ void k_dbg_rec_g1_to_raw(size_t n, const uint32_t* rec, uint8_t* out);
#endif
