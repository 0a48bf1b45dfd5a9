// Shared-message verification (blsgpu_verify_shared_batch, blsgpu_verify_shared_indexed_batch): Signature::verify for many
// (key, signature) items that come in GROUPS, each group under one message (reference src/signature.rs:130-138 per item, as
// PublicKeyShare::verify calls it for every share of a signing session, src/public_key_share.rs:55-72).  H(m) is computed and made
// affine once per group; an item then costs its identity checks, ONE inversion for its own two points, and the two-pair pairing.
// The per-item functions, shared by the kernels (tu_verify_shared.inc) and the host harness (tests/hostsim_verify_shared):
//   * shared_group_of: the group of item i of the batch -- the last group that starts at or before i (empty groups share their
//     start with the next one and own nothing);
//   * prepare_shared_item: core_verify's stage 1 (reference src/traits/sig_core.rs:126-145: signature identity, then key identity)
//     with the group's point given in affine form, into the two-pair layout of verify.cuh;
//   * shared_expand_src: where byte b of the per-item message buffer of the MessageAugmentation path comes from;
//   * group_lines_build: the normalised line table of one group's H(m) (Bls12381G2Impl), one inversion per group.
#pragma once
#include "verify.cuh"
#include "tower_split.cuh"

// offs: n_groups + 1 entries from 0, never decreasing; i < offs[n_groups]; n_groups >= 1
BLS_FN size_t shared_group_of(const uint64_t* offs, size_t n_groups, uint64_t i) {
  size_t lo = 0, hi = n_groups - 1;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo + 1) / 2;
    if (offs[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Bls12381G1Impl: P[0] = H (the group's point, NOT cofactor-cleared), Q[0] = pk, P[1] = sig, Q[1] = -[c] g2 (g2_negc_gen: the pair
// that balances an uncleared message point).  h.inf cannot happen for a hash output in practice; the slots then hold zeros, exactly
// what prepare_hashed_item leaves.
BLS_FN int prepare_shared_item(g1_aff* P, g2_aff* Q, const g2_jac& pk, const g1_jac& sig, const g1_aff& h) {
  if (jac_is_inf(sig)) return BLS_ERR_SIG_IDENTITY;
  if (jac_is_inf(pk)) return BLS_ERR_PK_IDENTITY;
  g1g2_to_aff(P[1], Q[0], sig, pk);
  P[0] = h;
  g2_negc_gen(Q[1]);
  return BLS_OK;
}
// Bls12381G2Impl: P[0] = pk, Q[0] = H (cleared), P[1] = -g1, Q[1] = sig.  swap: the two pairs change places -- the table form of the
// lane-split line kernel (k_lines2s_shared) walks pair 0's G2 member, which must be the signature, and evaluates the group's rows
// at pair 1's G1 member, the key.  The product of the two pairings does not depend on the order.
BLS_FN int prepare_shared_item(g1_aff* P, g2_aff* Q, const g1_jac& pk, const g2_jac& sig, const g2_aff& h, bool swap = false) {
  if (jac_is_inf(sig)) return BLS_ERR_SIG_IDENTITY;
  if (jac_is_inf(pk)) return BLS_ERR_PK_IDENTITY;
  const int a = swap ? 1 : 0, b = 1 - a;
  g1g2_to_aff(P[a], Q[b], pk, sig);
  Q[a] = h;
  g1_neg_gen(P[b]);
  return BLS_OK;
}

// ---- the line table of a group (Bls12381G2Impl, lane-split path).  The pair (pk_i, H(m_g)) has the same G2 member for every item
// of group g, so its 68 line values differ between items only in where they are evaluated: the rows
//     (n0, c)_e = (l0 / h, g / h)_e       with (l0, g, h)_e the coefficients of entry e's tangent or chord (pairing.cuh)
// are computed once per group and the line value at P = (x, y) is n0 + (c x) w^2 + y w^3 -- the normalised form of
// g2neg_lines.cuh *_LINES_N, what tower.cuh lines_merge_y takes.  Layout: SHARED_ROW_WORDS words per entry (n0.c0, n0.c1, c.c0,
// c.c1, FP_NL limbs each, canonical), entry e of group g at word (g 68 + e) SHARED_ROW_WORDS: 15,232 bytes per group.
#define SHARED_ROW_WORDS (4 * FP_NL)
#define SHARED_TABLE_WORDS (MILLER_ENTRIES * SHARED_ROW_WORDS)
// Walks Q = (qx, qy) through the 68 entries once and leaves the rows through `io`; ONE inversion, by a running product over the 68
// h values.  io.st(e, slot, v) / io.ld(v, e, slot) keep entry e's values between the two passes: slots 0 and 1 are the two Fp2 of
// the table row (first l0 and g as they come, at the end n0 and c through io.st_canon), slots 2 and 3 a scratch row of the same
// size (h and the running product).  F2: fp2, or hfp2 on a lane pair (the host emulation of tower_split.cuh included).
// Returns false when Q is the identity or some h vanishes (neither happens for a hash output): the rows are then meaningless and
// the caller takes the general two-pair form.
template <class F2, class IO>
BLS_FN bool group_lines_build(const F2& qx, const F2& qy, bool q_inf, const IO& io) {
  g2_hom_t<F2> T;
  T.x = qx;
  T.y = qy;
  fp2_one(T.z);
  fp one;
  fp_one(one);
  const miller_regs<F2> st = {T, one, one, &qx, &qy};      // evaluated at (1, 1): the steps leave l2 = g and l3 = h
  bool ok = !q_inf;
  F2 l0, g, h, pre;
  for (int e = 0; e < MILLER_ENTRIES; e++) {
    if (miller_entry_is_add(e)) miller_add_step_at(st, l0, g, h);
    else miller_dbl_step_at(st, l0, g, h);
    fp2_mul_fp(l0, l0, one);                                // every stored value is a product: what fp_store / fp_load carry
    if (fp2_is_zero(h)) ok = false;
    if (e == 0) pre = h;
    else fp2_mul(pre, pre, h);
    io.st(e, 0, l0);
    io.st(e, 1, g);
    io.st(e, 2, h);
    io.st(e, 3, pre);
  }
  F2 inv, hi;
  fp2_inv(inv, pre);                                        // 0 -> 0: a vanished h leaves zero rows
  for (int e = MILLER_ENTRIES - 1; e >= 0; e--) {
    if (e) {
      io.ld(pre, e - 1, 3);
      fp2_mul(hi, inv, pre);                                // 1 / h_e
      io.ld(h, e, 2);
      fp2_mul(inv, inv, h);
    } else {
      hi = inv;
    }
    io.ld(l0, e, 0);
    io.ld(g, e, 1);
    fp2_mul(l0, l0, hi);
    fp2_mul(g, g, hi);
    io.st_canon(e, 0, l0);
    io.st_canon(e, 1, g);
  }
  return ok;
}

// MessageAugmentation: every item hashes pk_i || m, so nothing is shared and the call hands run_verify_items one message per item.
// Item j's copy of its group's message starts at x_offs[j] = sum over the items before it of their groups' message lengths; byte b
// of that buffer belongs to the last item j with x_offs[j] <= b whose message is not empty, which is what the same search over the
// n_items + 1 entries of x_offs finds (items with empty messages share their offset with the next one).  Returns the byte's place
// in the callers' message blob.
BLS_FN uint64_t shared_expand_src(const uint64_t* x_offs, size_t n_items, const uint64_t* item_offs, size_t n_groups,
                                  const uint64_t* msg_offs, uint64_t b) {
  const size_t j = shared_group_of(x_offs, n_items, b);
  const size_t g = shared_group_of(item_offs, n_groups, (uint64_t)j);
  return msg_offs[g] + (b - x_offs[j]);
}

#if defined(__HIPCC__)
#include "kernels.cuh"
// where a lane pair that runs group_lines_build (k_group_lines; tu_keyset.inc k_keyset_lines) keeps a point's values: this lane's
// component (real on the even lane, imaginary on the odd one) of the two Fp2 of entry e's table row (slots 0, 1) and scratch row
// (slots 2, 3)
struct group_lines_io {
  uint32_t* row;
  uint32_t* scr;
  __device__ __forceinline__ uint32_t* at(int e, int slot) const {
    return (slot < 2 ? row : scr) + (size_t)e * SHARED_ROW_WORDS + (slot & 1) * (2 * FP_NL);
  }
  __device__ __forceinline__ void st(int e, int slot, const hfp2& v) const { fp_store(at(e, slot), v.v); }
  __device__ __forceinline__ void ld(hfp2& v, int e, int slot) const { fp_load(v.v, at(e, slot)); }
  __device__ __forceinline__ void st_canon(int e, int slot, const hfp2& v) const {
    fp t;
    fp_canon(t, v.v);
    fp_store(at(e, slot), t);
  }
};
// ---- kernels (tu_verify_shared1.hip: Bls12381G1Impl and the group-independent one, tu_verify_shared2.hip: Bls12381G2Impl)
// the n_groups hash outputs (RAW_PROJ, group SG) -> RAW_AFFINE records, all-zero for the identity: one inversion per GROUP
template <int SG>
__global__ void k_group_affine(size_t n_groups, const uint8_t* hashes, uint8_t* aff);
// one item per lane: its group by shared_group_of over the item's index IN THE BATCH, the identity checks folded into status[i],
// and its two-pair record with one inversion.  A status other than BLS_OK leaves the pair slots unwritten: every later stage
// skips the item on its status.
// swap (Bls12381G2Impl): the pair order of the table form, see prepare_shared_item; group_of != nullptr: item i's group is left there
template <int SG>
__global__ void k_prepare_shared(size_t n, size_t n_groups, const uint64_t* item_offs, const uint8_t* pks, const uint8_t* sigs, int fmt,
                                 const uint8_t* group_aff, uint32_t* pairs, int32_t* status, int swap, uint32_t* group_of);
// Bls12381G2Impl, lane-split path: one lane pair per group runs group_lines_build on the group's affine point (RAW_AFFINE record)
// into table / scratch (SHARED_TABLE_WORDS words per group each); flags[g] = 1 when the group's rows are unusable, and then
// flags[n_groups] = 1 as well (the caller clears that word before the launch)
__global__ void k_group_lines(size_t n_groups, const uint8_t* group_aff, uint32_t* table, uint32_t* scratch, int32_t* flags);
// the per-item message buffer of the MessageAugmentation path: out[b] = msgs[shared_expand_src(b)], one byte per lane
__global__ void k_shared_expand(size_t total, const uint64_t* x_offs, size_t n_items, const uint64_t* item_offs, size_t n_groups,
                                const uint64_t* msg_offs, const uint8_t* msgs, uint8_t* out);
#endif
