/* blsgpu.h -- C ABI of libblsgpu.so: MI355X-native batch BLS12-381 signature verification.
 *
 * This is the drop-in boundary for the verify path of dashpay/agora-blsful (`blsful` 3.0.0-pre8).  Each entry
 * point names the reference interface it replaces (file:line relative to the reference crate); INTEGRATION.md
 * shows the Rust binding a maintainer adds behind a `hip` cargo feature.
 *
 * Conventions
 *   - Every buffer is caller-owned and borrowed for the duration of the call.  Pointers may be host pointers or
 *     HIP device pointers; the library detects which (hipPointerGetAttributes) and stages host buffers itself.
 *   - All calls are blocking, thread-safe and deterministic.  Each bound device owns a small pool of contexts (stream +
 *     workspace, BLSGPU_CONTEXTS, default 2): concurrent callers lease different contexts and overlap on the device.
 *   - Return value: 0 = the call ran (look at the status outputs), < 0 = runtime failure (HIP error, bad argument);
 *     blsgpu_last_error() then gives a message.  There is NO CPU fallback: without a usable gfx950 device every
 *     compute entry point fails with BLSGPU_E_NO_DEVICE.
 *   - sig_group selects the reference's backend type: 1 = Bls12381G1Impl (signature in G1, public key in G2,
 *     src/impls/g1.rs), 2 = Bls12381G2Impl (signature in G2, public key in G1, src/impls/g2.rs).
 *   - scheme = SignatureSchemes (src/sig_types.rs:6-13): 0 Basic, 1 MessageAugmentation, 2 ProofOfPossession.
 *   - Point formats (fmt):
 *       BLSGPU_FMT_RAW_PROJ    Jacobian (X, Y, Z), Montgomery form, little-endian limbs: the in-memory layout of
 *                              blst_p1 (144 B) / blst_p2 (288 B) that G1Projective / G2Projective wrap; Z = 0 is
 *                              the identity.  A `&[PublicKey<C>]` slice can be passed as it is.  RAW points are what the
 *                              reference's types hold -- members of the prime-order subgroups (from_bytes checks it);
 *                              verification relies on that (its verdict for a point outside its subgroup, which no
 *                              reference value can be, is unspecified).
 *       BLSGPU_FMT_RAW_AFFINE  (x, y) Montgomery, 96 B / 192 B; all-zero = identity.
 *       BLSGPU_FMT_COMPRESSED  ZCash compressed encoding 48 B / 96 B (modern), checked on decode.
 *       BLSGPU_FMT_LEGACY      Dash legacy header variant of the same (src/impls/legacy.rs:9-67).
 *   - Scalars are 32 bytes little-endian.
 *   - Status codes mirror BlsError (src/error.rs:5-55) on this path; the shim maps them back to the exact
 *     variants and strings.
 */
#ifndef BLSGPU_H
#define BLSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLSGPU_FMT_RAW_PROJ 0
#define BLSGPU_FMT_RAW_AFFINE 1
#define BLSGPU_FMT_COMPRESSED 2
#define BLSGPU_FMT_LEGACY 3

#define BLSGPU_SCHEME_BASIC 0
#define BLSGPU_SCHEME_AUG 1
#define BLSGPU_SCHEME_POP 2

/* per-item / per-call status (>= 0) */
#define BLSGPU_OK 0                  /* Ok(()) */
#define BLSGPU_INVALID_SIGNATURE 1   /* BlsError::InvalidSignature            sig_core.rs:144,176; secure_aggregation.rs:193 */
#define BLSGPU_SIG_IDENTITY 2        /* InvalidInputs("signature is the identity point")        sig_core.rs:127,156 */
#define BLSGPU_PK_IDENTITY 3         /* InvalidInputs("public key is the identity point") :132; aggregate form
                                        "public key at {aux0} is the identity point" (1-based)   sig_core.rs:163-166 */
#define BLSGPU_DUPLICATE_MESSAGE 4   /* InvalidInputs("duplicate messages detected at {aux0} and {aux1}") sig_basic.rs:51-55 */
#define BLSGPU_INVALID_COEFFICIENT 5 /* BlsError::InvalidCoefficient           secure_aggregation.rs:99,326 */
#define BLSGPU_BAD_LENGTH 6          /* BlsError::InvalidLength                public_key.rs:159-164 */
#define BLSGPU_BAD_ENCODING 7        /* BlsError::DeserializationError         legacy.rs:76-78,110,121 */
#define BLSGPU_LEGACY_FORMAT 8       /* BlsError::LegacyFormatError            legacy.rs:54-57 */
/* blsgpu_sig_proof_verify_batch only (src/traits/sig_proof.rs:110-128); there BLSGPU_INVALID_SIGNATURE stands for
 * BlsError::InvalidProof (:140) and BLSGPU_PK_IDENTITY for InvalidInputs("pk is the identity point") (:120-124) */
#define BLSGPU_COMMITMENT_IDENTITY 9 /* InvalidInputs("commitment is the identity point")        sig_proof.rs:110-114 */
#define BLSGPU_PROOF_IDENTITY 10     /* InvalidInputs("proof is the identity point")             sig_proof.rs:115-119 */
#define BLSGPU_ZERO_CHALLENGE 11     /* InvalidInputs("y is the zero")                           sig_proof.rs:125-127 */
/* blsgpu_combine_shares only */
#define BLSGPU_INVALID_SCHEME 12     /* BlsError::InvalidSignatureScheme       error.rs:19-20; signature.rs:152-154 */
#define BLSGPU_VSSS_ERROR 13         /* BlsError::VsssError                    error.rs:25-26,60-64 */
/* the threshold signcryption calls only */
#define BLSGPU_INVALID_DECRYPTION_SHARE 14 /* BlsError::InvalidDecryptionShare  sign_decryption_share.rs:45-62 */
#define BLSGPU_BAD_FRAME 15          /* no BlsError: decrypt returns None (no length prefix, or a length beyond the frame) sign_crypt.rs:122-136 */
/* blsgpu_elgamal_proof_verify_batch only: the three InvalidInputs of BlsElGamal::verify_proof, tested in this order */
#define BLSGPU_ELGAMAL_IDENTITY 16   /* InvalidInputs("Parameters or ciphertext values are identity point")   elgamal.rs:187-192 */
#define BLSGPU_ELGAMAL_ZERO_PROOF 17 /* InvalidInputs("Proof values are zero")                                elgamal.rs:193-195 */
#define BLSGPU_CHALLENGE_MISMATCH 18 /* InvalidInputs("Challenge values do not match")                        elgamal.rs:219-222 */

/* runtime failures (< 0): return codes.  One of them can also appear IN a status entry: BLSGPU_E_HIP when the device-side work of
 * that item failed (single-verdict checks run on workgroups that wait for each other with a bound; a wait that ran out is not a
 * verdict).  Calls whose statuses pass through host memory report it as their return code instead. */
#define BLSGPU_E_NO_DEVICE (-1)
#define BLSGPU_E_HIP (-2)
#define BLSGPU_E_ARG (-3)
#define BLSGPU_E_NOT_INIT (-4)

/* Library life cycle.  device = HIP ordinal, or -1 for the current device.  Idempotent for the same device; a second call
 * that names a DIFFERENT device fails with BLSGPU_E_ARG (shut down first to rebind). */
int blsgpu_init(int device);
/* One process driving several GPUs: binds the first ndev visible devices (ndev <= 0: all) and returns how many are bound
 * (or < 0).  blsgpu_verify_batch, blsgpu_multi_verify, blsgpu_aggregate_verify and blsgpu_verify_secure then shard
 * their items over the bound devices inside the library (contiguous ranges, one host thread per device) and fold the
 * per-device partial results -- key sums, Fp12 Miller products, MSM partials -- on device 0; results are identical to
 * the single-device ones.  The one-process-per-GPU alternative over RCCL is agora-blsful_amd/dist.py. */
int blsgpu_init_devices(int ndev);
int blsgpu_device_count(void);
void blsgpu_shutdown(void);
/* copies the last error message of the calling thread's most recent failing call; returns its length */
size_t blsgpu_last_error(char* buf, size_t cap);

/* NEW additive API (no batch entry exists in the reference: every reference call verifies one signature).
 * status[i] = verdict of  Signature::<C>::verify(&pk[i], msg[i])              src/signature.rs:130-138
 *   -> BlsSignature{Basic,MessageAugmentation,Pop}::verify                    src/traits/sig_basic.rs:36-38,
 *                                                                             sig_aug.rs:20-24, sig_pop.rs:37-39
 *   -> BlsSignatureCore::core_verify                                          src/traits/sig_core.rs:120-146
 * msgs is the concatenation of all messages, msg_offsets has n + 1 entries. */
int blsgpu_verify_batch(int sig_group, int scheme, const void* pks, const void* sigs, const uint8_t* msgs,
                        const uint64_t* msg_offsets, size_t n, int fmt, int32_t* status);

/* BlsSignatureCore::core_verify(pk, sig, msg, dst) for n items that share an explicit DST, no message augmentation
 * (reference src/traits/sig_core.rs:120-146).  pop_verify is core_verify(pk, sig, pk_bytes, POP_DST)
 * (src/traits/sig_pop.rs:67-70); the sharded verify_secure tail uses it with the scheme's DST. */
int blsgpu_core_verify(int sig_group, const uint8_t* dst, size_t dst_len, const void* pks, const void* sigs,
                       const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, int fmt, int32_t* status);

/* core_verify for n items whose message points H(m_i) are already known (RAW_PROJ, from blsgpu_hash_to_g1/g2 under the
 * scheme's DST): the identity checks of src/traits/sig_core.rs:126-135 in the reference's order, then the pairing check
 * (:137-145).  Lets a caller hash the message while it still adds up or exchanges keys.  All points RAW_PROJ. */
int blsgpu_core_verify_hashed(int sig_group, const void* pks, const void* sigs, const void* hashes, size_t n, int32_t* status);

/* MultiSignature::<C>::verify(MultiPublicKey::from_public_keys(pks), msg)     src/multi_signature.rs:127-135,
 * src/multi_public_key.rs:79-83 -> BlsMultiKey::from_public_keys (serial sum) src/traits/pk_multi.rs:7-13;
 * fused form BlsSignaturePop::multi_sig_verify                                src/traits/sig_pop.rs:42-49. */
int blsgpu_multi_verify(int sig_group, int scheme, const void* pks, size_t n, const void* sig, const uint8_t* msg,
                        size_t msg_len, int fmt, int32_t* status);

/* AggregateSignature::<C>::verify(&[(pk, msg)])                               src/aggregate_signature.rs:230-239
 *   -> scheme aggregate_verify (Basic: duplicate-message rejection)           src/traits/sig_basic.rs:41-64,
 *                                                                             sig_aug.rs:27-38, sig_pop.rs:52-58
 *   -> BlsSignatureCore::core_aggregate_verify                                src/traits/sig_core.rs:149-178
 * aux[0], aux[1] receive the indices that the reference formats into its error strings (see status codes). */
int blsgpu_aggregate_verify(int sig_group, int scheme, const void* pks, const uint8_t* msgs,
                            const uint64_t* msg_offsets, size_t n, const void* sig, int fmt, int32_t* status,
                            uint64_t* aux);

/* Signature::<C>::verify_secure(&pks, msg)                                    src/signature.rs:177-197
 * and verify_secure_with_mode(&pks, msg, format)                              src/signature.rs:256-276
 *   -> verify_secure_with_dst_internal                                        src/secure_aggregation.rs:173-208
 *   -> hash_public_keys_with_sorted[_mode]                                    src/secure_aggregation.rs:37-106,269-335
 * ser_format: 0 = Modern, 1 = Legacy (only sig_group 2 has 48-byte keys).  n == 0: Ok iff sig is the identity. */
int blsgpu_verify_secure(int sig_group, int scheme, const void* pks, size_t n, const void* sig, const uint8_t* msg,
                         size_t msg_len, int ser_format, int fmt, int32_t* status);

/* The coefficient step of hash_public_keys_with_sorted on already-serialised keys (width = 48 or 96 bytes each):
 * out_perm[i] = input index of the i-th key in sorted order; out_scalars[i] = t_i (32 B LE).
 * src/secure_aggregation.rs:41-103. */
int blsgpu_secure_coefficients(const uint8_t* key_bytes, size_t n, size_t width, uint32_t* out_perm,
                               uint8_t* out_scalars, int32_t* status);

/* The same step split for callers that shard the keys over several GPUs (agora-blsful_amd/dist.py): every rank sorts the
 * gathered key bytes on its device, ONE rank hashes the sorted stream (the only sequential part) and broadcasts the
 * 32-byte digest, every rank derives the coefficients of its own keys.
 *   blsgpu_sort_keys               out_perm[i] = input index of the i-th key in stable byte-lexicographic order  (:41-44)
 *   blsgpu_sorted_keys_digest      out_digest = SHA-256(keys concatenated in the order of perm)                  (:45-59)
 *   blsgpu_coefficients_for_range  t_i = SHA-256(BE32(i) || digest) mod r for the input keys [base, base + count):
 *                                  out_scalars[g - base] (32 B LE) belongs to input key g; *status OK or
 *                                  INVALID_COEFFICIENT                                                            (:61-100)
 *   blsgpu_first_occurrence        out_idx[p] = input index of the FIRST key equal to the p-th sorted key: the `position`
 *                                  search of aggregate_secure (duplicated keys take their first signature)        (:150-162) */
int blsgpu_sort_keys(const uint8_t* key_bytes, size_t n, size_t width, uint32_t* out_perm);
int blsgpu_sorted_keys_digest(const uint8_t* key_bytes, const uint32_t* perm, size_t n, size_t width, uint8_t* out_digest);
int blsgpu_coefficients_for_range(const uint8_t* digest, const uint32_t* perm, size_t n, size_t base, size_t count,
                                  uint8_t* out_scalars, int32_t* status);
int blsgpu_first_occurrence(const uint8_t* key_bytes, const uint32_t* perm, size_t n, size_t width, uint32_t* out_idx);

/* HashToPoint::hash_to_point(msg, dst)                                        src/traits/hash_to_point.rs:11,
 * impls src/impls/g1.rs:17-19 (group 1) and src/impls/g2.rs:15-17 (group 2).  out: RAW_PROJ points. */
int blsgpu_hash_to_g1(const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, const uint8_t* dst, size_t dst_len,
                      void* out);
int blsgpu_hash_to_g2(const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, const uint8_t* dst, size_t dst_len,
                      void* out);

/* BlsSignatureCore::aggregate_public_keys / aggregate_signatures              src/traits/sig_core.rs:38-59
 * (= BlsMultiKey::from_public_keys, src/traits/pk_multi.rs:7-13).  out: one RAW_PROJ point. */
int blsgpu_sum_g1(const void* pts, size_t n, int fmt, void* out);
int blsgpu_sum_g2(const void* pts, size_t n, int fmt, void* out);

/* sum_i scalars[i] * pts[i]: the loop `aggregated_pk += pk.0 * *coeff`        src/secure_aggregation.rs:201-204
 * (and the sign-side loop :163-166).  out: one RAW_PROJ point.  Scalars are taken modulo the group order r (a reference
 * Scalar is always < r; any 256-bit value is accepted and reduced) and the points must lie in the prime-order subgroup,
 * which every reference type guarantees. */
int blsgpu_msm_g1(const void* pts, const uint8_t* scalars, size_t n, int fmt, void* out);
int blsgpu_msm_g2(const void* pts, const uint8_t* scalars, size_t n, int fmt, void* out);

/* Pairing::pairing(&[(a_i, b_i)]).is_identity()                               src/traits/pairings.rs:50,
 * glue src/helpers.rs:41-63 (G1 member first).  *is_one = 1 iff the product of pairings is the identity. */
int blsgpu_pairing_product_is_one(const void* g1s, const void* g2s, size_t n, int fmt, int32_t* is_one);

/* point codec: to_bytes / from_bytes [_with_mode]                             src/public_key.rs:58-74,146-171,
 * src/impls/legacy.rs:85-170.  group = 1 (G1, 48 B) or 2 (G2, 96 B).  status[i]: 0 or BAD_ENCODING/LEGACY_FORMAT. */
int blsgpu_serialize(int group, const void* pts, size_t n, int fmt_in, int fmt_out, void* out, int32_t* status);

/* ProofOfPossession::<C>::verify(pk) for n pairs: pop_verify = core_verify(pk, proof, pk.to_bytes(), POP_DST)
 * (src/proof_of_possession.rs:79-81, src/traits/sig_pop.rs:67-70). */
int blsgpu_pop_verify_batch(int sig_group, const void* pks, const void* proofs, size_t n, int fmt, int32_t* status);

/* aggregate_secure / aggregate_secure_with_mode / AggregateSignature::from_signatures_secure: the signature that
 * verify_secure accepts, sum t_i * sig[idx_i] over the sorted keys (src/secure_aggregation.rs:110-169,338-352,
 * src/aggregate_signature.rs:191-227; duplicate keys pick the first matching signature, as the reference's position
 * search does).  out_sig: one RAW_PROJ point; *status: BLSGPU_OK or BLSGPU_INVALID_COEFFICIENT. */
int blsgpu_aggregate_secure(int sig_group, const void* pks, const void* sigs, size_t n, int ser_format, int fmt,
                            void* out_sig, int32_t* status);

/* OPT-IN grouped verification of independent items (sig_group 1 only): same arguments and status vector as
 * blsgpu_verify_batch (raw formats), but groups of eight items share one final exponentiation through a random linear
 * combination with 128-bit scalars; every group whose combined check fails is re-verified item by item, so
 *   - a valid item is never reported invalid, identity errors are reported as in blsgpu_verify_batch,
 *   - an invalid item is reported valid only if its group's combined check passes.
 * The scalars are derived INSIDE the library from the group's own inputs (SHA-256 over the keys, signatures and messages of
 * the group's eight items, their indices, n and `seed`; csrc/kernels.cuh grouped_scalar): whoever chooses the inputs learns
 * the scalars only once all of them are fixed, so forging takes about 2^128 hash evaluations per group (64-bit scalars, as
 * in round 3, could be ground offline in 2^64 by whoever knows `seed`).  `seed` SHOULD be a fresh random value per call: it makes
 * the scalars unpredictable even to someone who knows every other input.  It needs no secrecy afterwards.  Not the reference's semantics to the last bit (the reference has no batched
 * verification); callers opt in.  Pays on all-valid input; failing groups cost their items' ordinary verification on top. */
int blsgpu_verify_batch_grouped(int sig_group, int scheme, const void* pks, const void* sigs, const uint8_t* msgs, const uint64_t* msg_offsets,
                                size_t n, int fmt, uint64_t seed, int32_t* status);

/* Wire ingest: PublicKey::try_from / from_bytes_with_mode and Signature::from_bytes_with_mode -- checked decompression
 * (on curve, subgroup) of 48-byte (group 1) or 96-byte (group 2) encodings, modern or legacy header
 * (src/public_key.rs:58-74,158-171, src/signature.rs:231-253, src/impls/legacy.rs:39-82,100-126,144-170).
 * out: RAW_PROJ; status[i]: 0, BLSGPU_BAD_ENCODING or BLSGPU_LEGACY_FORMAT.  blsgpu_verify_batch also accepts
 * fmt = BLSGPU_FMT_COMPRESSED / BLSGPU_FMT_LEGACY directly (keys and signatures in the same format); a decode failure
 * becomes that item's status.  The order per item is the one a caller who deserialises first would see: the key's decode
 * status, then the signature's, and only for an item whose both decoded the identity checks (signature, then key) and the
 * pairing -- so an infinity key beside an undecodable signature is that signature's BAD_ENCODING / LEGACY_FORMAT. */
int blsgpu_deserialize(int group, const uint8_t* bytes, size_t n, int fmt_in, void* out, int32_t* status);

/* Signature::<C>::try_from(&[u8]) and Vec<u8>::from(&Signature<C>) (src/signature.rs:112-126): the serde_bare form of the
 * Signature enum is its variant index as one byte (0 Basic, 1 MessageAugmentation, 2 ProofOfPossession) followed by the
 * compressed point -- 49 bytes (Bls12381G1Impl) / 97 bytes (Bls12381G2Impl) per record, the lengths the reference asserts at
 * src/signature.rs:285-286.  n records back to back.  from_tagged: out_schemes[i] = the tag, out = RAW_PROJ points (checked
 * decompression incl. the subgroup test), status[i] = OK or BAD_ENCODING (unknown tag, invalid point; the reference maps
 * every serde error to InvalidInputs(..)). */
int blsgpu_signatures_from_tagged(int sig_group, const uint8_t* bytes, size_t n, uint8_t* out_schemes, void* out, int32_t* status);
int blsgpu_signatures_to_tagged(int sig_group, const uint8_t* schemes, const void* sigs, size_t n, int fmt, uint8_t* out);

/* Sharded aggregate verify (one process per GPU): the shard-local part of core_aggregate_verify
 * (src/traits/sig_core.rs:149-178).  out_f12 (576 B) = an Fp12 value whose final exponentiation is the product of the pairings
 * of the shard's (H(m_i), pk_i) pairs [times (sig, -g) when sig != NULL] -- a product of Miller values (for Bls12381G1Impl
 * taken at the message points before their cofactor clearing, the signature's at -[c] g2, c = h_eff^-1 mod r: the same
 * verdict); only products of such records and their final exponentiation are meaningful -- a record is defined up to factors that
 * the final exponentiation removes (the line values are scaled by elements of Fp2, differently from one library build to another), so
 * compare verdicts, never record bytes, and fold only records that ranks of ONE library build produced; *first_bad = local index of the first identity
 * key, n when the signature is the identity, -1 otherwise (identity pairs contribute 1 to the record, so it can always be
 * folded).  out_f12 and first_bad may be device pointers: then nothing crosses to the host and the caller hands them to
 * RCCL as they are.  Ranks exchange the records (all-gather) and finish with blsgpu_fp12_product_is_one.
 * Duplicate-message detection (Basic, src/traits/sig_basic.rs:46-58) is global: blsgpu_first_duplicate_message. */
int blsgpu_aggregate_partial(int sig_group, int scheme, const void* pks, const uint8_t* msgs, const uint64_t* msg_offsets,
                             size_t n, const void* sig, int fmt, void* out_f12, int64_t* first_bad);
int blsgpu_fp12_product_is_one(const void* f12s, size_t k, int32_t* is_one);
/* The Basic scheme's duplicate-message rule on its own (src/traits/sig_basic.rs:46-58), for sharded callers that gathered
 * the messages: out2 = (index of the earlier equal message, the first index whose message was seen before) -- the two
 * numbers of the reference's error string -- or (~0, ~0) when all messages are distinct.  Exact (bytes are compared). */
int blsgpu_first_duplicate_message(const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, uint64_t* out2);

/* ---- other two-pairing checks of the reference that reuse the same pairing stages ----
 *
 * SignCryptCiphertext::is_valid for n ciphertexts (u, v, w)               src/sign_crypt_ciphertext.rs:86-101
 *   -> BlsSignCrypt::valid: W' = H(u.to_bytes() || v), e(w, -g) * e(W', u) == 1, u and w not the identity
 *                                                                             src/traits/sign_crypt.rs:69-77,153-160
 * vs is the concatenation of the v fields, v_offsets has n + 1 entries.  status[i] == BLSGPU_OK <=> Choice(1); any other
 * status (INVALID_SIGNATURE, SIG_IDENTITY for w, PK_IDENTITY for u) <=> Choice(0). */
int blsgpu_signcrypt_valid_batch(int sig_group, int scheme, const void* us, const void* ws, const uint8_t* vs,
                                 const uint64_t* v_offsets, size_t n, int fmt, int32_t* status);

/* ProofOfKnowledge::<C>::verify(pk, msg, y) for n proofs (u = commitment, v = proof)   src/proof_of_knowledge.rs:132-164
 *   -> BlsSignatureProof::verify                                              src/traits/sig_proof.rs:102-142
 * (ProofOfKnowledgeTimestamp::verify derives y from (u, t) and runs the same check: blsgpu_sig_proof_timestamp_verify_batch).
 * ys: the challenges, 32 B little-endian canonical scalars.  status[i]: OK, COMMITMENT_IDENTITY, PROOF_IDENTITY,
 * PK_IDENTITY, ZERO_CHALLENGE (checked in that order) or INVALID_SIGNATURE (= BlsError::InvalidProof). */
int blsgpu_sig_proof_verify_batch(int sig_group, int scheme, const void* commitments, const void* proofs, const void* pks,
                                  const uint8_t* ys, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, int fmt,
                                  int32_t* status);

/* HashToScalar::hash_to_scalar(m, salt) for n inputs                           src/impls/g1.rs:25-27 -> src/helpers.rs:9-26
 * (ProofCommitmentChallenge::from_hash with KEYGEN_SALT, src/proof_commitment.rs:256-261; SecretKey::from_hash,
 * src/secret_key.rs:276-281): HKDF-SHA-256 extract with the salt over m || 0x00, expand to 48 bytes with info = 00 30, reduce
 * modulo r.  msgs is the concatenation of the inputs, msg_offsets has n + 1 entries.  out: n x 32 B little-endian canonical.
 * The reference repeats the expand while the result is zero, which cannot end; here a zero result is written as zero.
 * Not constant time: public inputs only. */
int blsgpu_hash_to_scalar(const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, const uint8_t* salt, size_t salt_len, uint8_t* out);

/* BlsSignatureProof::compute_y(u, t) for n commitments                         src/traits/sig_proof.rs:38-46
 * y = hash_to_scalar(u.to_bytes() || LE64(t), "BLS_POK__BLS12381_XOF:HKDF-SHA2-256_"): the modern compressed encoding of u whatever
 * fmt it came in (all four formats).  out_ys: n x 32 B, the form blsgpu_sig_proof_verify_batch reads.  A COMPRESSED / LEGACY
 * commitment that does not decode gets y = 0. */
int blsgpu_sig_proof_challenge_batch(int sig_group, const void* commitments, const uint64_t* timestamps, size_t n, int fmt, uint8_t* out_ys);

/* ProofOfKnowledgeTimestamp::<C>::verify(pk, msg, timeout_ms) for n proofs     src/proof_of_knowledge.rs:287-326
 *   -> BlsSignatureProof::verify_timestamp_proof                              src/traits/sig_proof.rs:145-166
 * timestamps: n x u64 milliseconds (the proof's t).  timeout_ms < 0: None.  The library reads no clock: now_ms is the caller's.
 * status[i] is what blsgpu_sig_proof_verify_batch gives the item with y = compute_y(u, t), except that, with a timeout and tested
 * before anything else (:154-161): t > now_ms puts BLSGPU_E_ARG into the slot (the reference panics there), and
 * now_ms - t > timeout_ms gives BLSGPU_INVALID_SIGNATURE (= InvalidProof) whatever the points are; elapsed == timeout_ms passes.
 * All four point formats; a COMPRESSED / LEGACY point that does not decode gives the item its decode status (BAD_ENCODING, ...:
 * commitment, proof, key in that order) unless the timeout rule applies. */
int blsgpu_sig_proof_timestamp_verify_batch(int sig_group, int scheme, const void* commitments, const void* proofs, const void* pks,
                                            const uint64_t* timestamps, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n,
                                            int fmt, uint64_t now_ms, int64_t timeout_ms, int32_t* status);

/* n independent products of two pairings: is_one[i] = Pairing::pairing(&[(g1a_i, g2a_i), (g1b_i, g2b_i)]).is_identity()
 * (src/traits/pairings.rs:50, src/helpers.rs:41-63) -- the shape of BlsSignCrypt::verify_share
 * (src/traits/sign_crypt.rs:192-207: pairs (-W', share), (w, pk); its identity checks stay with the caller).
 * Points must lie in the prime-order subgroups, which every reference type guarantees. */
int blsgpu_pairing2_check_batch(const void* g1a, const void* g2a, const void* g1b, const void* g2b, size_t n, int fmt,
                                int32_t* is_one);

/* n independent single pairings, the VALUE: out_gt[576 i ..) = Pairing::pairing(&[(g1s_i, g2s_i)]).to_bytes() (src/helpers.rs:41-63:
 * multi_miller_loop, then final_exponentiation) -- what TimeCryptCiphertext::decrypt (src/traits/time_crypt.rs:76-141) hashes.
 * Two facts fix these bytes, and they are pinned to different degrees:
 *   the value   The backend's final exponentiation raises to 3 (p^12 - 1) / r (its hard part is the chain whose exponent is
 *               (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3), so Gt is the CUBE of the textbook reduced pairing.  This library's chains are
 *               that chain; tests/test_timecrypt_cases.py checks the cube against a plain power, bilinearity and the order r.
 *   the bytes   ASSUMED, and not verifiable without the backend: the six Fp2 coefficients over w^0 .. w^5 (w^6 = xi; in tower terms
 *               c0.a0, c1.a0, c0.a1, c1.a1, c0.a2, c1.a2), each its real part, then its imaginary part, each part 48 bytes
 *               big-endian, the canonical residue (not Montgomery).  One place on the device (csrc/timecrypt.cuh gt_part_offset and
 *               gt_tower_wpow, through which both exports -- coop_gt_bytes of the one-wave kernels, fx_export of k_finalexp2s_value
 *               -- place every part) and one test function (tests/timecrypt_ref.py gt_bytes) know this order; should it be wrong,
 *               the fix is a permutation there.
 * fmt: any of the four BLSGPU_FMT_* (both members in the same format).  A COMPRESSED / LEGACY pair that does not decode gets its
 * decode status (the G1 member's first, then the G2 member's) and 576 zero bytes.  A pair with an identity member gets Gt one
 * (00 .. 01 in the first 48 bytes, then zeros) and BLSGPU_OK, as multi_miller_loop skips it.  RAW formats are not subgroup-checked,
 * as everywhere else.  status: n entries, BLSGPU_OK or a decode status.  Pointers may be host or device memory.  Launch sequence:
 * k_decompress x 2 (wire formats), k_pairing_value_prepare, then the pairing-value step.  Below BLSGPU_VALUE_SPLIT_MIN items (default
 * 8,192; 0: always) that is one wave per item (k_pairing_value) over chunks of at most 4,096 items; from it up, two lanes per item in
 * chunks of BLSGPU_MILLER_CHUNK items: k_linesp (pass 1), k_millerfp3, k_finalexp2s_value.  Both plans write the same bytes.  The call
 * runs on the first bound device. */
int blsgpu_pairing_batch(const void* g1s, const void* g2s, size_t n, int fmt, uint8_t* out_gt, int32_t* status);

/* TimeCryptCiphertext::decrypt(sig) (src/time_crypt_ciphertext.rs:38-50 -> BlsTimeCrypt::unseal, src/traits/time_crypt.rs:76-116) for
 * many ciphertexts grouped under one signature each -- a time-lock service publishes one signature per round, and every ciphertext
 * sealed to that round opens with it.  Group g is items item_offsets[g] .. item_offsets[g + 1] - 1 (n_groups + 1 offsets, from 0,
 * never decreasing, else BLSGPU_E_ARG; n = item_offsets[n_groups]), with signature sigs[g] (sig_group's group) and its scheme tag
 * sig_schemes[g] (0 / 1 / 2).  Item i has u_i (us, the key group), v_i (vs, n x 32 bytes), w_i = ws[w_offsets[i] .. w_offsets[i + 1])
 * (n + 1 offsets, as above; any length below 512 MiB, zero included) and its scheme tag ct_schemes[i].  fmt: any of the four
 * BLSGPU_FMT_* (signatures and u in the same format).  frames is as large as ws, with the same offsets; pt_range holds
 * (offset, length) per item, as in blsgpu_signcrypt_open_batch: the message of item i is frames[w_offsets[i] + offset ..) of that
 * length.  Pointers may be host or device memory.  Per item, exactly the reference:
 *   K = e(sig, u) (the G1 member first);  alpha = SHA-256(K.to_bytes()) xor v -- K.to_bytes() as blsgpu_pairing_batch states the
 *   assumption --;  frame = SHAKE128(alpha) xor w;  the frame's length prefix (the varint of blsgpu_signcrypt_open_batch): when
 *   `peek` FAILS the message is EMPTY and the check goes on (time_crypt.rs:89-102 -- not the signcryption rule), a length beyond the
 *   frame is None, otherwise the message is frame[overhead .. overhead + len);  r = hash_to_scalar(alpha || SHA-256(message)) under
 *   the salt "TIMELOCK_BLS12381_XOF:HKDF-SHA2-256_" (a zero r is kept as zero, as blsgpu_hash_to_scalar writes it, and fails);
 *   Some <=> g r == u, the scheme tags are equal, and neither sig nor u is the identity.
 * status[i] is the first that applies of: the decode status of u_i, then of sig_g (wire formats); BLSGPU_INVALID_SCHEME
 * (ct_schemes[i] != sig_schemes[g]); BLSGPU_SIG_IDENTITY; BLSGPU_PK_IDENTITY (u is the identity); BLSGPU_BAD_FRAME (a length beyond
 * the frame, only); BLSGPU_INVALID_SIGNATURE (g r != u); BLSGPU_OK.  status[i] == BLSGPU_OK <=> is_some().  An item that is not OK
 * gets pt_range (0, 0), and its frame bytes are not part of the contract.  Launch sequence: k_decompress x 2 (wire formats),
 * k_timecrypt_prepare, the pairing-value step of blsgpu_pairing_batch (either plan), then k_timecrypt_open, one lane per item; the
 * call runs on the first bound device. */
int blsgpu_timecrypt_open_batch(int sig_group, const void* sigs, const uint8_t* sig_schemes, const uint64_t* item_offsets, size_t n_groups,
                                const void* us, const uint8_t* vs, const uint8_t* ws, const uint64_t* w_offsets, const uint8_t* ct_schemes,
                                int fmt, uint8_t* frames, uint64_t* pt_range, int32_t* status);

/* Measurement hooks (not part of the reference interface): when enabled, every kernel launch of the library is
 * bracketed by HIP events on the library's own stream; blsgpu_profile_get returns the accumulated device time and
 * launch count per kernel since the last enable.  bench.py derives the roofline figures from these. */
int blsgpu_profile_enable(int on);
int blsgpu_profile_count(void);
int blsgpu_profile_get(int kernel_id, char* name, size_t name_cap, double* total_ms, uint64_t* launches);

/* Self-test / measurement hook of the row-wide Fp multiplier behind the single-verification latency path (csrc/wide.cuh):
 * out[i] = a[i] * b[i]^reps in Fp, elements as 48-byte Montgomery words (the coordinate format of RAW_PROJ). */
int blsgpu_debug_wide_mul(const uint8_t* a, const uint8_t* b, size_t n, int reps, uint8_t* out);
/* The same for the table-driven engine on top of it (csrc/wide_engine.cuh): runs `prog` (len steps of two words, the
 * format of csrc/wide_tables.cuh, Fp12 operations on the arrays F, T, U, W, ACC only) `reps` times on one workgroup with
 * F = U = W = ACC = the Fp12 at f_in (twelve 48-byte Montgomery elements) and T = 0; t_out <- T.  prog: host memory. */
int blsgpu_debug_wide_program(const uint32_t* prog, size_t len, int reps, const uint8_t* f_in, uint8_t* t_out);
/* Self-test hook of the engine operation by operation (not part of the reference interface): ANY table operation of either set on
 * caller-supplied limbs.  set: 0 = F12 (wide_tb_f12), 1 = PT (wide_tb_pt).  prog: len steps of two words, the format of
 * csrc/wide_tables.cuh, len <= the set's PROG_MAX; it runs `reps` times on each of n 256-thread workgroups (n <= 4096), one item
 * each.  Before staging every word of every value of an item's store is `fill`; then the set's constants are staged as the shipped
 * kernels stage them, and the n_in values in_idx names take the item's inputs: `in` is n x n_in x sixteen signed 32-bit words, the
 * internal form (28-bit limbs at words 0..13, R = 2^392, as blsgpu_debug_field_op passes them; words 14 and 15 as given).  After the
 * run the n_out values out_idx names come back the same way (out: n x n_out x sixteen words); the whole store may be asked for.
 * BLSGPU_E_ARG, and nothing is launched: an operation id that is neither in the set's table nor FPINV (set F12 only) -- the
 * hand-over built-ins ACQ, PUB, ACQF, PUBF are always refused --, a step whose destination or operand reference, extended by what
 * the operation reads or writes from it, passes the set's value count, an empty program or one longer than PROG_MAX, a value index
 * past the store.  The caller keeps the operands inside the engine's input contract (|value| < 0.6 p, limbs after a carry pass);
 * nothing else is checked here.  Host pointers. */
int blsgpu_debug_wide_steps(int set, const uint32_t* prog, size_t len, int reps, size_t n, const uint32_t* in_idx, size_t n_in, const int32_t* in,
                            int32_t fill, const uint32_t* out_idx, size_t n_out, int32_t* out);
/* Self-test hook of the batch final exponentiation + verdict on caller-supplied Fp12 records (576 B, the record format of
 * blsgpu_fp12_product_is_one).  form 0 = k_finalexp2s, 1 = k_finalexp_seg + k_cyc_run4, 2 = k_finalexps; chunk = items per chunk
 * of the chunked forms (0: the library's).  status is in/out: an entry that is not BLSGPU_OK on entry is skipped and left as it
 * is, as the verify path skips identity items; the others become BLSGPU_OK (fin^(3 (p^12 - 1) / r) == 1) or
 * BLSGPU_ERR_INVALID_SIGNATURE. */
int blsgpu_debug_finalexp_batch(const void* f12s, size_t n, int form, size_t chunk, int32_t* status);
/* Self-test hook of the final exponentiation WITH THE Gt EXPORT (k_finalexp2s_value, the lane-split kernel of the pairing-value
 * calls from BLSGPU_VALUE_SPLIT_MIN items up) on the same records: out_gt = n x 576 bytes, Gt::to_bytes() of fin^(3 (p^12 - 1) / r)
 * as assumed below.  chunk = items per chunk (0: the library's).  status[i] is read only, the item's flag as those calls set it:
 * 0 runs the chain, 1 gives Gt one, any other value 576 zero bytes. */
int blsgpu_debug_finalexp_value(const void* f12s, size_t n, size_t chunk, uint8_t* out_gt, const int32_t* status);
/* Self-test hook of the field leaves and the lane-split tower (not part of the reference interface): ONE operation of
 * csrc/debug_ops.h on n caller-supplied records.  Elements cross in the internal form -- fourteen signed 32-bit limbs of 28 bits
 * per Fp, R = 2^392 -- so that lazy, redundant and negative operands can be injected.  A record of `in` is n_in limb vectors
 * followed by n_par 32-bit parameters, a record of `out` n_out limb vectors (blsgpu_debug_field_op_shape; an Fp2 is two vectors,
 * an Fp12 twelve in tower order).  lanes = 1: one item per lane; 2: item j on lanes 2j and 2j + 1.  reps > 1 (operations with
 * chain = 1 only) feeds the output back as the first operand.  Host pointers.  The caller keeps the operands inside the input
 * contract of the function under test (fp.cuh); nothing is checked here. */
int blsgpu_debug_field_op_shape(int op, int* lanes, int* n_in, int* n_out, int* n_par, int* chain);
int blsgpu_debug_field_op(int op, const int32_t* in, size_t n, int reps, int32_t* out);
/* Self-test hook of the Miller accumulator's kernel (not part of the reference interface): k_millerf2s itself, launched as the
 * verify path launches it, on a caller-supplied line table.  lines: n x 68 entries x five Fp2 coefficients in the order c0, c2,
 * c4, c3, c5 (c0 then c1 of each, fourteen limbs each, reduced form).  status: an item that is not BLSGPU_OK is skipped and its
 * output left zero.  out_f12: n x twelve limb vectors in tower order.  Host pointers, n <= 4096. */
int blsgpu_debug_millerf(const int32_t* lines, size_t n, const int32_t* status, int32_t* out_f12);
/* Self-test hook of hash-to-curve behind expand_message_xmd (not part of the reference interface): the shipped kernels in their
 * compile-time form that reads the uniform bytes from memory where the product expands a message, so that the field elements
 * u0, u1 are the caller's choice (zero, equal, opposite, on a pole of the isogeny, at the edges of the 512-bit reduction).
 * uniform: n x 128 bytes (group 1) or n x 256 bytes (group 2), what expand_message_xmd would have produced.  out: n RAW_PROJ
 * points (Jacobian, Z = 0 for the identity).  uncleared = 1: the point before the cofactor clearing.  path: one kernel path;
 * a (group, path, uncleared) triple that no launch of the library uses is BLSGPU_E_ARG:
 *   group 1: LANE 0 / 1, PAIR 0 / 1, WIDE 0 / 1, WIDE_REC 1, ENGINE 0 / 1 (1: the cut check's record, program G1_HASH_MAP)
 *   group 2: LANE 0, PAIR 0 / 1, PAIR_CLEAR_WIDE 0, ENGINE 0, MAPS_TAIL 0
 * Host pointers, n <= 4096. */
#define BLSGPU_H2C_LANE 0             /* k_hash_to_g1 / k_hash_to_g2, one lane per item (the form the prepare kernels call) */
#define BLSGPU_H2C_PAIR 1             /* the same kernels, two lanes per item */
#define BLSGPU_H2C_WIDE 2             /* k_hash_to_g1_wide: one wave per item, point through `out` */
#define BLSGPU_H2C_ENGINE 3           /* k_hash_to_g1_engine / k_hash_to_g2_engine: one workgroup per item */
#define BLSGPU_H2C_MAPS_TAIL 4        /* k_hash_to_g2_maps, then k_g2_hash_tail_wide */
#define BLSGPU_H2C_WIDE_REC 5         /* k_hash_to_g1_wide writing the cut check's record (uncleared), converted to RAW_PROJ */
#define BLSGPU_H2C_PAIR_CLEAR_WIDE 6  /* k_hash_to_g2 on lane pairs without the clearing, then k_g2_clear_wide */
int blsgpu_debug_map_to_curve(int group, int path, int uncleared, const uint8_t* uniform, size_t n, void* out);
/* Self-test hook of the wave-cooperative pairing kernels (not part of the reference interface): the shipped kernels, launched as
 * the verify path launches them, on caller-supplied pairs.  pairs: n x twelve limb vectors in reduced form -- P.x, P.y, Q.x.c0,
 * Q.x.c1, Q.y.c0, Q.y.c1 of pair 0, then of pair 1 (affine; nothing is checked, the points need not lie in the subgroups).
 * fixed_g2 as the verify path passes it: 0 = two general pairs, 1 = pair 1's G2 member is -g2, 2 = it is the constant of
 * G2NEGC_LINES (pair 1's Q is then not read).  status is in/out: an item that is not BLSGPU_OK on entry is skipped.
 * mode 0: k_pairing_coop_easy; out_f12 gets the exported easy-part value miller(pairs)^((p^6 - 1)(p^2 + 1)) per item as twelve limb
 *         vectors in tower order, and every limb of a skipped item is BLSGPU_DEBUG_COOP_SENTINEL; status is left as it is.
 * mode 1: k_pairing_coop; status becomes BLSGPU_OK or BLSGPU_ERR_INVALID_SIGNATURE; out_f12 is not used.
 * mode 2: k_finalexp_coop; `pairs` is n x twelve limb vectors of an Fp12 in tower order instead, each run as slot 0 of a workspace of
 *         stride n; status becomes the verdict; out_f12 is not used.
 * Host pointers, n <= 4096. */
#define BLSGPU_DEBUG_COOP_SENTINEL ((int32_t)0xa5a5a5a5)
int blsgpu_debug_coop_pairing(int mode, int fixed_g2, const int32_t* pairs, size_t n, int32_t* status, int32_t* out_f12);
/* Self-test hook of the one-wave pairing kernel that reads a registered key's line rows (not part of the reference interface):
 * k_pairing_coop_keyed, launched as the verify path launches it.  pairs, status, out_f12 and the sentinel are those of
 * blsgpu_debug_coop_pairing with fixed_g2 = 2, except that pair 0's G2 member is entry idx[i] of `keyset`, a set created with
 * BLSGPU_KEYSET_LINES (Bls12381G1Impl): the record's own Q members are not read.  Every named entry must be a finite key with usable
 * rows; the rows of other entries are not defined.
 * mode 0: out_f12 gets the exported easy-part value per item, every limb of a skipped item is BLSGPU_DEBUG_COOP_SENTINEL, status is
 *         left as it is.   mode 1: status becomes BLSGPU_OK or BLSGPU_ERR_INVALID_SIGNATURE; out_f12 is not used.
 * BLSGPU_E_ARG: a set without line tables, an index that is not below the set's size, n > 4096, any other mode.  Host pointers. */
int blsgpu_debug_coop_pairing_keyed(int mode, uint64_t keyset, const uint32_t* idx, const int32_t* pairs, size_t n, int32_t* status, int32_t* out_f12);
/* Self-test hook of the kernels that PRODUCE line values on the lane-split path (not part of the reference interface): one shipped
 * kernel, launched with the grid, row stride, first / count, lines3 offset and pass order of the verify path / the product paths, one
 * chunk of `chunk` items after another (0: the library's own chunk).  items: n records of limb vectors in reduced form -- twelve per
 * two-pair item as blsgpu_debug_coop_pairing takes them, six (P.x, P.y, Q.x.c0, Q.x.c1, Q.y.c0, Q.y.c1) per one-pair item of the
 * product kernels.  status: an item that is not BLSGPU_OK (the product kernels: not zero) is skipped.  The line workspace holds the
 * byte pattern of BLSGPU_DEBUG_COOP_SENTINEL before every chunk and is read back before the next: every limb of a skipped item is the
 * sentinel, and *stray counts the words written where nothing may be: on lanes beyond a chunk's items, in the lines3 rows of the
 * two-pass forms for an item pass 1 skips, and anywhere else in the workspace behind the output rows.  out, per item and entry (68 entries in loop order):
 *   line5: five Fp2 coefficients c0, c2, c4, c3, c5 (c0 then c1 of each, fourteen limbs each) -- the layout blsgpu_debug_millerf takes;
 *   line3: three, l0, l2, l3.
 *   BLSGPU_LINES_2S        k_lines2s; variant = fixed_g2: 1, 2 one launch (pass 0), 0 passes 1 then 2                  -> line5 per item
 *   BLSGPU_LINES_2S_KEYED  k_lines2s_keyed: pair 0's G2 member is entry idx[i] of `keyset` (BLSGPU_KEYSET_LINES)         -> line5 per item
 *   BLSGPU_LINES_P1        k_linesp pass 1 (half = the chunk's count: no partners)                                      -> line3 per item
 *   BLSGPU_LINES_P12       k_linesp passes 1 and 2 over all n items, half = ceil(n / 2): virtual item v merges item v with item
 *                          v + half (absent for the last one when n is odd)                                             -> line5 per virtual item
 *   BLSGPU_LINES_P4        k_linesp4                                                                                    -> line3 per item
 *   BLSGPU_LINES_FIXED     k_lines_fixed; variant = fixed_g2 1, 2                                                       -> line3 of item 0
 *   BLSGPU_LINES_P_KEYED   k_linesp_keyed: item i < t_b reads the rows of entry idx[i], item i >= t_b the constant's     -> line3 per item
 *   BLSGPU_LINES_MILLER2S  k_miller2s, the one-kernel loop; variant = fixed_g2 0, 1, 2          -> twelve limb vectors per item, tower order
 * BLSGPU_E_ARG: another kernel or variant, a set without line tables, an index that is not below the set's size, n > 4096.  Host pointers. */
#define BLSGPU_LINES_2S 0
#define BLSGPU_LINES_2S_KEYED 1
#define BLSGPU_LINES_P1 2
#define BLSGPU_LINES_P12 3
#define BLSGPU_LINES_P4 4
#define BLSGPU_LINES_FIXED 5
#define BLSGPU_LINES_P_KEYED 6
#define BLSGPU_LINES_MILLER2S 7
int blsgpu_debug_lines(int kernel, int variant, const int32_t* items, size_t n, const int32_t* status, size_t chunk, uint64_t keyset, const uint32_t* idx, size_t t_b,
                       int32_t* out, uint64_t* stray);
/* Self-test hook of the two kernels whose pairs BOTH read their rows from one table in global memory (not part of the reference
 * interface): the signcryption share check by key index of Bls12381G2Impl.  points: m RAW_AFFINE G2 points (192 bytes each), made into
 * a table by the library's row builder; every point must be finite with usable rows.  pairs, status and the sentinel are those of
 * blsgpu_debug_coop_pairing with fixed_g2 = 0, except that pair 0's G2 member is entry t0[i] of the table and pair 1's entry t1[i]: the
 * records' own Q members are not read.
 * mode 0: k_pairing_coop_tables2 with the export: out gets the easy-part value per item (twelve limb vectors, tower order), every limb
 *         of a skipped item is the sentinel, status is left as it is.
 * mode 1: k_pairing_coop_tables2 as the verify path launches it: status becomes BLSGPU_OK or BLSGPU_ERR_INVALID_SIGNATURE.
 * mode 2: k_lines2s_tables2, one chunk of `chunk` items after another (0: the library's own chunk): out gets line5 per item and *stray
 *         the words written where nothing may be, both as BLSGPU_LINES_2S_KEYED of blsgpu_debug_lines.
 * BLSGPU_E_ARG: another mode, m = 0 or m > 4096, n > 4096, an index that is not below m, a point without usable rows.  Host pointers. */
int blsgpu_debug_tables2(int mode, const void* points, size_t m, const uint32_t* t0, const uint32_t* t1, const int32_t* pairs, size_t n, int32_t* status,
                         size_t chunk, int32_t* out, uint64_t* stray);
/* Self-test hooks of the one-wave pairing kernel that reads a registered message's line rows (not part of the reference interface).
 * blsgpu_debug_msgset_from_points: a message set (below: blsgpu_msgset_*) of scheme Basic whose n entries are the given RAW_AFFINE
 *   points of group sig_group (host or device memory) instead of hash outputs, so that crafted G2 points can reach the rows; flags as
 *   blsgpu_msgset_create.  Nothing is checked: an all-zero record is the identity.
 * blsgpu_debug_coop_pairing_rows: k_pairing_coop_rows, launched as the verify path launches it.  pairs, status, out_f12 and the
 *   sentinel are those of blsgpu_debug_coop_pairing with fixed_g2 = 0, except that pair 0's G2 member is entry msg_of[i] of `msgset`, a
 *   Bls12381G2Impl set with rows: the record's own pair-0 Q is not read.  Every named entry must be a finite point with usable rows;
 *   the rows of other entries are not defined.
 *   mode 0: out_f12 gets the exported easy-part value per item, every limb of a skipped item is BLSGPU_DEBUG_COOP_SENTINEL, status is
 *           left as it is.   mode 1: status becomes BLSGPU_OK or BLSGPU_ERR_INVALID_SIGNATURE; out_f12 is not used.
 *   BLSGPU_E_ARG: a set without rows, an index that is not below the set's size, n > 4096, any other mode.  Host pointers. */
int blsgpu_debug_msgset_from_points(int sig_group, const void* points, size_t n, int flags, uint64_t* out_handle);
int blsgpu_debug_coop_pairing_rows(int mode, uint64_t msgset, const uint32_t* msg_of, const int32_t* pairs, size_t n, int32_t* status, int32_t* out_f12);

/* Sign side, provided so that benchmarks and tests can build inputs on the device:
 * pk[i] = sk[i] * g (SecretKey::public_key, src/secret_key.rs:342-344) and
 * sig[i] = sk[i] * H(msg[i]) (BlsSignatureCore::core_sign, src/traits/sig_core.rs:108-117; the Aug scheme prefixes
 * the public-key bytes, src/traits/sig_aug.rs:12-17).  sks: 32 B little-endian each; outputs RAW_PROJ. */
int blsgpu_sign_batch(int sig_group, int scheme, const uint8_t* sks, const uint8_t* msgs, const uint64_t* msg_offsets,
                      size_t n, void* out_pks, void* out_sigs);

/* Threshold recovery: Signature::from_shares (src/signature.rs:151-165) and PublicKey::from_shares (src/public_key.rs:128-134) ->
 * core_combine_signature_shares / core_combine_public_key_shares (src/traits/sig_core.rs:92-105), for n_sets independent
 * recoveries in one call.  Each is Lagrange interpolation at zero, as the dependency (vsss-rs) does it:
 *     lambda_i = prod_{j != i} x_j / (x_j - x_i),   result = sum_i lambda_i P_i.
 * group: the group the points live in, 1 = G1, 2 = G2.  For Bls12381G2Impl signatures are group 2 and public keys group 1; for
 *     Bls12381G1Impl signatures are group 1 and public keys group 2.
 * set_offsets: n_sets + 1 entries, set s is shares set_offsets[s] .. set_offsets[s + 1]; it starts at 0 and never decreases
 *     (anything else: BLSGPU_E_ARG).  The total share count is set_offsets[n_sets].
 * ids: one 32-byte little-endian identifier per share (IdentifierPrimeField<Scalar>): full 255-bit values are handled.
 * pts: one point per share, BLSGPU_FMT_RAW_PROJ or BLSGPU_FMT_RAW_AFFINE (fmt); compressed input goes through blsgpu_deserialize
 *     first (device pointers chain).
 * schemes: NULL (PublicKey::from_shares: no scheme check) or one BLSGPU_SCHEME_* byte per share.
 * out: n_sets RAW_PROJ points with Z = 1, or all-zero bytes for the identity; a set whose status is not OK gets the identity.
 * status: one entry per set, the first of these that applies:
 *     BLSGPU_BAD_ENCODING   an identifier >= r (the reference type cannot hold it: deserialisation fails before from_shares)
 *     BLSGPU_INVALID_SCHEME the scheme tags differ within the set
 *     BLSGPU_VSSS_ERROR     fewer than two shares (an empty set included), a zero identifier, or two equal identifiers
 *     BLSGPU_OK
 * The reference maps every error of the dependency to the one VsssError, so which of its checks fires first is not observable.
 * Two assumptions of this library: at least two shares are required, and identity share values are accepted (they add
 * nothing).  Fewer shares than the threshold is not an error: it yields a different point, as in the reference.
 * Every pointer may be host or device memory; a device `out` feeds blsgpu_verify_batch without a host round trip. */
int blsgpu_combine_shares(int group, const uint8_t* ids, const void* pts, const uint8_t* schemes, const uint64_t* set_offsets,
                          size_t n_sets, int fmt, void* out, int32_t* status);

/* Batched verify_secure: Signature::verify_secure / verify_secure_with_mode (src/signature.rs:177-197,256-276 ->
 * src/secure_aggregation.rs:182-205,236-246) for n_sets independent (keys, signature, message) sets in one call.
 * key_offsets: n_sets + 1 entries; set s owns keys key_offsets[s] .. key_offsets[s + 1] of pks (it starts at 0 and never
 *     decreases; anything else is BLSGPU_E_ARG).  The total key count must be below 2^32.
 * sigs: one signature per set.  msgs / msg_offsets: one message per set (msg_offsets: n_sets + 1 entries).
 * scheme, ser_format and fmt apply to every set and take the same values as in blsgpu_verify_secure (RAW_PROJ or RAW_AFFINE
 *     points; Legacy only for sig_group 2).  MessageAugmentation only switches the DST: no key prefix (:236-246).
 * status[s] equals what blsgpu_verify_secure returns for set s alone: an empty set is BLSGPU_OK iff its signature is the
 *     identity, else BLSGPU_INVALID_SIGNATURE (:189-195); a zero coefficient is BLSGPU_INVALID_COEFFICIENT (:97-100); otherwise
 *     the identity checks and the pairing check of core_verify (src/traits/sig_core.rs:126-140), in that order.
 * Sets below BLSGPU_SECURE_BATCH_MAX keys are sorted, hashed and summed together on the device; larger ones run one at a time
 *     through blsgpu_verify_secure's steps; every set shares one verification tail.  The knob changes the plan, never a status.
 * Every pointer may be host or device memory; a device `status` stays on the device.  The call runs on one device even when
 *     several are bound (whole sets are not sharded over devices). */
int blsgpu_verify_secure_batch(int sig_group, int scheme, const void* pks, const uint64_t* key_offsets, size_t n_sets,
                               const void* sigs, const uint8_t* msgs, const uint64_t* msg_offsets, int ser_format, int fmt,
                               int32_t* status);

/* Batched aggregate verify: AggregateSignature::verify (src/aggregate_signature.rs:230-239) for n_sets independent
 * (keys, messages, aggregate signature) sets in one call.
 * set_offsets: n_sets + 1 entries; set s owns pairs set_offsets[s] .. set_offsets[s + 1] of pks / msg_offsets (it starts at 0
 *     and never decreases; anything else is BLSGPU_E_ARG).  The total pair count T = set_offsets[n_sets] must be below 2^32.
 * msgs / msg_offsets: one message per pair (msg_offsets: T + 1 entries).  sigs: one aggregate signature per set.
 * fmt: BLSGPU_FMT_RAW_PROJ or BLSGPU_FMT_RAW_AFFINE points.  status: n_sets entries.  aux: NULL, or 2 n_sets entries.
 * status[s], aux[2 s], aux[2 s + 1] equal what blsgpu_aggregate_verify returns for set s alone, indices local to the set:
 *     Basic only: the first pair i whose message equals an earlier one OF THE SAME SET is BLSGPU_DUPLICATE_MESSAGE, aux =
 *     (earlier index, i), 0-based (src/traits/sig_basic.rs:46-58); then an identity signature is BLSGPU_SIG_IDENTITY, the
 *     first identity key BLSGPU_PK_IDENTITY with aux[2 s] = its 1-based index (src/traits/sig_core.rs:155-167); then the
 *     pairing product gives BLSGPU_OK or BLSGPU_INVALID_SIGNATURE.  aux is (0, 0) otherwise.  An empty set with a
 *     non-identity signature is BLSGPU_INVALID_SIGNATURE.
 * Sets below BLSGPU_AGG_BATCH_MAX pairs are hashed, paired, multiplied and exponentiated together on the device; larger ones
 *     run one at a time through blsgpu_aggregate_verify's kernels.  The knob changes the plan, never a status.
 * Every pointer may be host or device memory; a device `status` / `aux` stays on the device.  n_sets == 0 returns 0.  The
 *     call runs on one device even when several are bound (whole sets are not sharded over devices). */
int blsgpu_aggregate_verify_batch(int sig_group, int scheme, const void* pks, const uint8_t* msgs, const uint64_t* msg_offsets,
                                  const uint64_t* set_offsets, size_t n_sets, const void* sigs, int fmt, int32_t* status,
                                  uint64_t* aux);

/* Batched multi verify: MultiSignature::<C>::verify(MultiPublicKey::from_public_keys(pks), msg) (src/multi_signature.rs:127-135,
 * src/multi_public_key.rs:79-83 -> src/traits/pk_multi.rs:7-13) for n_sets independent (keys, signature, message) sets in one call.
 * key_offsets: n_sets + 1 entries; set s owns keys key_offsets[s] .. key_offsets[s + 1] of pks (it starts at 0 and never
 *     decreases; anything else is BLSGPU_E_ARG).  The total key count must be below 2^32.
 * sigs: one signature per set.  msgs / msg_offsets: one message per set (msg_offsets: n_sets + 1 entries).
 * fmt: BLSGPU_FMT_RAW_PROJ or BLSGPU_FMT_RAW_AFFINE points (anything else is BLSGPU_E_ARG); scheme and fmt apply to every set.
 *     Under MessageAugmentation the message of set s is prefixed with the compressed bytes of the set's summed key
 *     (src/traits/sig_aug.rs:20-24).
 * status[s] equals what blsgpu_multi_verify returns for set s alone, the order of core_verify (src/traits/sig_core.rs:126-140):
 *     BLSGPU_SIG_IDENTITY        the signature is the identity
 *     BLSGPU_PK_IDENTITY         the summed key is the identity: an empty set, or keys that cancel (P, -P); an identity key
 *                                inside a set adds nothing
 *     BLSGPU_INVALID_SIGNATURE   the pairing check fails
 *     BLSGPU_OK
 * The keys are summed by one segmented point sum over all sets (strips of BLSGPU_MULTI_STRIP keys, by default as many strips as
 *     a single sum over all keys has lanes); every set shares one verification tail.  The knob changes the plan, never a status.
 * Every pointer may be host or device memory; a device `status` stays on the device.  key_offsets (and msg_offsets) are read
 *     and checked on the host.  n_sets == 0 returns 0.  n_sets == 1 is blsgpu_multi_verify itself, its split over the bound
 *     devices included; in every other case the call runs on one device even when several are bound (whole sets are not sharded
 *     over devices). */
int blsgpu_multi_verify_batch(int sig_group, int scheme, const void* pks, const uint64_t* key_offsets, size_t n_sets,
                              const void* sigs, const uint8_t* msgs, const uint64_t* msg_offsets, int fmt, int32_t* status);

/* ---- threshold signcryption: the decryption-share side of SignCryptCiphertext (src/sign_crypt_ciphertext.rs,
 * src/sign_decryption_share.rs, src/traits/sign_crypt.rs:101-150,192-207).  Only public data enters: ciphertexts, public-key
 * shares and decryption shares.  "pk group": the group of public keys (u, the decryption shares, the public-key shares);
 * "sig group": where w lives.  The n_ct ciphertexts are given as in the validity call above: us, ws, and the v fields concatenated in
 * vs with n_ct + 1 entries in v_offsets.  Offsets start at 0 and never decrease (anything else: BLSGPU_E_ARG); they are read and
 * checked on the host.  fmt: BLSGPU_FMT_RAW_PROJ or BLSGPU_FMT_RAW_AFFINE for every point.  Every pointer may be host or device
 * memory.  Both calls run on one device.
 *
 * Batched BlsSignCrypt::verify_share (sign_crypt.rs:192-207) for every share of every ciphertext:
 * shares / pk_shares: one decryption share and the matching public-key share per entry (pk group), share_offsets[c] ..
 *     share_offsets[c + 1] belong to ciphertext c (n_ct + 1 entries); the total must be below 2^32.
 * status: one entry per share: BLSGPU_OK, or BLSGPU_INVALID_DECRYPTION_SHARE for every way the reference's Choice is 0: an identity
 *     share, an identity public-key share, an identity w, or a pairing product e(-W', share) e(w, pk) that is not one.  As in the
 *     reference, u is not checked for the identity here and the ciphertext's own validity plays no part.
 * W' = H(u.to_bytes() || v) under the DST of `scheme` is computed once per ciphertext, on the device; every share of that
 *     ciphertext pairs against it.  SignDecryptionShare::verify always passes the Basic DST, whatever the ciphertext's scheme is
 *     (sign_decryption_share.rs:54): a caller that mirrors it passes BLSGPU_SCHEME_BASIC. */
int blsgpu_signcrypt_share_verify_batch(int sig_group, int scheme, const void* us, const void* ws, const uint8_t* vs,
                                        const uint64_t* v_offsets, size_t n_ct, const void* shares, const void* pk_shares,
                                        const uint64_t* share_offsets, int fmt, int32_t* status);

/* The same with share i's public-key share at position idx[i] of a registered key set (blsgpu_keyset_create; a committee's key shares
 * are fixed for hours while its members' decryption shares arrive per ciphertext).  idx has share_offsets[n_ct] entries; the sig group is
 * the set's; fmt describes us, ws and shares.  BLSGPU_E_ARG with no status written: an unknown handle, offsets that decrease or do not
 * start at 0, a null required argument, 2^32 or more shares.  No shares: 0.  The call runs on the key set's device and does not shard.
 * status[i], every share its own set, the first that applies: BLSGPU_E_ARG in the slot for a position outside the table (nothing
 * outside the table is read); the entry's creation status for an invalid entry; otherwise exactly what the by-value call gives for that
 * share with the gathered key (the identity entry is a valid entry: BLSGPU_INVALID_DECRYPTION_SHARE).  Repeated indices are repeated keys.
 * Above BLSGPU_WIDE_MAX shares the call reads line rows where that saves a walk and never where it changes a status: for
 * Bls12381G1Impl the key's rows of a set created with BLSGPU_KEYSET_LINES (only the share is walked); for Bls12381G2Impl the rows of
 * -W' and w, built once per ciphertext, when the call has at least BLSGPU_SIGNCRYPT_LINES_MIN shares per ciphertext on average
 * (a share then walks nothing; 0: never; unset: 64, the measured default). */
int blsgpu_signcrypt_share_verify_indexed_batch(int scheme, uint64_t keyset, const uint32_t* idx, const void* us, const void* ws,
                                                const uint8_t* vs, const uint64_t* v_offsets, size_t n_ct, const void* shares,
                                                const uint64_t* share_offsets, int fmt, int32_t* status);

/* Batched BlsSignCrypt::unseal_with_shares = SignCryptCiphertext::decrypt_with_shares (sign_crypt.rs:106-119,
 * sign_crypt_ciphertext.rs:60-72):
 * ids / shares / share_offsets: the decryption shares of all ciphertexts, flat, with their 32-byte little-endian identifiers.
 * frames: as large as vs, same offsets: SHAKE128(G.to_bytes()) xor v per ciphertext (G.to_bytes(): 48 bytes for Bls12381G2Impl, 96
 *     for Bls12381G1Impl; the identity is c0 00 ..).  pt_range: two uint64 per ciphertext, the offset of the plaintext inside its
 *     frame and its length.  status: one entry per ciphertext.
 * Per ciphertext, in the reference's order:
 *   1. fewer than two shares (an empty set included): BLSGPU_VSSS_ERROR (CtOption::new(vec![], 0), :114-116), pt_range (0, 0);
 *   2. G = sum lambda_i share_i over ALL shares passed (the shares are not verified here), by the machinery of the share-recovery
 *      call above, its ladder and MSM plans included; a set that machinery rejects (a zero or duplicate identifier, an identifier
 *      >= r) yields the identity point and goes on (combine().unwrap_or_default(), :117);
 *   3. valid = BlsSignCrypt::valid, the verdict of the validity call above;
 *   4. frame = SHAKE128(G.to_bytes()) xor v;
 *   5. the frame is parsed as varint(len) || message || padding (:122-136); on success pt_range = (overhead, len).
 * status, the first that applies: BLSGPU_VSSS_ERROR (1.); the validity check's status when it is not OK (BLSGPU_INVALID_SIGNATURE,
 *     BLSGPU_SIG_IDENTITY for w, BLSGPU_PK_IDENTITY for u); BLSGPU_BAD_FRAME when the parse fails; BLSGPU_OK.  status == BLSGPU_OK
 *     <=> is_some().  The frame bytes and pt_range of an item that is not OK are not part of the contract (pt_range is (0, 0)).  As
 *     in the reference, a valid ciphertext opened with wrong or too few shares can still parse and return BLSGPU_OK with garbage.
 * A third assumption of this library, beside the two of the share-recovery call: the varint is the unsigned encoding of the
 *     uint-zigzag crate -- seven value bits per byte, least significant group first, the top bit set on every byte but the last;
 *     `peek` looks at up to 19 bytes (the longest encoding of a u128) and fails if none of them terminates or the frame ends
 *     first; the value is taken modulo 2^64 (`as usize`); the parse succeeds iff len <= frame_len - overhead.  One function holds
 *     the rule (csrc/signcrypt.cuh signcrypt_parse_frame).
 * Keys in place of shares (SignCryptDecryptionKey::decrypt, sign_crypt_ciphertext.rs:157-163): ids == NULL and share_offsets == NULL
 *     means `shares` holds exactly one pk-group point per ciphertext, used as G; step 1 does not apply. */
int blsgpu_signcrypt_open_batch(int sig_group, int scheme, const void* us, const void* ws, const uint8_t* vs,
                                const uint64_t* v_offsets, size_t n_ct, const uint8_t* ids, const void* shares,
                                const uint64_t* share_offsets, int fmt, uint8_t* frames, uint64_t* pt_range, int32_t* status);

/* ---- ElGamal over the public-key group (src/traits/elgamal.rs): the checks that need no secret key.  Points are in the KEY group
 * of sig_group (G2 for Bls12381G1Impl = 1, G1 for Bls12381G2Impl = 2); scalars are 32 bytes little-endian.
 *
 * BlsElGamal::message_generator() (elgamal.rs:20-23): the hash-to-curve of the compressed generator of the key group under ENC_DST
 * (src/impls/g1.rs:129, g2.rs:127; the tag names the other group than the one it hashes into, as in the reference).  Computed once
 * per process and cached.  fmt_out: any of the four formats; out: one point, host or device memory. */
int blsgpu_elgamal_message_generator(int sig_group, int fmt_out, void* out);

/* Batched BlsElGamal::verify_proof (elgamal.rs:177-226) = ElGamalProof::verify (src/elgamal_proof.rs:74-84): n independent proofs.
 * pks: n_pks points, n_pks == n (a key per proof) or 1 (every proof is to the same recipient); anything else is BLSGPU_E_ARG.
 * generators: NULL (the message generator, what ElGamalProof::verify passes) or n points (the trait's Some(generator)).
 * c1s, c2s: n points each.  message_proofs, blinder_proofs, challenges: n scalars each.  fmt: any of the four point formats, the
 *     same for every point of the call.  Every pointer may be host or device memory.  n == 0 returns 0 and touches nothing.
 * status[i], the first that applies:
 *     BLSGPU_BAD_ENCODING        a point does not decode (wire formats; BLSGPU_LEGACY_FORMAT where the decoder says so), or a scalar
 *                                is >= r: no reference value can hold it, deserialisation fails before verify_proof runs;
 *     BLSGPU_ELGAMAL_IDENTITY    pk, generator, c1 or c2 is the identity;
 *     BLSGPU_ELGAMAL_ZERO_PROOF  one of the three scalars is zero;
 *     BLSGPU_CHALLENGE_MISMATCH  the challenge recomputed from r1 = (-c) c1 + bp G, r2 = (-c) c2 + mp H + bp pk differs;
 *     BLSGPU_OK                  the proof verifies.
 * Two assumptions of this library, neither pinned by a vector of the crates themselves: Merlin's STROBE runs
 *     the permutation whenever an absorb or squeeze fills the 166-byte block (STROBE v1.0.2), and Scalar::from_bytes_wide reads its
 *     64 bytes as one little-endian integer. */
int blsgpu_elgamal_proof_verify_batch(int sig_group, const void* pks, size_t n_pks, const void* generators, const void* c1s,
                                      const void* c2s, const uint8_t* message_proofs, const uint8_t* blinder_proofs,
                                      const uint8_t* challenges, size_t n, int fmt, int32_t* status);

/* Batched ElGamalDecryptionKey::from_shares + decrypt (src/elgamal_decryption_share.rs:76-90) for n_ct ciphertexts.
 * c2s: the second component of every ciphertext.  ids / shares / share_offsets: the decryption shares of all ciphertexts, flat, as
 *     in blsgpu_signcrypt_open_batch; the key of ciphertext s is what blsgpu_combine_shares gives for its set (the same stages).
 * fmt: BLSGPU_FMT_RAW_PROJ or BLSGPU_FMT_RAW_AFFINE.  out: n_ct RAW_PROJ records, c2 - key; status: n_ct entries, the status of
 *     blsgpu_combine_shares for the set (BLSGPU_BAD_ENCODING, BLSGPU_VSSS_ERROR or BLSGPU_OK).  out[s] is the identity (all-zero
 *     bytes) when status[s] is not BLSGPU_OK.
 * Keys in place of shares (ElGamalDecryptionKey::decrypt): ids == NULL and share_offsets == NULL means `shares` holds one ready key
 *     per ciphertext; every status is BLSGPU_OK.
 * Every pointer may be host or device memory; a device `out` stays there.  n_ct == 0 returns 0.
 * The sum of ciphertexts (src/elgamal_ciphertext.rs:74-83) is blsgpu_sum_batch over the c1s and over the c2s. */
int blsgpu_elgamal_open_batch(int sig_group, const void* c2s, const uint8_t* ids, const void* shares, const uint64_t* share_offsets,
                              size_t n_ct, int fmt, void* out, int32_t* status);

/* ---- batched aggregation: the objects the batched verifiers above consume, made for many sets in one call.
 *
 * Batched secure aggregation: aggregate_secure / aggregate_secure_with_mode = AggregateSignature::from_signatures_secure
 * (src/secure_aggregation.rs:110-169,338-352, src/aggregate_signature.rs:191-227) for n_sets independent (keys, signatures) sets.
 * key_offsets: n_sets + 1 entries; set s owns keys AND signatures key_offsets[s] .. key_offsets[s + 1] of pks / sigs, one signature
 *     per key at the same index (it starts at 0 and never decreases; anything else is BLSGPU_E_ARG).  The total must be below 2^32.
 * ser_format and fmt apply to every set and take the same values as in blsgpu_aggregate_secure (RAW_PROJ or RAW_AFFINE points;
 *     Legacy only for sig_group 2).
 * out_sigs: n_sets RAW_PROJ records of the signature group; status: n_sets entries, BLSGPU_OK or BLSGPU_INVALID_COEFFICIENT.
 * out_sigs[s] and status[s] are what blsgpu_aggregate_secure returns for set s alone: sum_p t_p sig[idx_p] over the sorted
 *     positions p of the set's keys, where idx_p is the FIRST input position of the set whose serialised key equals the p-th sorted
 *     key (the reference's `position` search, :138-147), so duplicate keys all pick the first copy's signature.  An empty set gives
 *     the identity and BLSGPU_OK.  Where status[s] is BLSGPU_INVALID_COEFFICIENT (:97-100) the record is all-zero.  The point
 *     is the same group element as the single call's; its projective representative need not be.
 * Sets below BLSGPU_SECURE_BATCH_MAX keys are sorted, hashed and summed together on the device; larger ones run one at a time
 *     through blsgpu_aggregate_secure's steps, and one large set alone is that call.  The knob changes the plan, never a result.
 * Every pointer may be host or device memory; a device out_sigs feeds blsgpu_verify_secure_batch without a host round trip.
 *     key_offsets are read and checked on the host.  n_sets == 0 returns 0.  The call runs on one device. */
int blsgpu_aggregate_secure_batch(int sig_group, const void* pks, const void* sigs, const uint64_t* key_offsets, size_t n_sets,
                                  int ser_format, int fmt, void* out_sigs, int32_t* status);

/* Batched plain sums: the point sum of MultiSignature::from_signatures and AggregateSignature::from_signatures
 * (src/multi_signature.rs:80-107,147, src/aggregate_signature.rs:123-148,171) and of MultiPublicKey::from_public_keys
 * (src/multi_public_key.rs:79-83) for n_sets independent sets; the scheme rules of those constructors are the caller's.
 * group: 1 (G1) or 2 (G2).  offsets: n_sets + 1 entries; set s owns points offsets[s] .. offsets[s + 1] of pts (it starts at 0 and
 *     never decreases; anything else is BLSGPU_E_ARG).  The total must be below 2^32.  fmt: RAW_PROJ or RAW_AFFINE.
 * out: n_sets RAW_PROJ records; out[s] is the sum of set s, the identity (all-zero) for an empty set.
 * One segmented point sum over all sets, the one of blsgpu_multi_verify_batch (strips of BLSGPU_MULTI_STRIP points); a single
 *     set is a plan with one set and stays on one device.
 * Every pointer may be host or device memory; a device `out` feeds the batched verifiers directly.  n_sets == 0 returns 0. */
int blsgpu_sum_batch(int group, const void* pts, const uint64_t* offsets, size_t n_sets, int fmt, void* out);

/* ---- Registered key sets: a long-lived table of public keys on the device; a set of signers is a list of positions in it.
 * The callers this serves keep a masternode list or a validator registry for hours and name signers as bitsets over it: they
 * deserialise and upload every key ONCE (blsgpu_keyset_create) and afterwards pass 4 bytes per (set, key).
 *
 * A handle is an opaque non-zero id from a registry inside the library, never a pointer; every entry point given a stale or
 * unknown id returns BLSGPU_E_ARG.  Concurrent calls may read one set.  A set changes only through blsgpu_keyset_update and
 * blsgpu_keyset_append, and those take no lock against its readers: running any call on a set while another thread updates,
 * appends to or destroys the same set is the caller's error (the call may then read half-written entries or freed device memory).
 * blsgpu_shutdown frees every key set.  The memory
 * is hipMalloc'd outside the context arenas on the device of the context that ran blsgpu_keyset_create (device 0 of a
 * multi-device binding unless the call came from a sharded sub-call); the indexed entry points run on that device and do not
 * shard.
 *
 * create: `keys` (host or device) holds n keys of the group the signatures of sig_group do NOT live in, in any BLSGPU_FMT_*
 * (LEGACY for sig_group 2 only).  Wire formats go through the checked decompression of blsgpu_deserialize and status[i] (n
 * entries, host or device, may be NULL) is what that call gives for key i; raw formats are trusted as everywhere else and give
 * BLSGPU_OK.  A key whose status is not BLSGPU_OK is kept as an INVALID ENTRY and creation still succeeds; the identity is a valid
 * entry.  Nothing of the caller's buffers is retained.  flags & BLSGPU_KEYSET_TABLES also builds the fixed-base tables (about
 * 29 KB per key) that turn a scalar multiplication of an entry into about 64 mixed additions and no doubling; when they would
 * exceed BLSGPU_KEYSET_TABLE_MB MiB (default 4096) or the device has no room, the set is created without them and `has_tables`
 * reports 0.  Tables never change a result.
 * flags & BLSGPU_KEYSET_LINES (Bls12381G1Impl, keys in G2; accepted and without effect for sig_group 2, whose keys have no lines)
 * also derives every key's 68 normalised Miller-loop rows (15,232 bytes per key; the reference's G2Prepared::from(pk), kept instead
 * of recomputed per call): blsgpu_verify_indexed_batch and blsgpu_verify_shared_indexed_batch above BLSGPU_WIDE_MAX items -- the
 * one-wave path up to BLSGPU_COOP_MAX items (k_pairing_coop_keyed) and the lane-split path beyond (k_lines2s_keyed) -- then read
 * rows where they walked the key, under every scheme; calls of at most BLSGPU_WIDE_MAX items run on the row-wide engine, which
 * derives the key's lines beside the hash and does not read the rows.  So do the batched sets of
 * blsgpu_aggregate_verify_indexed_batch (whatever their number), whose signature items read the constant rows of -[c] g2 as
 * well.  The lines are not built, and the set works
 * without them, when they would not stay below 2^32 bytes (more than 281,970 keys), when together with the fixed-base tables they
 * would exceed BLSGPU_KEYSET_TABLE_MB MiB, or when the device has no room.  A call that names a finite entry whose rows are
 * unusable (no key of order r; raw input only) walks the keys of all its items.  Line tables never change a status.
 * info: *has_tables is the mask of what was built -- bit 0 (BLSGPU_KEYSET_TABLES) the fixed-base tables, bit 1 (BLSGPU_KEYSET_LINES)
 * the line tables -- so a caller that created the set with flags 0 or 1 reads the 0 or 1 it read before; device_bytes counts both.
 * get: entries idx[0 .. count) in any format, with their creation statuses (status may be NULL); an invalid entry leaves as the
 * identity.  mul: out[i] = scalars[i] * key[idx[i]] as RAW_PROJ (scalars: 32 bytes little-endian each, any value below 2^256,
 * reduced modulo r as blsgpu_msm_* does); the identity and invalid entries give the identity (Z = 0).  Both return BLSGPU_E_ARG when an index is not below the set's size. */
#define BLSGPU_KEYSET_TABLES 1
#define BLSGPU_KEYSET_LINES 2
int blsgpu_keyset_create(int sig_group, const void* keys, size_t n, int fmt, int flags, int32_t* status, uint64_t* out_handle);
int blsgpu_keyset_destroy(uint64_t handle);
int blsgpu_keyset_info(uint64_t handle, int* sig_group, uint64_t* n, int* has_tables, uint64_t* device_bytes);
int blsgpu_keyset_get(uint64_t handle, const uint32_t* idx, size_t count, int fmt_out, void* out, int32_t* status);
int blsgpu_keyset_mul(uint64_t handle, const uint32_t* idx, const uint8_t* scalars, size_t count, void* out);

/* A registered list changes -- a masternode list by a handful of entries every block, a validator registry by growth every epoch
 * -- and the set follows in place.  After either call the set is what blsgpu_keyset_create with the same flags gives for the
 * final key list, through every call above and below: records, Modern bytes, creation statuses, fixed-base tables, line rows.
 *
 * update: entry pos[i] becomes keys[i] (count keys; `keys`, `fmt` and `status` exactly as at creation: any BLSGPU_FMT_*, LEGACY for
 * sig_group 2 only, wire formats through the checked decompression, status[i] -- may be NULL -- what deserialisation gives for
 * key i, a key that fails kept as an invalid entry, raw formats trusted).  pos, keys and status may be host or device memory; pos
 * is read and checked on the host (copied down first when it lives on the device).  A position not below the set's size, the same
 * position twice in one call, an unknown handle, a null pos or keys with count > 0 and a bad format return BLSGPU_E_ARG with
 * nothing written to the set and no status written.  count == 0 returns 0.  For every named entry the call rewrites all the set
 * has of it, so an entry may gain or lose its table and its line rows (a real key in the place of the identity, and the reverse);
 * no other entry changes.  The work is that of creation on the named entries alone, in chunks of 4,096 keys.
 *
 * append: the set grows from n to n + count entries (fewer than 2^32 - 1, as at creation; more is BLSGPU_E_ARG), *out_first
 * (may be NULL) receives n, and the new entries are keys[0 .. count) as for update.  The arrays are reallocated and copied on
 * the device, each new array allocated before the old one is freed; when the device has no room for the grown records the call
 * returns BLSGPU_E_HIP and the set is unchanged.  Tables and lines follow the creation rule on the final size: where the grown
 * tables or lines would exceed BLSGPU_KEYSET_TABLE_MB MiB, break the 2^32-byte bound of the lines or find no room on the device,
 * they are dropped, the set works without them, blsgpu_keyset_info reports the new mask, and no status of any later call changes.
 * A set created empty gets the tables and lines it was created for with its first keys.  device_bytes afterwards is what
 * creation of the final list reports.
 * Both run on the key set's device. */
int blsgpu_keyset_update(uint64_t handle, const uint32_t* pos, const void* keys, size_t count, int fmt, int32_t* status);
int blsgpu_keyset_append(uint64_t handle, const void* keys, size_t count, int fmt, int32_t* status, uint64_t* out_first);

/* The batched entry points with (keyset, idx) in place of the keys: blsgpu_multi_verify_batch, blsgpu_verify_secure_batch,
 * blsgpu_sum_batch, blsgpu_verify_batch (one key per item) and blsgpu_aggregate_verify_batch over positions in a key set.  sig_group comes from the key set and
 * fmt (RAW_PROJ / RAW_AFFINE) describes the signatures only; idx, the offsets, sigs, msgs and status may be host or device memory.
 * status[s] is the first of: BLSGPU_E_ARG (-3, in the status slot; the call still returns 0 and the other sets are unaffected)
 * when the set names an index that is not below the key set's size -- nothing outside the table is read; the creation status of
 * the first invalid entry the set names, in input order (the reference fails at deserialisation, before any verify); otherwise
 * exactly what the non-indexed entry point returns for the gathered keys (repeated indices are repeated keys, the empty-set
 * rules are unchanged).  blsgpu_sum_indexed_batch has no status vector: an index outside the table makes the call return
 * BLSGPU_E_ARG, invalid entries add nothing, as identities do. */
int blsgpu_multi_verify_indexed_batch(int scheme, uint64_t keyset, const uint32_t* idx, const uint64_t* key_offsets, size_t n_sets,
                                      const void* sigs, const uint8_t* msgs, const uint64_t* msg_offsets, int fmt, int32_t* status);
int blsgpu_verify_secure_indexed_batch(int scheme, uint64_t keyset, const uint32_t* idx, const uint64_t* key_offsets, size_t n_sets,
                                       const void* sigs, const uint8_t* msgs, const uint64_t* msg_offsets, int ser_format, int fmt, int32_t* status);
int blsgpu_sum_indexed_batch(uint64_t keyset, const uint32_t* idx, const uint64_t* offsets, size_t n_sets, void* out /* RAW_PROJ */);
int blsgpu_verify_indexed_batch(int scheme, uint64_t keyset, const uint32_t* idx, const void* sigs, const uint8_t* msgs,
                                const uint64_t* msg_offsets, size_t n, int fmt, int32_t* status);
/* blsgpu_aggregate_verify_batch with pair i's key at position idx[i] of the key set (idx has set_offsets[n_sets] = T entries):
 * AggregateSignature::verify, many keys with one message each, over a registered key set.  sig_group comes from the key set and
 * fmt (RAW_PROJ / RAW_AFFINE) describes the signatures only; set_offsets, msg_offsets (T + 1 entries), msgs, aux (NULL or
 * 2 n_sets entries) and the T < 2^32 rule are the by-value entry point's.  Every pointer may be host or device memory; a device
 * status / aux stays on the device.  n_sets == 0 returns 0.  An unknown or destroyed handle, offsets that decrease or do not
 * start at 0, and a null required argument are BLSGPU_E_ARG, and no status is written.  The call runs on the key set's device,
 * without sharding.
 * status[s] is the first of: BLSGPU_E_ARG in the slot when the set names an index that is not below the key set's size (nothing
 * outside the table is read); the creation status of the first invalid entry the set names, in input order; otherwise exactly
 * what blsgpu_aggregate_verify_batch returns for the gathered keys -- Basic's duplicate-message rule per set, the identity
 * signature, the first identity key with its 1-based index in aux, the pairing product, the empty-set rules.  The identity is a
 * valid entry (BLSGPU_PK_IDENTITY as by value), repeated indices are repeated keys, and a set decided by one of the first two rules
 * gets aux (0, 0); its neighbours never see it.  Sets below BLSGPU_AGG_BATCH_MAX pairs are batched, larger ones run one at a time
 * on the gathered keys, as by value.  Over a set with line tables (BLSGPU_KEYSET_LINES, Bls12381G1Impl) no item of the batched
 * sets walks a G2 point; a call that names a finite entry without usable rows walks all its items.  Line tables never change
 * a status or an aux value. */
int blsgpu_aggregate_verify_indexed_batch(int scheme, uint64_t keyset, const uint32_t* idx, const uint8_t* msgs, const uint64_t* msg_offsets,
                                          const uint64_t* set_offsets, size_t n_sets, const void* sigs, int fmt, int32_t* status, uint64_t* aux);

/* ---- Shared-message verify: Signature::verify (src/signature.rs:130-138) for items that come in GROUPS under one message each --
 * the signature shares of a signing session checked one by one against the members' key shares (PublicKeyShare::verify,
 * src/public_key_share.rs:55-72), or unaggregated attestations: a handful of messages, many (key, signature) items, one verdict
 * per item.
 * Group g owns items item_offsets[g] .. item_offsets[g + 1] of pks / sigs, and message g = msgs[msg_offsets[g] .. msg_offsets[g + 1]).
 *     Both offset arrays have n_groups + 1 entries, start at 0 and never decrease (anything else is BLSGPU_E_ARG, and no status
 *     is written); they are read and checked on the host.  A group may be empty.  The item count must be below 2^32.
 * fmt: RAW_PROJ or RAW_AFFINE.  status: one entry per ITEM, exactly what blsgpu_verify_batch returns for the item with its
 *     group's message (signature identity, then key identity, then the pairing: src/traits/sig_core.rs:126-145).
 * Basic and ProofOfPossession hash every message ONCE and make the point affine once per group; an item costs its identity checks,
 *     one inversion and the two-pair pairing.  For Bls12381G2Impl on the lane-split path (more than BLSGPU_COOP_MAX items) with
 *     at least BLSGPU_SHARED_LINES_MIN items per group on average (0: never; unset: 4, and only in batches of at least 98,304
 *     items, where the form was measured to pay) and line tables (15,232 bytes per group) below 4 GiB, H(m)'s 68 Miller-loop
 *     lines are derived once per group as well and an item walks one G2 point instead of two.  The knob changes the plan, never
 *     a status.  Under MessageAugmentation every item hashes pk_i || m: nothing is
 *     shared, the messages are copied out per item on the device and the items run as blsgpu_verify_batch runs them.
 * Every pointer may be host or device memory; a device status stays on the device.  n_groups == 0 or no items returns 0.  The
 *     call runs on one device. */
int blsgpu_verify_shared_batch(int sig_group, int scheme, const void* pks, const void* sigs, const uint64_t* item_offsets, size_t n_groups,
                               const uint8_t* msgs, const uint64_t* msg_offsets, int fmt, int32_t* status);
/* The same with item i's key at position idx[i] of a registered key set; sig_group comes from the key set, fmt describes the
 * signatures, and status[i] follows the precedence of the other indexed calls with every item its own set: BLSGPU_E_ARG for a
 * position outside the table, then the entry's creation status, then what blsgpu_verify_shared_batch gives. */
int blsgpu_verify_shared_indexed_batch(int scheme, uint64_t keyset, const uint32_t* idx, const void* sigs, const uint64_t* item_offsets,
                                       size_t n_groups, const uint8_t* msgs, const uint64_t* msg_offsets, int fmt, int32_t* status);

/* ---- Registered message sets: the messages of blsgpu_verify_shared_batch hashed ONCE and kept on the device.  The shares of a
 * signing session or the attestations of a slot arrive over many calls; each of them would hash the same message again
 * (hash-to-G2 is more than half of one Bls12381G2Impl verification).  A set keeps per message what a shared-message call computes
 * per group before its items start -- the hash-to-curve point under the scheme's DST as an affine record (Bls12381G1Impl: before
 * the cofactor clearing; Bls12381G2Impl: cleared), 96 or 192 bytes -- and later calls name a group's message by its position.
 *
 * Handles follow the key sets' rules: an opaque non-zero id, never a pointer; a stale or unknown id (a key set's included) returns
 * BLSGPU_E_ARG; hipMalloc'd outside the context arenas on the device of the context that ran the creation, freed by
 * blsgpu_msgset_destroy or blsgpu_shutdown; update and append take no lock against readers (running any call on a set while another
 * thread updates, appends to or destroys it is the caller's error).
 *
 * create: msgs / msg_offsets (n + 1 entries from 0, never decreasing) as everywhere; empty messages and n == 0 are valid; scheme is
 *   Basic or ProofOfPossession -- MessageAugmentation hashes pk || m, so there is nothing to register: BLSGPU_E_ARG.  Nothing of the
 *   caller's buffers is retained.  flags & BLSGPU_MSGSET_LINES (Bls12381G2Impl; accepted and without effect for sig_group 1, whose
 *   messages are G1 points and have no lines): every entry also gets the 68 normalised Miller rows of its point, 15,232 bytes, so
 *   that a verification above BLSGPU_WIDE_MAX items walks the signature alone (k_pairing_coop_rows up to BLSGPU_COOP_MAX items, the
 *   table form of the line kernel beyond).  The rows are not built, and the set works without them, when they would reach 2^32 bytes
 *   (281,970 entries), exceed BLSGPU_KEYSET_TABLE_MB MiB, or find no room on the device.  An entry whose point is the identity or
 *   whose walk meets a vanishing denominator (neither happens for a hash output) keeps its point and has no usable rows: a call that
 *   names it walks all its items.  Rows change the plan, never a status.
 * info: *has_lines is 1 when the set has rows.
 * update: entry pos[i] becomes the hash of message i; a position outside the set or named twice is BLSGPU_E_ARG and nothing is
 *   written.  append: the set grows by `count` messages, *out_first (may be null) gets the first new position; when the device has
 *   no room for the grown records the set is unchanged.  Both hash and build the touched entries only; afterwards the set is what
 *   creation of the final message list gives (rows the grown set has no room for are dropped, rows the creator asked for and an
 *   empty set could not have are built).  pos, msgs and msg_offsets may be host or device memory. */
#define BLSGPU_MSGSET_LINES 1
int blsgpu_msgset_create(int sig_group, int scheme, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, int flags, uint64_t* out_handle);
int blsgpu_msgset_destroy(uint64_t handle);
int blsgpu_msgset_info(uint64_t handle, int* sig_group, int* scheme, uint64_t* n, int* has_lines, uint64_t* device_bytes);
int blsgpu_msgset_update(uint64_t handle, const uint32_t* pos, const uint8_t* msgs, const uint64_t* msg_offsets, size_t count);
int blsgpu_msgset_append(uint64_t handle, const uint8_t* msgs, const uint64_t* msg_offsets, size_t count, uint64_t* out_first);
/* blsgpu_verify_shared_batch with group g's message named as entry msg_idx[g] of a message set: the group structure, item_offsets,
 * pks, sigs, fmt and status are that call's (empty groups allowed; two groups may name one entry); sig_group and scheme come from the
 * set.  status[i] is, first, BLSGPU_E_ARG in the slot when the item's group names an index outside the set (other groups are
 * unaffected and the call returns 0); else exactly what blsgpu_verify_shared_batch returns for the item under the entry's message
 * bytes.  No call hashes anything.  Every pointer may be host or device memory; the call runs on the set's device. */
int blsgpu_verify_msgset_batch(uint64_t msgset, const uint32_t* msg_idx, const void* pks, const void* sigs, const uint64_t* item_offsets, size_t n_groups,
                               int fmt, int32_t* status);
/* The same with item i's key at position idx[i] of a registered key set of the same orientation on the same device (anything else:
 * BLSGPU_E_ARG).  status[i]: the message index rule above first, then the key set's two rules in their order (a position outside the
 * table, the entry's creation status), then the verification.  Over a Bls12381G1Impl key set with line tables an item above
 * BLSGPU_WIDE_MAX items needs nothing but its signature. */
int blsgpu_verify_msgset_indexed_batch(uint64_t msgset, const uint32_t* msg_idx, uint64_t keyset, const uint32_t* idx, const void* sigs,
                                       const uint64_t* item_offsets, size_t n_groups, int fmt, int32_t* status);
/* blsgpu_aggregate_verify_batch with pair i's message named as entry msg_idx[i] of a message set (msg_idx has set_offsets[n_sets] =
 * T entries): AggregateSignature::verify over registered messages.  sig_group and scheme (Basic or ProofOfPossession) come from the
 * set; pks, set_offsets, sigs, fmt, status, aux (NULL or 2 n_sets entries) and the T < 2^32 rule are the by-value entry point's.
 * Every pointer may be host or device memory; a device status / aux stays on the device.  set_offsets is read and checked on the
 * host, msg_idx on the device.  n_sets == 0 returns 0.  An unknown or destroyed handle, offsets that decrease or do not start at
 * 0, and a null required argument are BLSGPU_E_ARG, and nothing is written.  The call runs on the message set's device.
 * By bilinearity the pairs of a set that name one message are ONE factor e(sum of their keys, H(m)): the call forms one Miller
 * value per (set, message) class and one per signature, sums the keys of a class with the complete additions of the batched multi
 * verify (the same key twice is a doubling; P and -P give the identity, whose factor is 1 -- not an error), and hashes nothing.
 * status[s] / aux[2 s ..] is the first of: BLSGPU_E_ARG in the slot, aux (0, 0), when the set names a message index outside the
 * message set (nothing outside the table is read, other sets are unaffected, the call returns 0); otherwise exactly what
 * blsgpu_aggregate_verify_batch returns for those keys under the entries' message bytes -- Basic's duplicate rule with aux
 * (earlier, i), the identity signature, the first identity key with its 1-based index in INPUT order, the pairing product, the
 * empty-set rules.  All of these are decided on the pairs before anything is merged.
 * The duplicate rule without message bytes: a message set keeps no bytes, so under Basic two pairs of one set have "the same
 * message" when their entries hold equal affine hash records -- the same position named twice, or two positions created from
 * equal bytes.  The one assumption: unequal bytes never give equal records (that would be a hash-to-curve collision).  Under
 * ProofOfPossession classes go by position; two positions of equal bytes may stay two classes, the product is the same.
 * Every set runs through the segmented kernels whatever its size: BLSGPU_AGG_BATCH_MAX does not apply, because there are no
 * message bytes to hand to the single call's path.  With BLSGPU_MSGSET_LINES (Bls12381G2Impl) the class items take both lines of
 * every step from the entries' rows and only the n_sets signature items walk a G2 point; a call that names an entry without usable
 * rows walks all its items.  Rows change the plan, never a status or an aux value. */
int blsgpu_aggregate_verify_msgset_batch(uint64_t msgset, const uint32_t* msg_idx, const void* pks, const uint64_t* set_offsets, size_t n_sets,
                                         const void* sigs, int fmt, int32_t* status, uint64_t* aux);
/* The same with pair i's key at position idx[i] of a registered key set of the same orientation on the same device (anything else:
 * BLSGPU_E_ARG).  status[s]: the message index rule above first; then the key set's two rules in their order (a position outside
 * the table, then the creation status of the first invalid entry in input order; aux (0, 0)); then the verification.  Key set
 * line tables are not used by these entry points: a summed key has no table. */
int blsgpu_aggregate_verify_msgset_indexed_batch(uint64_t msgset, const uint32_t* msg_idx, uint64_t keyset, const uint32_t* idx,
                                                 const uint64_t* set_offsets, size_t n_sets, const void* sigs, int fmt, int32_t* status, uint64_t* aux);

/* ---- Registered signature sets: the third member beside key sets and message sets.  A time-lock service keeps a growing list of
 * round signatures; ciphertexts arrive for any of those rounds, in any order, over many calls.  blsgpu_timecrypt_open_batch makes
 * the caller sort them into groups, ship every signature again and have it decoded and subgroup-checked again, and under
 * Bls12381G2Impl walks the same G2 point through the 68 Miller entries once per ciphertext.  A set keeps per signature what that call
 * works out per group before its items start -- the point as a RAW_AFFINE record of its group (96 or 192 bytes, all-zero for the
 * identity), its scheme tag (0 / 1 / 2; any byte is kept as it comes and compared as the by-value call compares it) and its
 * creation status -- and later calls name an item's signature by its position.
 *
 * Handles follow the key sets' rules: an opaque non-zero id, never a pointer; a stale or unknown id (a key set's or a message set's
 * included) returns BLSGPU_E_ARG; hipMalloc'd outside the context arenas on the device of the context that ran the creation, freed
 * by blsgpu_sigset_destroy or blsgpu_shutdown; append takes no lock against readers (running any call on a set while another thread
 * appends to or destroys it is the caller's error).  There is no update: a published round signature does not change.
 *
 * create: n signatures of sig_group in format fmt (any of the four) with one scheme tag each; n == 0 is valid.  status (may be null)
 *   gets the n creation statuses: on COMPRESSED / LEGACY the decode status, subgroup test included (BLSGPU_OK, BLSGPU_BAD_ENCODING,
 *   BLSGPU_LEGACY_FORMAT); the raw formats are not subgroup-checked, as everywhere else, and every entry is BLSGPU_OK.  An identity
 *   signature is a valid entry with status BLSGPU_OK: the items that name it get BLSGPU_SIG_IDENTITY.  Nothing of the caller's
 *   buffers is retained.  flags & BLSGPU_SIGSET_LINES (Bls12381G2Impl; accepted and without effect for sig_group 1, whose signatures
 *   are G1 points and have no lines): every entry also gets the 68 normalised Miller rows of its point, 15,232 bytes, so that
 *   K = e(u, sig) evaluates the rows at u and walks nothing (k_pairing_value_rows).  The rows are not built, and the set works
 *   without them, when they would reach 2^32 bytes (281,970 entries), exceed BLSGPU_KEYSET_TABLE_MB MiB, or find no room on the
 *   device.  An entry that did not decode, is the identity, or whose walk meets a vanishing denominator has no usable rows: a call
 *   that names it walks all its items.  Rows change the plan, never a status or a byte.
 * info: *has_lines is 1 when the set has rows.
 * append: the set grows by `count` signatures, *out_first (may be null) gets the first new position, status (may be null) the new
 *   entries' creation statuses; when the device has no room for the grown records the set is unchanged.  Only the new entries are
 *   decoded and built; afterwards the set is what creation of the final list gives (rows the grown set has no room for are dropped,
 *   rows the creator asked for and an empty set could not have are built).  sigs, schemes and status may be host or device memory. */
#define BLSGPU_SIGSET_LINES 1
int blsgpu_sigset_create(int sig_group, const void* sigs, const uint8_t* schemes, size_t n, int fmt, int flags, int32_t* status, uint64_t* out_handle);
int blsgpu_sigset_destroy(uint64_t handle);
int blsgpu_sigset_info(uint64_t handle, int* sig_group, uint64_t* n, int* has_lines, uint64_t* device_bytes);
int blsgpu_sigset_append(uint64_t handle, const void* sigs, const uint8_t* schemes, size_t count, int fmt, int32_t* status, uint64_t* out_first);
/* blsgpu_pairing_batch with the signature-group member of pair i at entry idx[i] of a signature set and the other member (G2 under
 * Bls12381G1Impl, G1 under Bls12381G2Impl) in `points`, n of them in format fmt.  The same three outcomes: the 576 bytes of
 * Gt::to_bytes() with BLSGPU_OK; Gt one with BLSGPU_OK when a member is the identity; 576 zero bytes with the decode status when a
 * member did not decode (the G1 member's first; the entry's is its creation status).  And one more, before them: BLSGPU_E_ARG in the
 * slot, with 576 zero bytes, for an index outside the set; other items are unaffected and the call returns 0.  There are no groups
 * and the caller owes no order.  Every pointer may be host or device memory; the call runs on the set's device. */
int blsgpu_pairing_sigset_batch(uint64_t sigset, const uint32_t* idx, const void* points, size_t n, int fmt, uint8_t* out_gt, int32_t* status);
/* blsgpu_timecrypt_open_batch with item i's signature named as entry idx[i] of a signature set: no groups, no item offsets, no order.
 * us, vs, ws, w_offsets, ct_schemes, fmt, frames, pt_range and the w_offsets rule are that call's.  status[i] is the first of:
 * BLSGPU_E_ARG in the slot for an index outside the set (other items are unaffected and the call returns 0); otherwise exactly what
 * blsgpu_timecrypt_open_batch returns for the item in a group under the entry's signature and tag -- in order the decode status of
 * u_i, the entry's creation status, BLSGPU_INVALID_SCHEME, BLSGPU_SIG_IDENTITY, BLSGPU_PK_IDENTITY, BLSGPU_BAD_FRAME,
 * BLSGPU_INVALID_SIGNATURE, BLSGPU_OK.  A failed item's pt_range is (0, 0).  Every pointer may be host or device memory; w_offsets is
 * read and checked on the host; the call runs on the set's device.  Launch sequence: k_decompress of the u (wire formats),
 * k_sigset_prepare, the pairing-value step and k_timecrypt_open.  The step, below BLSGPU_VALUE_SPLIT_MIN items: chunks of at most
 * 4,096 items on k_pairing_value_rows over a Bls12381G2Impl set with rows, on k_pairing_value otherwise; from it up, chunks of
 * BLSGPU_MILLER_CHUNK items on k_millerf_rows1 (such a set) or k_linesp and k_millerfp3 (otherwise), then k_finalexp2s_value.  A call
 * that names an entry without usable rows walks, on either plan. */
int blsgpu_timecrypt_open_indexed_batch(uint64_t sigset, const uint32_t* idx, const void* us, const uint8_t* vs, const uint8_t* ws,
                                        const uint64_t* w_offsets, const uint8_t* ct_schemes, size_t n, int fmt, uint8_t* frames, uint64_t* pt_range,
                                        int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* BLSGPU_H */
