// libblsgpu.so: host side of the C ABI declared in include/blsgpu.h.  HIP runtime only (no torch types).
// There is no CPU compute path in this library: without a gfx950 device every entry point fails loudly.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/blsgpu.h"
#include "kernels.cuh"
#include "shares.cuh"
#include "secure.cuh"
#include "agg_batch.cuh"
#include "multi_batch.cuh"
#include "keyset.cuh"
#include "signcrypt.cuh"
#include "elgamal.cuh"
#include "verify_shared.cuh"
#include "msgset.cuh"
#include "agg_msgset.cuh"
#include "hkdf.cuh"
#include "timecrypt.cuh"
#include "sigset.cuh"
#include "debug_ops.h"
#include "host_sha256.h"

namespace {

const uint32_t FP_ONE_HOST[12] = FP_RAW_ONE_WORDS;   // 1 as the C ABI's Fp12 records carry it
thread_local std::string t_err;
thread_local size_t t_devidx = 0;    // which bound device the calling thread's leases come from (the sharded entry points set it)
thread_local bool t_nested = false;  // inside a sharded call: the per-device sub-calls must not shard again

enum {
  KID_PREPARE, KID_MILLER2, KID_FINALEXP, KID_PREPARE_AGG, KID_PAIRS_AFF, KID_MILLER1, KID_F12_FOLD, KID_FINALEXP_ONE,
  KID_HASH, KID_ACCUM, KID_POINT_FOLD, KID_COMPRESS, KID_SIGN, KID_F12_IO, KID_MSM_SORT, KID_MSM_BUCKET, KID_MSM_CHUNK, KID_DECOMPRESS, KID_PAIRING_COOP, KID_KEY_SORT, KID_COEFF, KID_DUP, KID_FIRST_BAD, KID_MSM_PREP, KID_MSM_NORM, KID_MSM_MERGE, KID_WIDE, KID_LINES, KID_CYCRUN,
  // round 4: one id per kernel on the paths bench.py reports (lumped ids made "the dominant kernel" meaningless)
  KID_MILLER2_V1, KID_FINALEXP_V1, KID_LINESP, KID_LINESP4, KID_LINE_QUAD, KID_F12_FOLD4, KID_F12_TREE, KID_HORNER, KID_MILLERFP, KID_PAIRING_POST, KID_PAIRING_PRE,
  KID_TAIL,        // everything launched on a context's tail stream: runs BESIDE the main stream's kernels, so its time is not additive
  KID_SHARE_LAGRANGE, KID_SHARE_LADDER, KID_SHARE_FOLD, KID_SHARE_OUT,     // threshold recovery (blsgpu_combine_shares)
  KID_SECURE_RANK, KID_SECURE_GATHER, KID_SECURE_DIGEST, KID_SECURE_COEFF, KID_SECURE_OUT, KID_SECURE_FIN,   // blsgpu_verify_secure_batch
  KID_AGG_SEG_INDEX, KID_AGG_SEG_FOLD, KID_AGG_SEG_FIN,   // blsgpu_aggregate_verify_batch (its prepare, Miller and final-exp kernels count under theirs)
  KID_MULTI_SEG_ACCUM, KID_MULTI_OUT,                     // blsgpu_multi_verify_batch (its fold counts under KID_SHARE_FOLD)
  KID_SIGNCRYPT_GATHER, KID_SIGNCRYPT_KEYSTREAM,          // blsgpu_signcrypt_share_verify_batch / blsgpu_signcrypt_open_batch
  KID_SECURE_FIRST, KID_SECURE_LADDER, KID_SECURE_AGG_FOLD, KID_SECURE_AGG_OUT,   // blsgpu_aggregate_secure_batch (rank .. coeff count under theirs)
  KID_SUM_SEG_ACCUM, KID_SUM_FOLD, KID_SUM_OUT,           // blsgpu_sum_batch
  KID_KEYSET_SEAL, KID_KEYSET_BUILD, KID_KEYSET_CHECK, KID_KEYSET_GATHER, KID_KEYSET_ACCUM, KID_KEYSET_MUL, KID_KEYSET_FIN,   // registered key sets (keyset.cuh)
  KID_ELGAMAL_PREP, KID_ELGAMAL_LADDER, KID_ELGAMAL_TRANSCRIPT, KID_ELGAMAL_SUB,   // blsgpu_elgamal_proof_verify_batch / blsgpu_elgamal_open_batch
  KID_GROUP_LINES, KID_PREPARE_SHARED,   // blsgpu_verify_shared_batch (verify_shared.cuh; k_group_affine and k_shared_expand count under k_prepare_shared, k_lines2s_shared under k_lines2s)
  KID_KEYSET_LINES, KID_LINES_KEYED,     // key sets with line tables (keyset.cuh): the build at creation, and the line kernel that reads both rows
  KID_LINESP_KEYED,                      // ... and the one of the batched aggregate verify over such a set (in the place of k_linesp)
  KID_KEYSET_SEAL_AT, KID_KEYSET_BUILD_AT, KID_KEYSET_LINES_AT,   // blsgpu_keyset_update / blsgpu_keyset_append: the positional forms of seal, build, lines
  KID_PAIRING_COOP_KEYED,                // the one-wave pairing that reads a registered key's rows (in the place of k_pairing_coop)
  KID_HASH_TO_SCALAR, KID_PROOF_CHALLENGE, KID_PROOF_TIMEOUT,   // blsgpu_hash_to_scalar, blsgpu_sig_proof_challenge_batch / _timestamp_verify_batch (hkdf.cuh)
  KID_MSGSET_SEAL, KID_MSGSET_CHECK,     // registered message sets (msgset.cuh; k_msgset_mark counts under k_msgset_check, the rows' build under k_keyset_lines[_at])
  KID_PAIRING_COOP_ROWS,                 // the one-wave pairing that reads a registered message's rows (in the place of k_pairing_coop)
  KID_AGGM_CLASS, KID_AGGM_SUM, KID_AGGM_ITEMS,   // aggregate verify by message index (agg_msgset.cuh): check / class table / numbering, the class key sum, the flat items
  KID_PAIRING_VALUE_PREP, KID_PAIRING_VALUE,      // blsgpu_pairing_batch (timecrypt.cuh): pairs to affine and flags, the one-wave pairing that exports Gt bytes
  KID_TIMECRYPT_PREP, KID_TIMECRYPT_OPEN,         // blsgpu_timecrypt_open_batch: statuses and pairs before the pairing, the time-lock tail after it
  KID_SIGSET_SEAL, KID_SIGSET_PREP,                // registered signature sets (sigset.cuh): create / append, the prepare kernel of both calls over a set
  KID_PAIRING_VALUE_ROWS,                          // the one-wave pairing value that reads a registered signature's rows (in the place of k_pairing_value)
  KID_FINALEXP_VALUE, KID_MILLERF_ROWS1,           // pairing values on the lane-split kernels (run_pairing_values): the final exponentiation with the Gt export, the tabled accumulator
  KID_PAIRING_COOP_TABLES2, KID_LINES_TABLES2,     // two tabled pairs with both tables in global memory (blsgpu_signcrypt_share_verify_indexed_batch): one wave per item, the lane-split line kernel
  KID_COUNT
};
#define KID_DEBUG_OPS KID_WIDE   // the self-test hooks share one profile id
const char* KID_NAMES[KID_COUNT] = {"k_prepare", "k_millerf2s", "k_finalexp2s", "k_prepare_agg", "k_pairs_to_affine", "k_miller1s", "k_f12_fold",
                                    "k_finalexp_one", "k_hash_to_point", "k_accumulate", "k_point_fold", "k_compress", "k_sign", "k_f12_io", "k_msm_sort", "k_msm_bucket", "k_msm_chunk", "k_decompress", "k_pairing_coop", "k_key_sort", "k_sha256_coeff", "k_duplicate_rule", "k_first_identity", "k_msm_prep", "k_normalize", "k_msm_merge", "k_wide", "k_lines2s", "k_cyc_run4",
                                    "k_miller2s", "k_finalexps", "k_linesp", "k_linesp4", "k_line_quad", "k_f12_fold4", "k_f12_tree_seg", "k_f12_horner_wide", "k_millerfp", "k_pairing_post", "k_pairing_pre",
                                    "tail_stream_overlapped", "k_share_lagrange", "k_share_ladder", "k_share_fold", "k_share_out",
                                    "k_secure_rank", "k_secure_gather", "k_secure_digest", "k_secure_coeff", "k_secure_out", "k_secure_fin",
                                    "k_agg_seg_index", "k_f12_fold_seg", "k_agg_batch_fin",
                                    "k_multi_accumulate_seg", "k_multi_out",
                                    "k_signcrypt_share_pairs", "k_signcrypt_keystream",
                                    "k_secure_first", "k_secure_ladder", "k_secure_agg_fold", "k_secure_agg_out",
                                    "k_sum_accumulate_seg", "k_sum_fold", "k_sum_out",
                                    "k_keyset_seal", "k_keyset_build", "k_keyset_check", "k_keyset_gather", "k_keyset_accumulate_seg", "k_keyset_mul", "k_keyset_fin",
                                    "k_elgamal_prep", "k_elgamal_ladder", "k_elgamal_transcript", "k_elgamal_sub",
                                    "k_group_lines", "k_prepare_shared",
                                    "k_keyset_lines", "k_lines2s_keyed",
                                    "k_linesp_keyed",
                                    "k_keyset_seal_at", "k_keyset_build_at", "k_keyset_lines_at",
                                    "k_pairing_coop_keyed",
                                    "k_hash_to_scalar", "k_proof_challenge", "k_proof_timeout",
                                    "k_msgset_seal", "k_msgset_check",
                                    "k_pairing_coop_rows",
                                    "k_agg_msgset_class", "k_agg_msgset_sum", "k_agg_msgset_items",
                                    "k_pairing_value_prepare", "k_pairing_value",
                                    "k_timecrypt_prepare", "k_timecrypt_open",
                                    "k_sigset_seal", "k_sigset_prepare",
                                    "k_pairing_value_rows",
                                    "k_finalexp2s_value", "k_millerf_rows1",
                                    "k_pairing_coop_tables2", "k_lines2s_tables2"};

struct Ctx {
  int dev = -1;
  hipStream_t stream = nullptr;
  uint8_t* arena = nullptr;
  size_t arena_cap = 0, arena_off = 0;
  std::mutex mu;
  hipEvent_t ev_host = nullptr;   // "the host may read what was copied so far" marker (verify_secure)
  hipStream_t side = nullptr;     // side stream: the message hash of a multi_verify tail runs beside the key sum
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipStream_t side2 = nullptr;    // second side stream: the signature's half of a cut pairing check beside the message hash
  hipEvent_t ev_join2 = nullptr;
  uint8_t* hpin = nullptr;        // pinned host staging (sorted key bytes on their way to the host's SHA-256 stream)
  size_t hpin_cap = 0;
  uint8_t* hsmall = nullptr;      // pinned 64 KiB for the small host <-> device records of a call (offsets, flags, verdicts):
  size_t hsmall_off = 0;          // they outlive every early return, unlike stack variables
  hipStream_t tail = nullptr;     // the leftover items of a pairing product (run_miller_product) run here beside the main chunks
  hipEvent_t ev_tail_fork = nullptr, ev_tail_join = nullptr;
  uint32_t* fold_ws = nullptr;    // two small ping-pong buffers of the engine levels of an Fp12 fold tree (run_f12_fold)
  uint32_t* lines_ws = nullptr;   // merged line values on their way from k_lines2s to k_millerf2s (kernels.cuh): 19 KB per lane
  size_t lines_cap = 0;           // bytes; grown on demand, kept between calls
  uint32_t* stream_flags = nullptr;   // hand-over flags of the streamed cut (kernels.cuh k_pairing_stream): written by that kernel only
  uint32_t stream_epoch = 0;          // the value its last launch on this context published with
  // optional per-kernel timing with HIP events on `stream` (blsgpu_profile_*)
  bool prof_on = false;
  struct Pending { int kid; hipEvent_t e0, e1; };
  std::vector<Pending> prof_pending;
  std::vector<hipEvent_t> prof_pool;
  double prof_ms[KID_COUNT] = {0};
  uint64_t prof_cnt[KID_COUNT] = {0};
};
// One pool of contexts per bound device: a call leases a free context (own stream, own arena, own mutex), so concurrent
// callers overlap on the device instead of queueing behind one mutex.  Device index 0 is the device of blsgpu_init.
struct Device {
  int dev = -1;
  std::vector<Ctx*> pool;
  std::atomic<unsigned> rr{0};
};
std::vector<Device*> g_devices;     // written only under g_init_mu, before any compute call / after all of them
bool g_peer_ok = true;              // every bound device can read every other one's memory (needed to shard DEVICE buffers)
std::mutex g_init_mu;
bool initialised() { return !g_devices.empty(); }

void trim_workspaces(Ctx* c);
struct Lease {
  Ctx* c = nullptr;
  std::unique_lock<std::mutex> lk;
  Lease() = default;
  Lease(Lease&&) = default;
  // An entry point that fails half-way returns without having synchronised: drain what it enqueued before the caller's
  // buffers (and this context) are reused.  After a normal return every stream is idle and the queries cost nothing.
  ~Lease() {
    if (!c) return;
    for (hipStream_t s : {c->stream, c->side, c->side2, c->tail})
      if (s && hipStreamQuery(s) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(s);
      }
    trim_workspaces(c);
  }
};
Lease acquire_ctx(size_t devidx) {
  Device* d = g_devices[devidx];
  Lease L;
  for (Ctx* c : d->pool) {
    std::unique_lock<std::mutex> lk(c->mu, std::try_to_lock);
    if (lk.owns_lock()) {
      L.c = c;
      L.lk = std::move(lk);
      return L;
    }
  }
  Ctx* c = d->pool[d->rr.fetch_add(1) % d->pool.size()];
  L.lk = std::unique_lock<std::mutex>(c->mu);
  L.c = c;
  return L;
}
#define CTX_ACQUIRE_ON(c, devidx)        \
  Lease lease_ = acquire_ctx(devidx);     \
  Ctx* c = lease_.c;                      \
  c->hsmall_off = 0;                      \
  HIPCK(hipSetDevice(c->dev))
#define CTX_ACQUIRE(c) CTX_ACQUIRE_ON(c, t_devidx)
#define NOT_INIT() fail(BLSGPU_E_NOT_INIT, "blsgpu_init has not been called (or found no gfx950 device)")
// no C++ exception may unwind into a C / Rust caller
#define API_CATCH                                                                              \
  catch (const std::bad_alloc&) { return fail(BLSGPU_E_HIP, "out of host memory"); }           \
  catch (const std::exception& e) { return fail(BLSGPU_E_HIP, std::string("internal: ") + e.what()); } \
  catch (...) { return fail(BLSGPU_E_HIP, "internal: unknown exception"); }

int fail(int code, const std::string& msg) {
  t_err = msg;
  return code;
}
// ---- run-time knobs: every BLSGPU_* environment variable the library reads, parsed ONCE into one struct (VERDICT r3 weak #9,
// next #7).  Two classes:
//   tuning  documented in README.md, clamped to what the kernels assume, change plans and sizes, never results;
//   A/B     select kernel forms kept for measurements and for the suite's agreement tests; honoured only together with
//           BLSGPU_AB_KNOBS=1, so that a single stray variable in somebody else's process cannot switch the product's kernels.
// BLSGPU_STRICT_ENV=1: blsgpu_init refuses to start when the environment holds a BLSGPU_ variable this table does not know, or an
// A/B variable without the gate (a typo or a leftover must not go unnoticed in production).
extern "C" char** environ;
// blsgpu_verify_shared_batch, BLSGPU_SHARED_LINES_MIN unset: the per-group line tables are taken from this many items per group on
// average in a batch of at least this many items ("Shared-message verify": tools/bench_verify_shared.py -- a
// group's walk is one serial pass however few groups there are, so it pays where the pass it saves runs more than once)
#define SHARED_LINES_AUTO_MIN 4
#define SHARED_LINES_AUTO_ITEMS 98304
// blsgpu_pairing_batch, blsgpu_timecrypt_open_batch and the two calls over a signature set, BLSGPU_VALUE_SPLIT_MIN unset: from this
// many items the pairing values run on the lane-split kernels (run_pairing_values).  DESIGN.md section 4, "Pairing values on the
// lane-split kernels", has the measurement the figure follows from (tools/bench_value_split.py, profiles/value_split_bench.json).
#define VALUE_SPLIT_MIN_DEFAULT 8192
// blsgpu_signcrypt_share_verify_indexed_batch, Bls12381G2Impl, BLSGPU_SIGNCRYPT_LINES_MIN unset: the ciphertexts' line tables are built
// from this many shares per ciphertext on average.  DESIGN.md section 4, "Signcryption shares by key index", has the measurement the figure
// follows from (tools/bench_signcrypt_indexed.py, profiles/signcrypt_indexed_bench.json): the row builder's one serial walk costs
// 1.9 ms however few points it takes, which the tabled kernels win back at 256 x 16 and 1,024 x 64 shares and not at 64 x 32.
#define SIGNCRYPT_LINES_MIN_DEFAULT 64
struct Knobs {
  long coop_max = 4096, wide_max = 512, shard_min = 8192, contexts = 2, fake_devices = 0, acc_lanes = 57344;
  long msm_c = 0, msm_ch = 0, msm2_c = 0, msm2_ch = 0, msm2_q = 0;          // 0: the library's own choice
  long msm2_tables = 1;       // verify_secure: weighted window tables of every key, built while the host hashes (0: off)
  long stream_lines = 1;      // a check whose lines cannot be had early runs them BESIDE its Miller loop (k_pairing_stream; 0: two launches)
  long post_split = 3;        // the late part of a cut check runs its Miller loop on this many workgroups (k_pairing_post2: 3, 2; 0 or 1: one)
  long host_trace = 0, strict_env = 0, ab_knobs = 0;
  long shares_msm_min = 1024; // blsgpu_combine_shares: a set of at least this many shares is summed by the bucket MSM, not per-share ladders
  long secure_batch_max = 1024; // blsgpu_verify_secure_batch, blsgpu_aggregate_secure_batch: a set of at least this many keys runs through blsgpu_verify_secure's machinery
  long agg_batch_max = 32768;  // blsgpu_aggregate_verify_batch: a set of at least this many pairs runs through blsgpu_aggregate_verify's machinery
  long multi_strip = 0;        // blsgpu_multi_verify_batch: keys per strip of the segmented key sum (0: one strip per lane of a single sum, at least 4)
  long keyset_table_mb = 4096; // blsgpu_keyset_create: fixed-base and line tables above this many MiB together are not built (the set works without them)
  long ws_keep_mb = 4096;     // a context's line workspace above this many MiB is released when the call that grew it returns
  long value_split_min = VALUE_SPLIT_MIN_DEFAULT;   // the pairing-value calls: the smallest item count that takes the lane-split kernels (0: never); never changes a result
  long shared_lines_min = -1; // blsgpu_verify_shared_batch, Bls12381G2Impl: per-group line tables from this many items per group on average (0: never; unset: SHARED_LINES_AUTO_*)
  long signcrypt_lines_min = SIGNCRYPT_LINES_MIN_DEFAULT;   // blsgpu_signcrypt_share_verify_indexed_batch, Bls12381G2Impl: the ciphertexts' line tables from this many shares per ciphertext on average (0: never); never changes a result
  // A/B
  long miller_chunk = 65536, miller_v1 = 0, row_pad = 192, wide_mode = 2, finalexp_seg = 0, finalexp_v1 = 0, prepare_lanes = 0, product_tree = 1,
       tree_local = 0, lines4_max = -1, tree_engine_from = 0, agg_lanes = 0, msm_v1 = 0, msm_naive = 0, wide_test_block = 64;
  std::string problem;        // what BLSGPU_STRICT_ENV objects to (empty: nothing)
};
struct KnobSpec { const char* name; long Knobs::*field; long lo, hi; bool ab; };
const KnobSpec KNOB_TABLE[] = {
    {"BLSGPU_COOP_MAX", &Knobs::coop_max, 0, 1 << 20, false},          {"BLSGPU_WIDE_MAX", &Knobs::wide_max, 0, 4096, false},
    {"BLSGPU_SHARD_MIN", &Knobs::shard_min, 1, 1L << 40, false},        {"BLSGPU_CONTEXTS", &Knobs::contexts, 1, 16, false},
    {"BLSGPU_FAKE_DEVICES", &Knobs::fake_devices, 0, 64, false},        {"BLSGPU_ACC_LANES", &Knobs::acc_lanes, 64, 1 << 20, false},
    {"BLSGPU_MSM_C", &Knobs::msm_c, 4, 16, false},                      {"BLSGPU_MSM_CH", &Knobs::msm_ch, 1, 1 << 16, false},
    {"BLSGPU_MSM2_C", &Knobs::msm2_c, 4, 16, false},                    {"BLSGPU_MSM2_CH", &Knobs::msm2_ch, 1, 1 << 16, false},
    {"BLSGPU_MSM2_Q", &Knobs::msm2_q, 1, 8, false},                     {"BLSGPU_HOST_TRACE", &Knobs::host_trace, 0, 1, false},
    {"BLSGPU_WS_KEEP_MB", &Knobs::ws_keep_mb, 0, 1L << 20, false},        {"BLSGPU_MSM2_TABLES", &Knobs::msm2_tables, 0, 1, false},
    {"BLSGPU_STREAM_LINES", &Knobs::stream_lines, 0, 1, false},        {"BLSGPU_POST_SPLIT", &Knobs::post_split, 0, 3, false},
    {"BLSGPU_STRICT_ENV", &Knobs::strict_env, 0, 1, false},             {"BLSGPU_AB_KNOBS", &Knobs::ab_knobs, 0, 1, false},
    {"BLSGPU_SHARES_MSM_MIN", &Knobs::shares_msm_min, 2, 1L << 32, false},
    {"BLSGPU_SECURE_BATCH_MAX", &Knobs::secure_batch_max, 1, 1L << 32, false},
    {"BLSGPU_AGG_BATCH_MAX", &Knobs::agg_batch_max, 1, 1L << 32, false},
    {"BLSGPU_MULTI_STRIP", &Knobs::multi_strip, 0, 1L << 32, false},
    {"BLSGPU_KEYSET_TABLE_MB", &Knobs::keyset_table_mb, 0, 1L << 20, false},
    {"BLSGPU_SHARED_LINES_MIN", &Knobs::shared_lines_min, 0, 1L << 32, false},
    {"BLSGPU_VALUE_SPLIT_MIN", &Knobs::value_split_min, 0, 1L << 32, false},
    {"BLSGPU_SIGNCRYPT_LINES_MIN", &Knobs::signcrypt_lines_min, 0, 1L << 32, false},
    {"BLSGPU_MILLER_CHUNK", &Knobs::miller_chunk, 0, 65536, true},      {"BLSGPU_MILLER_V1", &Knobs::miller_v1, 0, 1, true},
    {"BLSGPU_ROW_PAD", &Knobs::row_pad, 0, 4096, true},                 {"BLSGPU_WIDE_MODE", &Knobs::wide_mode, 1, 2, true},
    {"BLSGPU_FINALEXP_SEG", &Knobs::finalexp_seg, 0, 1, true},          {"BLSGPU_FINALEXP_V1", &Knobs::finalexp_v1, 0, 1, true},
    {"BLSGPU_PREPARE_LANES", &Knobs::prepare_lanes, 0, 2, true},        {"BLSGPU_PRODUCT_TREE", &Knobs::product_tree, 0, 1, true},
    {"BLSGPU_TREE_LOCAL", &Knobs::tree_local, 0, 65536, true},          {"BLSGPU_LINES4_MAX", &Knobs::lines4_max, 0, 65536, true},
    {"BLSGPU_TREE_ENGINE_FROM", &Knobs::tree_engine_from, 0, 256, true}, {"BLSGPU_AGG_LANES", &Knobs::agg_lanes, 0, 2, true},
    {"BLSGPU_MSM_V1", &Knobs::msm_v1, 0, 1, true},                      {"BLSGPU_MSM_NAIVE", &Knobs::msm_naive, 0, 1, true},
    {"BLSGPU_WIDE_TEST_BLOCK", &Knobs::wide_test_block, 64, 256, true},
};
// read by the Python wrapper / debug builds only, never by this file's product paths: known names for the strict check
const char* const KNOB_OTHER_NAMES[] = {"BLSGPU_LIB", "BLSGPU_HASH_STOP"};
Knobs parse_knobs() {
  Knobs k;
  const char* gate = getenv("BLSGPU_AB_KNOBS");
  const bool ab_ok = gate && atol(gate) == 1;
  for (const KnobSpec& sp : KNOB_TABLE) {
    const char* e = getenv(sp.name);
    if (!e || !*e) continue;
    if (sp.ab && !ab_ok) {
      if (k.problem.empty()) k.problem = std::string(sp.name) + " is an A/B switch and needs BLSGPU_AB_KNOBS=1";
      fprintf(stderr, "libblsgpu: ignoring %s (an A/B switch: set BLSGPU_AB_KNOBS=1 to honour it)\n", sp.name);
      continue;
    }
    char* end = nullptr;
    long v = strtol(e, &end, 10);
    if (end == e || *end) {
      if (k.problem.empty()) k.problem = std::string(sp.name) + " is not an integer";
      continue;
    }
    k.*sp.field = v < sp.lo ? sp.lo : v > sp.hi ? sp.hi : v;     // clamped: a wild value cannot force a fallback by exhausting memory
  }
  for (char** e = environ; e && *e; e++) {
    if (strncmp(*e, "BLSGPU_", 7) != 0) continue;
    const char* eq = strchr(*e, '=');
    const std::string name(*e, eq ? (size_t)(eq - *e) : strlen(*e));
    bool known = false;
    for (const KnobSpec& sp : KNOB_TABLE) known = known || name == sp.name;
    for (const char* o : KNOB_OTHER_NAMES) known = known || name == o;
    if (!known && k.problem.empty()) k.problem = "unknown variable " + name;
  }
  return k;
}
// Parsed when the library binds its devices (blsgpu_init / blsgpu_init_devices on an unbound library, under g_init_mu) and constant
// until blsgpu_shutdown: no compute call can run while the library is unbound, so nobody reads the struct while it is rewritten.
Knobs g_knobs;
const Knobs& knobs() { return g_knobs; }

#define HIPCK(x)                                                                                   \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) {                                                                        \
      (void)hipGetLastError();                                                                     \
      return fail(BLSGPU_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_));                 \
    }                                                                                              \
  } while (0)

bool is_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// ---- bump arena in device memory, reset per call
size_t wide_max_items();
int arena_reserve(Ctx* c, size_t bytes) {
  bytes += (1u << 20) + wide_max_items() * (size_t)WREC_WORDS * 4;   // headroom that every call may rely on: the row-wide engine's per-item records
  if (bytes <= c->arena_cap) return 0;
  HIPCK(hipStreamSynchronize(c->stream));
  if (c->arena) HIPCK(hipFree(c->arena));
  c->arena = nullptr;
  c->arena_cap = 0;
  size_t cap = bytes + bytes / 8 + (1u << 20);
  HIPCK(hipMalloc((void**)&c->arena, cap));
  c->arena_cap = cap;
  return 0;
}
void* arena_take(Ctx* c, size_t bytes) {
  size_t off = (c->arena_off + 255) & ~(size_t)255;
  if (off + bytes > c->arena_cap) return nullptr;
  c->arena_off = off + bytes;
  return c->arena + off;
}
size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// small pinned records of a call (see Ctx::hsmall)
const size_t HSMALL_BYTES = 65536;
void* hsmall_take(Ctx* c, size_t bytes) {
  size_t off = (c->hsmall_off + 63) & ~(size_t)63;
  if (off + bytes > HSMALL_BYTES) return nullptr;
  c->hsmall_off = off + bytes;
  return c->hsmall + off;
}
// host -> device copy of a few bytes that live on the caller's stack
int h2d_small(Ctx* c, void* d, const void* src, size_t bytes) {
  void* h = hsmall_take(c, bytes);
  if (!h) return fail(BLSGPU_E_HIP, "internal: pinned record buffer exhausted");
  memcpy(h, src, bytes);
  HIPCK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
  return 0;
}
// One device word back to the host, where a plan waits for it: the launches before it checked, one copy into 4 pinned bytes and ONE
// synchronisation -- the caller's only one before its final copy-out.
int word_back(Ctx* c, const void* d_word, uint32_t* value) {
  uint32_t* h = (uint32_t*)hsmall_take(c, 4);
  if (!h) return fail(BLSGPU_E_HIP, "internal: pinned record buffer exhausted");
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, d_word, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BLSGPU_E_HIP, "a word's way back to the host failed: a launch before it, its copy or the synchronisation");
  }
  *value = *h;
  return 0;
}
// the way out of a call whose pending uploads read host vectors of its frame: nothing returns before the stream has drained
int drain(Ctx* c, int rc) {
  (void)hipStreamSynchronize(c->stream);
  return rc;
}

// device view of an input buffer: device pointers pass through, host buffers are staged into the arena
int stage_in(Ctx* c, const void* p, size_t bytes, const void** out) {
  if (bytes == 0) {
    *out = c->arena;
    return 0;
  }
  if (is_device_ptr(p)) {
    *out = p;
    return 0;
  }
  void* d = arena_take(c, bytes);
  if (!d) return fail(BLSGPU_E_HIP, "internal: arena too small");
  HIPCK(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, c->stream));
  *out = d;
  return 0;
}
// Several SMALL host buffers of one call (a single verification's key, signature, message, offsets) as ONE host-to-device copy
// through the context's pinned ring instead of one pageable copy each (~8 us apiece on the latency path).  Returns false when it
// does not apply (a device pointer among them, too large, ring full): the caller then stages one by one.
bool stage_in_packed(Ctx* c, const void* const* ptrs, const size_t* sizes, const void** outs, int k) {
  size_t total = 0;
  for (int j = 0; j < k; j++) {
    if (sizes[j] && is_device_ptr(ptrs[j])) return false;
    total += pad256(sizes[j]);
  }
  if (total == 0 || total > 16384) return false;
  uint8_t* h = (uint8_t*)hsmall_take(c, total);
  uint8_t* d = h ? (uint8_t*)arena_take(c, total) : nullptr;
  if (!h || !d) return false;
  size_t off = 0;
  for (int j = 0; j < k; j++) {
    if (sizes[j]) memcpy(h + off, ptrs[j], sizes[j]);
    outs[j] = d + off;
    off += pad256(sizes[j]);
  }
  if (hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}
int copy_out(Ctx* c, void* dst, const void* dsrc, size_t bytes) {
  if (bytes == 0) return 0;
  HIPCK(hipMemcpyAsync(dst, dsrc, bytes, is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  return 0;
}
// device view of an output buffer, the mirror of stage_in: a device pointer passes through, a host buffer gets arena bytes
// (nullptr: the arena is too small) that stage_back copies to it after the kernels that write them
template <class T>
T* stage_out(Ctx* c, void* out, size_t bytes) {
  return is_device_ptr(out) ? (T*)out : (T*)arena_take(c, bytes);
}
int stage_back(Ctx* c, void* out, const void* d, size_t bytes) { return d == out ? 0 : copy_out(c, out, d, bytes); }
// The buffers of a call, one per line: take (arena bytes) and stage_out (as above) clear `ok` when the arena refuses, and the call
// tests `ok` once after the last of them, before any kernel gets a pointer.
struct Carver {
  Ctx* c;
  bool ok = true;
  template <class T>
  T* take(size_t bytes) {
    T* p = (T*)arena_take(c, bytes);
    ok = ok && p;
    return p;
  }
  template <class T>
  T* stage_out(void* out, size_t bytes) { return is_device_ptr(out) ? (T*)out : take<T>(bytes); }
};
// the n + 1 offsets of a ragged argument, read on the host (they decide every size of the call) and checked: they never decrease,
// and start at 0 unless the caller indexes its flat array from offs[0] (from_zero = false)
int read_offsets(const uint64_t* p, size_t n, const char* what, std::vector<uint64_t>& offs, bool from_zero = true) {
  offs.resize(n + 1);
  if (is_device_ptr(p)) HIPCK(hipMemcpy(offs.data(), p, 8 * (n + 1), hipMemcpyDeviceToHost));
  else memcpy(offs.data(), p, 8 * (n + 1));
  if (from_zero && offs[0] != 0) return fail(BLSGPU_E_ARG, std::string(what) + "[0] must be 0");
  for (size_t s = 0; s < n; s++)
    if (offs[s + 1] < offs[s]) return fail(BLSGPU_E_ARG, std::string(what) + " must not decrease");
  return 0;
}
int upload_offsets(Ctx* c, const std::vector<uint64_t>& offs, const uint64_t** d) {
  void* p = arena_take(c, 8 * offs.size());
  if (!p) return fail(BLSGPU_E_HIP, "internal: arena too small");
  HIPCK(hipMemcpyAsync(p, offs.data(), 8 * offs.size(), hipMemcpyHostToDevice, c->stream));
  *d = (const uint64_t*)p;
  return 0;
}
// a call's single verdict, decided on the host, to wherever the caller keeps it
int put_i32(int32_t* dst, int32_t v) {
  if (is_device_ptr(dst)) HIPCK(hipMemcpy(dst, &v, 4, hipMemcpyHostToDevice));
  else *dst = v;
  return 0;
}

// a call's verdicts: copy, then wait for the stream.  A few verdicts for host memory travel through the pinned record buffer (a
// device-to-host copy into pageable memory makes the runtime stage and wait internally, ~10 us more on a 1.5 ms call).
void prof_flush(Ctx* c);
int copy_out_and_sync(Ctx* c, void* dst, const void* dsrc, size_t bytes) {
  void* h = nullptr;
  if (bytes && bytes <= 4096 && !is_device_ptr(dst) && (h = hsmall_take(c, bytes))) {
    HIPCK(hipMemcpyAsync(h, dsrc, bytes, hipMemcpyDeviceToHost, c->stream));
  } else {
    int rc = copy_out(c, dst, dsrc, bytes);
    if (rc) return rc;
  }
  HIPCK(hipStreamSynchronize(c->stream));
  prof_flush(c);
  if (h) memcpy(dst, h, bytes);
  return 0;
}

// the statuses of a call on their way to the caller.  A device-side hand-over that ran out of its bounded wait (kernels.cuh
// BLS_ERR_STREAM_TIMEOUT; the only other negative value a kernel writes into a status is k_proof_timeout's BLSGPU_E_ARG, which IS
// the item's verdict) is a failure of the CALL, not a verdict:
// wherever the host gets to see the statuses it says so with the return code; a caller that keeps them on the device finds the
// -2 in the item's entry (include/blsgpu.h).
int status_out_and_sync(Ctx* c, int32_t* status, const int32_t* d_status, size_t n) {
  int rc = copy_out_and_sync(c, status, d_status, 4 * n);
  if (rc) return rc;
  if (n <= WPOST2_MAX_ITEMS && !is_device_ptr(status))
    for (size_t i = 0; i < n; i++)
      if (status[i] == BLS_ERR_STREAM_TIMEOUT) return fail(BLSGPU_E_HIP, "a workgroup hand-over on the device ran out of its bounded wait");
  return 0;
}

// bytes of one point of `group` (1: G1, 2: G2, twice as wide) in a caller format; the two compressed formats are equally long.
// This and key_group hold for group 1 or 2 only: every entry point checks its group argument before it gets here.
size_t point_bytes(int group, int fmt) {
  return (size_t)group * (fmt == BLSGPU_FMT_RAW_PROJ ? 144 : fmt == BLSGPU_FMT_RAW_AFFINE ? 96 : 48);
}
int key_group(int sig_group) { return 3 - sig_group; }   // the keys live in the group the signatures do not
size_t pk_size(int sg, int fmt) { return point_bytes(key_group(sg), fmt); }
size_t sig_size(int sg, int fmt) { return point_bytes(sg, fmt); }

const char* DST_TABLE[2][3] = {
    {"BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_", "BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_AUG_",
     "BLS_SIG_BLS12381G1_XMD:SHA-256_SSWU_RO_POP_"},  // reference src/impls/g1.rs:110,114,118
    {"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_", "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_AUG_",
     "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"},  // reference src/impls/g2.rs:108,112,116
};
// RFC 9380 section 5.3.3: a domain separation tag longer than 255 bytes enters expand_message_xmd as
// SHA-256("H2C-OVERSIZE-DST-" || DST) -- the interface this replaces takes any DST (reference src/traits/hash_to_point.rs:11,
// src/impls/g1.rs:17-19, g2.rs:15-17: ExpandMsgXmd<Sha256> in the dependency applies the same rule)
dst_arg make_dst(const uint8_t* d, size_t n) {
  dst_arg a;
  memset(&a, 0, sizeof a);
  if (n > 255) {
    host_sha256 h;
    h.update((const uint8_t*)"H2C-OVERSIZE-DST-", 17);
    h.update(d, n);
    h.final(a.b);
    a.len = 32;
    return a;
  }
  if (n) memcpy(a.b, d, n);
  a.len = (uint32_t)n;
  return a;
}
dst_arg scheme_dst(int sg, int scheme) {
  const char* s = DST_TABLE[sg - 1][scheme];
  return make_dst((const uint8_t*)s, strlen(s));
}

int check_common(int sg, int scheme, int fmt) {
  if (!initialised()) return NOT_INIT();
  if (sg != 1 && sg != 2) return fail(BLSGPU_E_ARG, "sig_group must be 1 (Bls12381G1Impl) or 2 (Bls12381G2Impl)");
  if (scheme < 0 || scheme > 2) return fail(BLSGPU_E_ARG, "scheme must be 0 (Basic), 1 (MessageAugmentation) or 2 (ProofOfPossession)");
  if (fmt != BLSGPU_FMT_RAW_PROJ && fmt != BLSGPU_FMT_RAW_AFFINE)
    return fail(BLSGPU_E_ARG, "this entry point takes BLSGPU_FMT_RAW_PROJ or BLSGPU_FMT_RAW_AFFINE points");
  return 0;
}
// the key serialisation of the secure calls; blsgpu_aggregate_secure has always given the Legacy refusal without its citation
int check_ser_format(int sig_group, int ser_format, bool cite = true) {
  if (ser_format != 0 && ser_format != 1) return fail(BLSGPU_E_ARG, "ser_format must be 0 (Modern) or 1 (Legacy)");
  if (ser_format == 1 && sig_group != 2)
    return fail(BLSGPU_E_ARG, std::string("Legacy serialization exists only for Bls12381G2Impl") +
                                  (cite ? " (48-byte keys), reference src/signature.rs:201-204" : ""));
  return 0;
}

hipEvent_t prof_event(Ctx* c) {
  if (!c->prof_pool.empty()) {
    hipEvent_t e = c->prof_pool.back();
    c->prof_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
void prof_pre(Ctx* c, int kid, hipStream_t s = nullptr) {
  if (!c->prof_on) return;
  Ctx::Pending p{kid, prof_event(c), prof_event(c)};
  (void)hipEventRecord(p.e0, s ? s : c->stream);
  c->prof_pending.push_back(p);
}
void prof_post(Ctx* c, hipStream_t s = nullptr) {
  if (!c->prof_on) return;
  (void)hipEventRecord(c->prof_pending.back().e1, s ? s : c->stream);
}
// call after the stream has been synchronised
void prof_flush(Ctx* c) {
  for (auto& p : c->prof_pending) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
      c->prof_ms[p.kid] += ms;
      c->prof_cnt[p.kid]++;
    } else {
      (void)hipGetLastError();
    }
    c->prof_pool.push_back(p.e0);
    c->prof_pool.push_back(p.e1);
  }
  c->prof_pending.clear();
}
#define KL(kid, kern, grid, block, ...)                                         \
  do {                                                                          \
    prof_pre(c, kid);                                                           \
    hipLaunchKernelGGL(kern, grid, block, 0, c->stream, __VA_ARGS__);           \
    prof_post(c);                                                               \
  } while (0)
// a launch on another stream of the context (tail / side): recorded with events on THAT stream; the stream is joined to the main
// one before the call's final synchronisation, so prof_flush finds the events complete
#define KLS(kid, strm, kern, grid, block, ...)                                  \
  do {                                                                          \
    prof_pre(c, kid, strm);                                                     \
    hipLaunchKernelGGL(kern, grid, block, 0, strm, __VA_ARGS__);                \
    prof_post(c, strm);                                                         \
  } while (0)
// The run-time group as a compile-time one: f gets std::integral_constant<int, 1> or <int, 2>, so a generic lambda names
// k_x<G()> / run_x<G()> once for both groups.  Returns what f returns: an rc, or nothing when f is a bare launch (KL needs `c`
// in scope; HIPCK / fail return from the lambda, not from its caller, so they stay outside or travel as the rc).
template <class F>
auto with_group(int group, F&& f) {
  if (group == 1) return f(std::integral_constant<int, 1>());
  return f(std::integral_constant<int, 2>());
}
// one Miller loop per MILLER1_GROUP items: leaves ceil(cnt / MILLER1_GROUP) partial products at the start of the Fp12 workspace
#define MILLER1_OUTPUTS(cnt) (((cnt) + MILLER1_GROUP - 1) / MILLER1_GROUP)
#define MILLER1_LAUNCH(cnt, ...) KL(KID_MILLER1, k_miller1s, dim3(blocks_for(2 * MILLER1_OUTPUTS(cnt))), dim3(BLS_BLOCK), cnt, __VA_ARGS__)
#define SYNC_FLUSH(c)                          \
  do {                                         \
    HIPCK(hipStreamSynchronize((c)->stream));  \
    prof_flush(c);                             \
  } while (0)

// batches up to this size use the wave-cooperative pairing (one wave per item); BLSGPU_COOP_MAX overrides (0 = never)
size_t coop_max_items() {
  // default 4096: measured crossover with the lane-split kernels (tools/dbg/mid3.py, round 3: whole calls from host lists): 11.4 vs 12.0 ms at
  // 3,072 items, 12.1 vs 12.1 at 4,096, 17.4 vs 12.5 at 6,144 (rounds 1-2, the one-kernel Miller loop: 6,144)
  return (size_t)knobs().coop_max;
}

// batches up to this size finish on the row-wide engine (one 256-thread workgroup per item; csrc/wide_engine.cuh):
// BLSGPU_WIDE_MAX overrides (0 = never).  One workgroup occupies the four SIMDs of a CU, so 256 items run side by side.
// measurement aid (tools/dbg/hash_phases.py): BLSGPU_HASH_STOP=k makes k_hash_to_g1_wide return after its k-th phase when it is
// launched through blsgpu_hash_to_g1 (the output is then meaningless); 0 / unset: the whole hash
int hash_phase_stop();
int hash_phase_stop() {
#if defined(BLS_DEBUG_KNOBS)        // measurement builds only (tools/dbg/hash_phases.py, hash2.py): a stray environment variable must
  const char* e = getenv("BLSGPU_HASH_STOP");   // not change hash outputs and verdicts of the product library
  return e ? atoi(e) & 0xff : 0;
#else
  return 0;
#endif
}
size_t wide_max_items() {
  // default 512: measured (tools/dbg/small.py): 1.9 ms up to 256 items (one workgroup per CU), 3.4 ms at 512, 5.3 ms at 768; the wave-cooperative path: 4.6-4.8 ms flat
  return (size_t)knobs().wide_max;
}

unsigned blocks_for(size_t n) { return (unsigned)((n + BLS_BLOCK - 1) / BLS_BLOCK); }

int pinned_reserve(Ctx* c, size_t bytes) {
  if (bytes <= c->hpin_cap) return 0;
  if (c->hpin) HIPCK(hipHostFree(c->hpin));
  c->hpin = nullptr;
  c->hpin_cap = 0;
  HIPCK(hipHostMalloc((void**)&c->hpin, bytes + bytes / 8 + 4096, hipHostMallocDefault));
  c->hpin_cap = bytes + bytes / 8 + 4096;
  return 0;
}

// exclusive prefix sum of m u32 counters (three launches, util_kernels.cuh); d_tiles: scan_tiles(m) words
size_t scan_tiles(size_t m) { return (m + UK_SCAN_TILE - 1) / UK_SCAN_TILE; }
int run_scan_u32(Ctx* c, int kid, size_t m, const uint32_t* d_in, uint32_t* d_out, uint32_t* d_tiles) {
  if (m == 0) return 0;
  const unsigned nt = (unsigned)scan_tiles(m);
  KL(kid, k_scan_tiles, dim3(nt), dim3(BLS_BLOCK), m, d_in, d_out, d_tiles);
  if (nt > 1) {
    KL(kid, k_scan_top, dim3(1), dim3(BLS_BLOCK), (size_t)nt, d_tiles);
    KL(kid, k_scan_apply, dim3(nt), dim3(BLS_BLOCK), m, d_out, (const uint32_t*)d_tiles);
  }
  HIPCK(hipGetLastError());
  return 0;
}
int run_scan_max_u32(Ctx* c, int kid, size_t m, uint32_t* d_v, uint32_t* d_tiles) {
  if (m == 0) return 0;
  const unsigned nt = (unsigned)scan_tiles(m);
  KL(kid, k_scan_max_tiles, dim3(nt), dim3(BLS_BLOCK), m, d_v, d_tiles);
  if (nt > 1) {
    KL(kid, k_scan_max_top, dim3(1), dim3(BLS_BLOCK), (size_t)nt, d_tiles);
    KL(kid, k_scan_max_apply, dim3(nt), dim3(BLS_BLOCK), m, d_v, (const uint32_t*)d_tiles);
  }
  HIPCK(hipGetLastError());
  return 0;
}



// ---- one process, several GPUs (blsgpu_init_devices): the items of a call are cut into contiguous ranges, one per bound
// device, each handled by a host thread whose leases come from that device's context pool
size_t shard_min_items() { return (size_t)knobs().shard_min; }   // BLSGPU_SHARD_MIN: below this many items a call stays on device 0
// how many devices a call over n items uses; device-resident inputs can only be sharded when the devices see each other
size_t shard_devices(size_t n, std::initializer_list<const void*> inputs) {
  if (t_nested || g_devices.size() < 2 || n < shard_min_items()) return 1;
  if (!g_peer_ok)
    for (const void* p : inputs)
      if (is_device_ptr(p)) return 1;
  size_t d = g_devices.size();
  while (d > 1 && n / d < shard_min_items() / 4) d--;
  return d;
}
// a helper thread that is joined when its owner goes out of scope, whichever way: an exception between the start of a helper and
// its join must unwind into API_CATCH, not into std::terminate of a process that holds the GPU (advisor finding, round 2)
struct JoinedThread {
  std::thread t;
  JoinedThread() = default;
  template <class F, class... A>
  explicit JoinedThread(F&& f, A&&... a) : t(std::forward<F>(f), std::forward<A>(a)...) {}
  JoinedThread(JoinedThread&&) = default;
  JoinedThread& operator=(JoinedThread&& o) {
    if (t.joinable()) t.join();
    t = std::move(o.t);
    return *this;
  }
  void join() { if (t.joinable()) t.join(); }
  ~JoinedThread() { if (t.joinable()) t.join(); }
};
// fn(d) for d < k on k host threads (thread d leases from device d); the first failure wins and its message is kept
template <class F>
int run_on_devices(size_t k, F&& fn) {
  std::vector<int> rcs(k, 0);
  std::vector<std::string> errs(k);
  std::vector<JoinedThread> th;        // joined on every way out, also when body(0) or an emplace_back throws
  auto body = [&](size_t d) {
    t_devidx = d;
    t_nested = true;
    try {
      rcs[d] = fn(d);
    } catch (const std::exception& e) {
      rcs[d] = fail(BLSGPU_E_HIP, std::string("internal: ") + e.what());
    } catch (...) {
      rcs[d] = fail(BLSGPU_E_HIP, "internal: unknown exception");
    }
    errs[d] = t_err;
  };
  th.reserve(k);
  for (size_t d = 1; d < k; d++) th.emplace_back(body, d);
  const size_t keep_dev = t_devidx;
  const bool keep_nested = t_nested;
  body(0);
  t_devidx = keep_dev;
  t_nested = keep_nested;
  for (auto& t : th) t.join();
  for (size_t d = 0; d < k; d++)
    if (rcs[d]) {
      t_err = errs[d];
      return rcs[d];
    }
  return 0;
}
struct NestedScope {     // the calling thread's own follow-up calls (fold, final verify) stay on device 0 and do not shard again
  bool keep;
  NestedScope() : keep(t_nested) { t_nested = true; }
  ~NestedScope() { t_nested = keep; }
};

// ---- shared device pipelines (stream-ordered; caller holds the context mutex) ------------------------

// items per pass of the two-kernel Miller loop (0: the one-kernel loop); one full machine round of lane pairs by default
size_t miller_chunk_items() { return knobs().miller_v1 ? 0 : (size_t)knobs().miller_chunk; }
size_t lanes_for(size_t items) { return (2 * items + BLS_BLOCK - 1) / BLS_BLOCK * BLS_BLOCK; }
// Row stride (in words) of the line workspace and the value store for that many lanes: NOT a power of two -- consecutive rows of
// a lane are a stride apart, and with 2^k-byte strides the 70 rows a wave touches per step camp on the same HBM channels
// (measured on the 262,144-lane chunks of config 4: BLSGPU_ROW_PAD=0 restores the bare stride for A/B runs)
size_t row_stride(size_t lanes) { return lanes + (size_t)knobs().row_pad; }
// the context's line workspace; 0 on success, non-zero (and no error recorded) when the device has no room for it
int lines_reserve(Ctx* c, size_t bytes) {
  if (bytes <= c->lines_cap) return 0;
  auto note = [&](const char* why) {      // the caller falls back to a slower plan: say so once per process instead of changing plans silently (advisor r3)
    static std::atomic<bool> said{false};
    if (!said.exchange(true)) fprintf(stderr, "libblsgpu: no room for a %zu MiB line workspace (%s): falling back to the one-kernel Miller loops\n", bytes >> 20, why);
  };
  if (hipStreamSynchronize(c->stream) != hipSuccess) {
    (void)hipGetLastError();
    note("stream error");
    return 1;
  }
  if (c->lines_ws) (void)hipFree(c->lines_ws);
  c->lines_ws = nullptr;
  c->lines_cap = 0;
  if (hipMalloc((void**)&c->lines_ws, bytes) != hipSuccess) {
    (void)hipGetLastError();
    c->lines_ws = nullptr;
    note("hipMalloc failed");
    return 1;
  }
  c->lines_cap = bytes;
  return 0;
}
// end of a call (Lease::~Lease, streams idle): a line workspace above BLSGPU_WS_KEEP_MB (default 4 GiB; the 65,536-item chunk of a
// batch needs 2.5 GB, the 262,144-pair plan of an aggregate 2.6 GB) does not stay with the pooled context for the life of the process
void trim_workspaces(Ctx* c) {
  if (c->lines_ws && (c->lines_cap >> 20) > (size_t)knobs().ws_keep_mb) {
    (void)hipFree(c->lines_ws);
    c->lines_ws = nullptr;
    c->lines_cap = 0;
  }
}

// the final exponentiation and verdict of items [first, first + cnt) of the Fp12 workspace d_f (stride n), two lanes per item, with
// the context's line workspace as the value store (FX_STORE_WORDS rows of row_stride(lanes_for(cnt)) words, reserved by the caller);
// items whose status is not BLS_OK are skipped.  seg: in segments, the compressed squarings of each a^x on four lanes per item at four
// waves per SIMD (k_cyc_run4) between them; otherwise one kernel (k_finalexp2s).
void launch_finalexp_chunk(Ctx* c, size_t n, size_t first, size_t cnt, const uint32_t* d_f, int32_t* d_status, bool seg) {
  const size_t nlanes = lanes_for(cnt), lanes = row_stride(nlanes);
  const dim3 grid((unsigned)(nlanes / BLS_BLOCK));
  if (seg) {
    const dim3 grid4(blocks_for(4 * cnt));
    for (int s = 0; s <= 5; s++) {
      KL(KID_FINALEXP, k_finalexp_seg, grid, dim3(BLS_BLOCK), s, n, first, cnt, d_f, c->lines_ws, lanes, d_status);
      if (s < 5) KL(KID_CYCRUN, k_cyc_run4, grid4, dim3(BLS_BLOCK), cnt, c->lines_ws, lanes, (const int32_t*)d_status, first);
    }
  } else {
    KL(KID_FINALEXP, k_finalexp2s, grid, dim3(BLS_BLOCK), n, first, cnt, d_f, c->lines_ws, lanes, d_status);
  }
}

// Which kernels the two-pair pairing check of n items runs on -- the ONE statement of the rule; every plan that depends on it asks here.
enum PairPath {
  PATH_ENGINE,      // up to BLSGPU_WIDE_MAX items (and BLSGPU_COOP_MAX): the row-wide engine, one 256-thread workgroup per item
  PATH_ONE_WAVE,    // up to BLSGPU_COOP_MAX items: one wave per item (coop.cuh)
  PATH_LANE_SPLIT   // above: two lanes per item (tower_split.cuh)
};
PairPath pair_path(size_t n) {
  if (n > coop_max_items()) return PATH_LANE_SPLIT;
  return n <= wide_max_items() ? PATH_ENGINE : PATH_ONE_WAVE;
}
// the lane-split path runs its Miller loop in two kernels, chunk after chunk (else: the one-kernel loop, which reads no table)
bool lane_split_chunked() { return miller_chunk_items() != 0; }
// does a call of n items run kernels that can take a G2 member from precomputed rows?  The engine walks every point, and so does
// the one-kernel Miller loop of the lane-split path.
bool pair_path_reads_rows(size_t n) {
  const PairPath path = pair_path(n);
  return path == PATH_ONE_WAVE || (path == PATH_LANE_SPLIT && lane_split_chunked());
}

// A G2 member taken from precomputed Miller-loop rows instead of being walked: item i's member is entry of[i] of the table `rows`.
struct TabledG2 {
  const uint32_t* rows = nullptr;   // null: the member is walked from the record
  const uint32_t* of = nullptr;     // device, one entry index per item
};
// What run_pairing2 knows about the G2 members of its two pairs beyond the records.  The launchers take the first that
// applies of: `key` (only with fixed_g2 = 2), then with fixed_g2 = 0 `msg` (one-wave) or `shared` (lane-split), then `both`; with none, two
// general pairs (or one, with fixed_g2).  So `key` may stand beside `shared` or `msg` -- fixed_g2 says which implementation the call
// is for -- and a role that the path taken does not read is ignored: a caller sets the role of the path it wrote its records for,
// asking pair_path(n).
struct PairTables {
  // the second pair's G2 member is a constant with precomputed lines: 0 = none, 1 = -g2, 2 = -[c] g2 (csrc/g2neg_lines.cuh).  Every path.
  int fixed_g2 = 0;
  // fixed_g2 = 0, shared-message verify (verify_shared.cuh): PAIR 1's G2 member is the point of item i's group shared.of[i], its
  // normalised rows in shared.rows; the records carry the SIGNATURE'S PAIR FIRST.  Read on the lane-split path only, where the chunk's
  // line launch is one k_lines2s_shared instead of two k_lines2s.
  TabledG2 shared;
  // fixed_g2 = 2, registered key sets with line tables (keyset.cuh): PAIR 0's G2 member is entry key.of[i] of the set; records in
  // their usual order.  Read on the lane-split path (k_lines2s_keyed reads both rows and walks nothing) and on the one-wave path
  // (k_pairing_coop_keyed, coop.cuh coop_miller2_tables); the engine and its BLSGPU_WIDE_MODE=1 branch ignore it.
  TabledG2 key;
  // fixed_g2 = 0, registered message sets with rows, Bls12381G2Impl (coop_rows.cuh): PAIR 0's G2 member is entry msg.of[i] of the set;
  // records in their usual pair order.  Read on the one-wave path only (k_pairing_coop_rows reads the rows while it walks the
  // signature); the lane-split path takes such a set as `shared`.
  TabledG2 msg;
  // fixed_g2 = 0, Bls12381G2Impl signcryption shares by key index (signcrypt.cuh): BOTH G2 members are entries of one table, pair 0's at
  // both.of[i] and pair 1's at both.of[n + i]; records in their usual order.  Read on the one-wave path (k_pairing_coop_tables2) and on
  // the lane-split path (k_lines2s_tables2 as the chunk's line launch): above the engine's range nothing is walked.
  TabledG2 both;
};
// no tabled member: both pairs as the records give them, the second one's G2 member the constant that fixed_g2 names
PairTables pairs_walked(int fixed_g2) {
  PairTables t;
  t.fixed_g2 = fixed_g2;
  return t;
}

// The only launch of the one-wave family: the kernel the descriptor names, one wave per item.  d_easy = null: final exponentiation and
// verdict into d_status; else the easy-part value of item i into d_easy + i * WIDE_EASY_WORDS (the BLSGPU_WIDE_MODE=1 branch, the hooks).
void launch_pairing_coop(Ctx* c, size_t n, const uint32_t* d_pairs, int32_t* d_status, const PairTables& t, uint32_t* d_easy = nullptr) {
  const dim3 grid((unsigned)n), block(BLS_BLOCK);
  if (t.fixed_g2 == 2 && t.key.rows)
    KL(KID_PAIRING_COOP_KEYED, k_pairing_coop_keyed, grid, block, n, d_pairs, d_status, t.key.rows, t.key.of, d_easy);
  else if (t.fixed_g2 == 0 && t.msg.rows)
    KL(KID_PAIRING_COOP_ROWS, k_pairing_coop_rows, grid, block, n, d_pairs, d_status, t.msg.rows, t.msg.of, d_easy);
  else if (t.fixed_g2 == 0 && t.both.rows)
    KL(KID_PAIRING_COOP_TABLES2, k_pairing_coop_tables2, grid, block, n, d_pairs, d_status, t.both.rows, t.both.of, t.both.of + n, d_easy);
  else if (d_easy)
    KL(KID_PAIRING_COOP, k_pairing_coop_easy, grid, block, n, d_pairs, (const int32_t*)d_status, t.fixed_g2, d_easy);
  else
    KL(KID_PAIRING_COOP, k_pairing_coop, grid, block, n, d_pairs, d_status, t.fixed_g2);
}
// Do the merged line values of a chunk need pass 1's plain lines of pair 0 behind them (two general pairs: k_lines2s in two passes)?
bool lines_two_pass(const PairTables& t) { return !t.fixed_g2 && !t.shared.rows && !t.both.rows; }
// The only line launch of a lane-split chunk: the merged line values of items [first, first + cnt) into the context's line workspace,
// rows `lanes` words apart (row_stride(lanes_for(cnt))), by the kernel the descriptor names.
void launch_lines2s(Ctx* c, size_t n, size_t first, size_t cnt, const uint32_t* d_pairs, const int32_t* d_status, const PairTables& t, size_t lanes) {
  const dim3 grid((unsigned)(lanes_for(cnt) / BLS_BLOCK)), block(BLS_BLOCK);
  uint32_t* lines3 = c->lines_ws + (size_t)MILLER_ENTRIES * LINE5_WORDS * lanes;
  if (t.fixed_g2 == 2 && t.key.rows) {
    KL(KID_LINES_KEYED, k_lines2s_keyed, grid, block, n, first, cnt, d_pairs, d_status, c->lines_ws, lanes, t.key.rows, t.key.of);
  } else if (t.fixed_g2) {
    KL(KID_LINES, k_lines2s, grid, block, n, first, cnt, d_pairs, d_status, c->lines_ws, lines3, lanes, t.fixed_g2, 0);
  } else if (t.shared.rows) {
    KL(KID_LINES, k_lines2s_shared, grid, block, n, first, cnt, d_pairs, d_status, c->lines_ws, lanes, t.shared.rows, t.shared.of);
  } else if (t.both.rows) {
    KL(KID_LINES_TABLES2, k_lines2s_tables2, grid, block, n, first, cnt, d_pairs, d_status, c->lines_ws, lanes, t.both.rows, t.both.of, t.both.of + n);
  } else {
    KL(KID_LINES, k_lines2s, grid, block, n, first, cnt, d_pairs, d_status, c->lines_ws, lines3, lanes, 0, 1);
    KL(KID_LINES, k_lines2s, grid, block, n, first, cnt, d_pairs, d_status, c->lines_ws, lines3, lanes, 0, 2);
  }
}

// the two-pair pairing check of every item whose status is still BLS_OK: status <- OK / INVALID_SIGNATURE
int run_pairing2(Ctx* c, size_t n, uint32_t* d_pairs, uint32_t* d_f, int32_t* d_status, const PairTables& t) {
  const int fixed_g2 = t.fixed_g2;
  const PairPath path = pair_path(n);
  if (path == PATH_ENGINE) {
    // single verifications and the one-verdict tails on the row-wide engine (csrc/wide_engine.cuh): one 256-thread workgroup
    // per item runs line coefficients, Miller loop, final exponentiation and verdict as one table program.
    // BLSGPU_WIDE_MODE=1: only the hard part of the final exponentiation on the engine, Miller loop + easy part per wave.
    if (knobs().wide_mode == 1) {
      uint32_t* d_easy = (uint32_t*)arena_take(c, (size_t)WIDE_EASY_WORDS * 4 * n);   // arena_reserve keeps 1 MiB of headroom: 768 B per item
      if (!d_easy) return fail(BLSGPU_E_HIP, "internal: arena too small");
      launch_pairing_coop(c, n, d_pairs, d_status, pairs_walked(fixed_g2), d_easy);
      KL(KID_WIDE, k_finalexp_wide, dim3((unsigned)n), dim3(WIDE_ENGINE_BLOCK), n, (const uint32_t*)d_easy, d_status);
    } else {
      KL(KID_WIDE, k_pairing_wide, dim3((unsigned)n), dim3(WIDE_ENGINE_BLOCK), n, (const uint32_t*)d_pairs, d_status, fixed_g2);
    }
  } else if (path == PATH_ONE_WAVE) {  // small batches: one wave per item
    launch_pairing_coop(c, n, d_pairs, d_status, t);
  } else {                      // two lanes per item (tower_split.cuh)
    // The Miller loop in two kernels (kernels.cuh k_lines2s / k_millerf2s), a chunk of at most miller_chunk_items() items at a
    // time: the chunk's merged line values pass through the context's line workspace.  BLSGPU_MILLER_V1=1, or no memory for
    // that workspace: the one-kernel loop of rounds 1 and 2.
    // BLSGPU_FINALEXP_SEG=1: the final exponentiation in six segments with the 63 compressed squarings of every a^x on FOUR lanes per
    // item at four waves per SIMD between them (k_cyc_run4).  Measured and not adopted (profiles/r03_pmc_finalexp_segments_cycrun4.json):
    // the squarings take 5.27 ms instead of ~5.6 ms inside k_finalexp2s, the six segments 4.28 ms: 9.55 ms against 9.49 ms for the one kernel.
    const bool finalexp_seg = knobs().finalexp_seg != 0;
    const bool finalexp_v1 = knobs().finalexp_v1 != 0;   // A/B: the one-kernel final exponentiation of rounds 1 and 2
    const size_t chunk = n < miller_chunk_items() ? n : miller_chunk_items();
    const size_t words_per_lane = (size_t)MILLER_ENTRIES * (LINE5_WORDS + (lines_two_pass(t) ? LINE3_WORDS_H : 0));   // two general pairs: pair 0's plain lines too
    if (lane_split_chunked() && lines_reserve(c, words_per_lane * 4 * row_stride(lanes_for(chunk))) == 0) {
      for (size_t first = 0; first < n; first += chunk) {
        const size_t cnt = n - first < chunk ? n - first : chunk;
        const size_t nlanes = lanes_for(cnt), lanes = row_stride(nlanes);       // `lanes` below: the row stride the kernels index with
        const dim3 grid((unsigned)(nlanes / BLS_BLOCK));
        launch_lines2s(c, n, first, cnt, d_pairs, d_status, t, lanes);
        KL(KID_MILLER2, k_millerf2s, grid, dim3(BLS_BLOCK), n, first, cnt, (const int32_t*)d_status, (const uint32_t*)c->lines_ws, lanes, d_f);
        // the chunk's line values are consumed: the same memory is the value store of the final exponentiation (3.4 KB per lane)
        if (!finalexp_v1) launch_finalexp_chunk(c, n, first, cnt, d_f, d_status, finalexp_seg);
      }
      if (finalexp_v1) KL(KID_FINALEXP_V1, k_finalexps, dim3(blocks_for(2 * n)), dim3(BLS_BLOCK), n, d_f, d_status);
    } else {
      KL(KID_MILLER2_V1, k_miller2s, dim3(blocks_for(2 * n)), dim3(BLS_BLOCK), n, d_pairs, d_status, d_f, fixed_g2);
      KL(KID_FINALEXP_V1, k_finalexps, dim3(blocks_for(2 * n)), dim3(BLS_BLOCK), n, d_f, d_status);
    }
  }
  HIPCK(hipGetLastError());
  return 0;
}

// ---- what the self-test hooks of the two-pair kernels share
// A hook's records (n items of `rec` words, item after item) in the workspace layout -- word w of item i at ws[w * n + i] -- staged with the
// statuses and, if the hook has one, an index array of of_words words, in that order.  The stream is synchronised before the
// transposed copy leaves scope (pageable memory).
struct DebugStaged {
  const uint32_t* pairs;
  int32_t* status;
  const uint32_t* of;      // null: no index array
};
static int debug_stage(Ctx* c, const int32_t* in, size_t rec, size_t n, const int32_t* status, DebugStaged* s, const uint32_t* of = nullptr, size_t of_words = 0) {
  std::vector<uint32_t> h(rec * n);
  for (size_t i = 0; i < n; i++)
    for (size_t w = 0; w < rec; w++) h[w * n + i] = (uint32_t)in[i * rec + w];
  const void *d_in, *d_st, *d_of = nullptr;
  int rc;
  if ((rc = stage_in(c, h.data(), rec * 4 * n, &d_in))) return rc;
  if ((rc = stage_in(c, status, 4 * n, &d_st))) return rc;
  if (of && (rc = stage_in(c, of, 4 * of_words, &d_of))) return rc;
  HIPCK(hipStreamSynchronize(c->stream));
  *s = {(const uint32_t*)d_in, (int32_t*)d_st, (const uint32_t*)d_of};
  return 0;
}
// The body of the one-wave hooks, after their argument checks, arena reservation and debug_stage: the kernel that `t` names runs on
// the staged records through launch_pairing_coop -- the launch of run_pairing2, by construction.  Mode 1: the verdicts into status.
// Mode 0: the easy-part values into out_f12, from the engine's value layout (value v = 2 * (power of w) + component, sixteen words
// each; an item that was skipped keeps the sentinel) to tower order, fourteen limbs each.
static int debug_pairing_coop(Ctx* c, int mode, const PairTables& t, const DebugStaged& s, size_t n, int32_t* status, int32_t* out_f12) {
  if (mode == 1) {
    launch_pairing_coop(c, n, s.pairs, s.status, t);
    HIPCK(hipGetLastError());
    return copy_out_and_sync(c, status, s.status, 4 * n);
  }
  uint32_t* d_easy = (uint32_t*)arena_take(c, (size_t)WIDE_EASY_WORDS * 4 * n);
  if (!d_easy) return fail(BLSGPU_E_HIP, "internal: arena too small");
  HIPCK(hipMemsetAsync(d_easy, BLSGPU_DEBUG_COOP_SENTINEL & 0xff, (size_t)WIDE_EASY_WORDS * 4 * n, c->stream));
  launch_pairing_coop(c, n, s.pairs, s.status, t, d_easy);
  HIPCK(hipGetLastError());
  std::vector<uint32_t> e((size_t)WIDE_EASY_WORDS * n);
  HIPCK(hipMemcpyAsync(e.data(), d_easy, e.size() * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCK(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < n; i++)
    for (size_t k = 0; k < 6; k++) {
      const size_t pw = k < 3 ? 2 * k : 2 * (k - 3) + 1;
      for (size_t comp = 0; comp < 2; comp++)
        for (size_t l = 0; l < FP_NL; l++) out_f12[i * WS_F_WORDS + (2 * k + comp) * FP_NL + l] = (int32_t)e[i * WIDE_EASY_WORDS + (2 * pw + comp) * 16 + l];
    }
  SYNC_FLUSH(c);
  return 0;
}

// The chunk loop of the line-kernel hooks: `total` items in chunks of `chunk` (0: miller_chunk_items(), or all of them).  The line
// workspace is filled with the sentinel byte before every chunk, launch(first, cnt, lanes) runs the chunk's line launch, and the
// workspace is read back whole before the next one.  The chunk's output rows -- rows[(e * out_words + w) * lanes + t], word w = 14 *
// (coefficient number) + limb, lane t = 2 * item + component -- go to `out` item after item; *stray counts the words written on lanes
// beyond the chunk's items and behind the output rows.  two_pass: the lines3 rows of the two-pass forms lie behind them, where pass 1
// writes the lanes of its live items, nothing for an item it skips and nothing beyond the chunk's items.
template <class L>
static int debug_line_chunks(Ctx* c, size_t total, size_t chunk, size_t out_words, bool two_pass, const int32_t* status, int32_t* out, uint64_t* stray, L&& launch) {
  const size_t E = MILLER_ENTRIES;
  const uint32_t sentinel = (uint32_t)BLSGPU_DEBUG_COOP_SENTINEL;
  size_t per = chunk ? chunk : miller_chunk_items() ? miller_chunk_items() : total;
  if (per > total) per = total;
  const size_t ws_words = E * (LINE5_WORDS + LINE3_WORDS_H) * row_stride(lanes_for(per));
  if (lines_reserve(c, ws_words * 4)) return fail(BLSGPU_E_HIP, "no room for the line workspace");
  std::vector<uint32_t> rows(ws_words);                 // the whole workspace: the output rows, pass 1's lines3 rows, the rest
  for (size_t first = 0; first < total; first += per) {
    const size_t cnt = total - first < per ? total - first : per;
    const size_t lanes = row_stride(lanes_for(cnt)), nrows = E * out_words;
    HIPCK(hipMemsetAsync(c->lines_ws, BLSGPU_DEBUG_COOP_SENTINEL & 0xff, ws_words * 4, c->stream));
    launch(first, cnt, lanes);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(rows.data(), c->lines_ws, ws_words * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    size_t at = nrows * lanes;
    if (two_pass)
      for (size_t r = 0; r < E * LINE3_WORDS_H; r++, at += lanes)
        for (size_t t = 0; t < lanes; t++) {
          const size_t j = t >> 1;
          const bool live = j < cnt && status[first + j] == 0;      // (BLS_OK = 0: both kernels skip on a non-zero entry)
          if (!live && rows[at + t] != sentinel) ++*stray;
        }
    for (; at < ws_words; at++)
      if (rows[at] != sentinel) ++*stray;
    for (size_t r = 0; r < nrows; r++) {
      const uint32_t* row = rows.data() + r * lanes;
      const size_t e = r / out_words, w = r % out_words, kk = w / FP_NL, l = w % FP_NL;
      for (size_t j = 0; j < cnt; j++)
        for (size_t comp = 0; comp < 2; comp++)
          out[((((first + j) * E + e) * (out_words / FP_NL) + kk) * 2 + comp) * FP_NL + l] = (int32_t)row[2 * j + comp];
      for (size_t t = 2 * cnt; t < lanes; t++)
        if (row[t] != sentinel) ++*stray;
    }
  }
  SYNC_FLUSH(c);
  return 0;
}

// the context's side stream (created on first use) starts where the main stream is now
// which: bit 0 = mark the fork point on the main stream, bit 1 = make the side streams wait for it (a caller may enqueue the
// main stream's next kernel between the two: the host's enqueue time of the side work then is off that kernel's path)
int side_fork(Ctx* c, int which = 3) {
  if (!c->side) {
    HIPCK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    HIPCK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    HIPCK(hipStreamCreateWithFlags(&c->side2, hipStreamNonBlocking));
    HIPCK(hipEventCreateWithFlags(&c->ev_join2, hipEventDisableTiming));
  }
  if (which & 1) HIPCK(hipEventRecord(c->ev_fork, c->stream));
  if (which & 2) {
    HIPCK(hipStreamWaitEvent(c->side, c->ev_fork, 0));
    HIPCK(hipStreamWaitEvent(c->side2, c->ev_fork, 0));
  }
  return 0;
}

// hash-to-G1 of a few messages on `stream`: one workgroup per message with the cofactor clearing on the engine while every
// message gets its own CU (up to 128 messages), one wave per message beyond that.  flags: bit 0 = every item hashes message 0.
void launch_hash_g1_small(hipStream_t stream, size_t n, const uint8_t* d_msgs, const uint64_t* d_offs, int flags, const dst_arg& dst, uint8_t* d_out,
                          uint32_t* d_rec) {
  if (n <= 128 && hash_phase_stop() == 0)     // measured (tools/dbg/small.py): at 256 items the pre-workgroups compete for the CUs and the one-wave hash wins
    hipLaunchKernelGGL(k_hash_to_g1_engine<false>, dim3((unsigned)n), dim3(WIDE_ENGINE_BLOCK), 0, stream, n, d_msgs, d_offs, flags, dst, d_out, d_rec);
  else
    hipLaunchKernelGGL(k_hash_to_g1_wide<false>, dim3((unsigned)n), dim3(BLS_BLOCK), 0, stream, n, d_msgs, d_offs, flags | hash_phase_stop() << 8, dst, d_out, d_rec);
}

// hash-to-G2 of a few messages on `stream` (RAW_PROJ out): one workgroup per message on the engine up to 128 messages; beyond
// that one WAVE per message for the maps and one workgroup per message for the engine program (d_pts: 768 bytes of scratch per
// message), or -- without scratch -- two lanes per message for the maps and one workgroup per point for the clearing.
bool launch_hash_g2_small(hipStream_t stream, size_t n, const uint8_t* d_msgs, const uint64_t* d_offs, int flags, const dst_arg& dst, uint8_t* d_out,
                          uint32_t* d_pts = nullptr, uint32_t* d_rec = nullptr) {
  // d_rec: the records of a cut check (WREC_Q0 of item i <- H(m_i)); true when they were written -- the lane-pair form only
  // fills d_out and the caller converts (k_prepare_keys part 4)
  if (n <= 128 && hash_phase_stop() == 0) {
    hipLaunchKernelGGL(k_hash_to_g2_engine<false>, dim3((unsigned)n), dim3(WIDE_ENGINE_BLOCK), 0, stream, n, d_msgs, d_offs, flags, dst, d_out, d_rec);
    return d_rec != nullptr;
  }
  if (d_pts && hash_phase_stop() == 0) {
    hipLaunchKernelGGL(k_hash_to_g2_maps<false>, dim3((unsigned)n), dim3(BLS_BLOCK), 0, stream, n, d_msgs, d_offs, flags, dst, d_pts);
    hipLaunchKernelGGL(k_g2_hash_tail_wide, dim3((unsigned)n), dim3(WIDE_ENGINE_BLOCK), 0, stream, n, (const uint32_t*)d_pts, d_out, d_rec);
    return d_rec != nullptr;
  }
  hipLaunchKernelGGL(k_hash_to_g2<false>, dim3(blocks_for(2 * n)), dim3(BLS_BLOCK), 0, stream, n, d_msgs, d_offs, dst, d_out, 3);
  hipLaunchKernelGGL(k_g2_clear_wide, dim3((unsigned)n), dim3(WIDE_ENGINE_BLOCK), 0, stream, n, d_out);
  return false;
}

// The hand-over flags of the kernels whose workgroups pass data to each other inside one launch (kernels.cuh k_pairing_stream,
// k_pairing_post2): a buffer of the context that those kernels alone write, and a value per launch that no earlier launch used.
static int stream_epoch_next(Ctx* c) {
  const size_t fb = (size_t)WPOST2_MAX_ITEMS * WSTREAM_FLAGS * 4;
  if (!c->stream_flags) {
    HIPCK(hipMalloc((void**)&c->stream_flags, fb));
    c->stream_epoch = 0;
  }
  if (c->stream_epoch == 0 || c->stream_epoch == 0xffffffffu) {      // first use, or the counter is about to repeat itself
    HIPCK(hipMemsetAsync(c->stream_flags, 0, fb, c->stream));
    c->stream_epoch = 0;
  }
  c->stream_epoch++;
  return 0;
}
// the late part of the cut check alone (its lines are in the record): for up to WPOST2_MAX_ITEMS items with the Miller loop on two
// workgroups per item (kernels.cuh k_pairing_post2)
int launch_post(Ctx* c, size_t n, uint32_t* d_rec, int32_t* d_status) {
  if (knobs().post_split >= 2 && n <= WPOST2_MAX_ITEMS) {
    int rc = stream_epoch_next(c);
    if (rc) return rc;
    // three workgroups per item while every item can have three CUs at once, two up to WPOST2_MAX_ITEMS
    const unsigned parts = (knobs().post_split >= 3 && n <= WSTREAM_MAX_ITEMS) ? 3u : 2u;
    KL(KID_PAIRING_POST, k_pairing_post2, dim3((unsigned)n, parts), dim3(WIDE_ENGINE_BLOCK), n, d_rec, d_status, c->stream_flags, c->stream_epoch);
    return 0;
  }
  KL(KID_PAIRING_POST, k_pairing_post, dim3((unsigned)n), dim3(WIDE_ENGINE_BLOCK), n, (const uint32_t*)d_rec, d_status);
  return 0;
}
// Pair 0's lines and the late part of the cut check: ONE launch in which the lines travel from one workgroup to two others while
// the Miller loop already runs there (kernels.cuh k_pairing_stream) -- for up to WSTREAM_MAX_ITEMS checks whose lines have nothing
// to hide behind; otherwise the launches k_pairing_pre (part 0), then the late part as above.
int launch_lines_and_post(Ctx* c, size_t n, uint32_t* d_rec, int32_t* d_status) {
  if (knobs().stream_lines != 0 && n <= WSTREAM_MAX_ITEMS) {
    int rc = stream_epoch_next(c);
    if (rc) return rc;
    KL(KID_PAIRING_POST, k_pairing_stream, dim3((unsigned)n, 3), dim3(WIDE_ENGINE_BLOCK), n, d_rec, d_status, c->stream_flags, c->stream_epoch);
    return 0;
  }
  KL(KID_PAIRING_PRE, k_pairing_pre, dim3((unsigned)n, 1), dim3(WIDE_ENGINE_BLOCK), n, d_rec, (const int32_t*)d_status, 0, 0);
  return launch_post(c, n, d_rec, d_status);
}

// one core_verify per item: statuses end up in d_status (device)
int run_verify_items(Ctx* c, int sg, int aug, const uint8_t* d_pks, const uint8_t* d_sigs, int fmt, const uint8_t* d_msgs,
                     const uint64_t* d_offs, int single_msg, const dst_arg& dst, size_t n, uint32_t* d_pairs, uint32_t* d_f,
                     int32_t* d_status, int pre_status = 0, const TabledG2& key = {}) {
  // key: the keys are entries of a registered set with line tables (PairTables::key); the two plans above BLSGPU_WIDE_MAX items
  // pass it on
  if (n == 0) return 0;
  const PairPath path = pair_path(n);
  if (sg == 1 && aug == 0 && !pre_status && path == PATH_ENGINE) {
    // Single verifications of Bls12381G1Impl without a key prefix, cut where the inputs allow (csrc/kernels.cuh k_pairing_pre /
    // k_pairing_post): this stream hashes the messages (row-wide field type) while the side stream checks keys and
    // signatures, derives every key's line coefficients and runs the Miller loop of the (signature, -g2) pair -- two
    // workgroups per item, none of which needs H(m); what is left after the join is the Miller loop of (H(m), key) over
    // ready-made lines and the final exponentiation.
    uint32_t* d_rec = (uint32_t*)arena_take(c, (size_t)WREC_WORDS * 4 * n);
    if (!d_rec) return fail(BLSGPU_E_HIP, "internal: arena too small");
    // the LONG chain -- staging copy, hash, then the rest of the check -- stays on this stream and is enqueued first, so that
    // neither an event hand-over (~20 us each) nor the host's enqueue time of the side work sits on the critical path; the
    // side stream does what finishes early anyway
    int rc = side_fork(c, 1);
    if (rc) return rc;
    prof_pre(c, KID_HASH);
    launch_hash_g1_small(c->stream, n, d_msgs, d_offs, single_msg, dst, (uint8_t*)nullptr, d_rec);
    prof_post(c);
    if ((rc = side_fork(c, 2))) {
      (void)hipStreamSynchronize(c->stream);
      return rc;
    }
    hipLaunchKernelGGL(k_prepare_keys<1>, dim3(blocks_for(n)), dim3(BLS_BLOCK), 0, c->side, n, d_pks, d_sigs, (const uint8_t*)nullptr, fmt, 3, d_rec, d_status);
    hipLaunchKernelGGL(k_pairing_pre, dim3((unsigned)n, 2), dim3(WIDE_ENGINE_BLOCK), 0, c->side, n, d_rec, (const int32_t*)d_status, 0, 1);
    hipError_t e1 = hipGetLastError(), e2 = hipEventRecord(c->ev_join, c->side);
    hipError_t e3 = hipStreamWaitEvent(c->stream, c->ev_join, 0);      // also when something failed: the side kernels read the arena
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
      (void)hipStreamSynchronize(c->side);
      return fail(BLSGPU_E_HIP, "side-stream launch failed");
    }
    if ((rc = launch_post(c, n, d_rec, d_status))) {
      (void)hipStreamSynchronize(c->side);
      return rc;
    }
    HIPCK(hipGetLastError());
    return 0;
  }
  if (sg == 2 && aug == 0 && !pre_status && (!single_msg || n == 1) && path == PATH_ENGINE) {
    // The same cut for Bls12381G2Impl, pairs (key, H(m)) (-g1, signature): this stream carries the long chain -- the hash to G2
    // (row-wide maps, cofactor clearing on the engine), H(m)'s record and lines -- and is enqueued first; the side stream
    // checks keys and signatures and runs the signature's lines and Miller function; after the join the Miller function of
    // (key, H(m)) and the rest.
    uint32_t* d_rec = (uint32_t*)arena_take(c, (size_t)WREC_WORDS * 4 * n);
    uint8_t* d_hashes = (uint8_t*)arena_take(c, 288 * n);
    uint32_t* d_maps = n > 128 ? (uint32_t*)arena_take(c, 768 * n) : nullptr;      // nullptr (arena full): the lane-pair maps
    if (!d_rec || !d_hashes) return fail(BLSGPU_E_HIP, "internal: arena too small");
    int rc = side_fork(c, 1);
    if (rc) return rc;
    prof_pre(c, KID_HASH);
    const bool rec_done = launch_hash_g2_small(c->stream, n, d_msgs, d_offs, 0, dst, d_hashes, d_maps, d_rec);
    prof_post(c);
    if (!rec_done)
      KL(KID_PREPARE, k_prepare_keys<2>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)nullptr, (const uint8_t*)nullptr, (const uint8_t*)d_hashes, 0, 4,
         d_rec, d_status);
    if ((rc = side_fork(c, 2))) {
      (void)hipStreamSynchronize(c->stream);
      return rc;
    }
    hipLaunchKernelGGL(k_prepare_keys<2>, dim3(blocks_for(n)), dim3(BLS_BLOCK), 0, c->side, n, d_pks, d_sigs, (const uint8_t*)nullptr, fmt, 3, d_rec, d_status);
    // the lines of H(m) skip items that failed the identity checks: this stream waits for the statuses written just above
    hipError_t e1 = hipGetLastError(), e2 = hipEventRecord(c->ev_join2, c->side);
    hipLaunchKernelGGL(k_pairing_pre, dim3((unsigned)n, 1), dim3(WIDE_ENGINE_BLOCK), 0, c->side, n, d_rec, (const int32_t*)d_status, 2, 2);
    hipError_t e3 = hipGetLastError(), e4 = hipEventRecord(c->ev_join, c->side);
    hipError_t e5 = hipStreamWaitEvent(c->stream, c->ev_join2, 0);
    hipError_t e6 = hipStreamWaitEvent(c->stream, c->ev_join, 0);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess || e5 != hipSuccess || e6 != hipSuccess) {
      (void)hipStreamSynchronize(c->side);
      return fail(BLSGPU_E_HIP, "side-stream launch failed");
    }
    // H(m)'s lines have nothing left to hide behind (the signature's half on the side stream ended under the hash): they run
    // beside the Miller loop that consumes them
    if ((rc = launch_lines_and_post(c, n, d_rec, d_status))) {
      (void)hipStreamSynchronize(c->side);
      return rc;
    }
    HIPCK(hipGetLastError());
    return 0;
  }
  if (sg == 1 && aug == 0 && !pre_status && path == PATH_ONE_WAVE && n <= 1024 && wide_max_items() > 0) {
    // 513 to 1,024 items (measured: 4.1 / 4.6 ms at 768 / 1,024 against 4.8 / 5.1; at 2,048 the two-lane hash wins): the wave-cooperative pairing, but with the one-wave row-wide hash (0.74 ms while every
    // message has a SIMD to itself, against 1.6 ms for the two-lane hash inside k_prepare) and the shared to-affine inversion after it
    uint8_t* d_hashes = (uint8_t*)arena_take(c, 144 * n);
    if (!d_hashes) return fail(BLSGPU_E_HIP, "internal: arena too small");
    // the hashes stay uncleared (bit 1) and the fixed pair is (sig, -[c] g2) (table 2), as everywhere for this implementation
    KL(KID_HASH, k_hash_to_g1_wide<false>, dim3((unsigned)n), dim3(BLS_BLOCK), n, d_msgs, d_offs, (single_msg & 1) | 2, dst, d_hashes, (uint32_t*)nullptr);
    KL(KID_PREPARE, k_prepare_hashed<1>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_pks, d_sigs, (const uint8_t*)d_hashes, d_pairs, d_status, fmt);
    PairTables t = pairs_walked(2);
    t.key = key;
    return run_pairing2(c, n, d_pairs, d_f, d_status, t);
  }
  // two lanes per item (the two SSWU maps side by side, G2 point arithmetic on the lane-split tower) for both implementations
  // and every batch size (rounds 1-2 used one lane per item for full Bls12381G1Impl batches; see below)
  const int force_lanes = (int)knobs().prepare_lanes;   // A/B aid: 1 or 2 lanes per item in k_prepare<1>
  // two lanes per item also for full Bls12381G1Impl batches since round 3: 1.69 against 1.80 ms at 65,536 items (k_prepare is a one-wave-per-SIMD kernel
  // otherwise, and a lone wave issues a multiply-add every 8.8 cycles where two waves share the pipe at 4.4)
  const int two_lanes = force_lanes == 1 && sg == 1 ? 0 : 1;
  unsigned nb = blocks_for(two_lanes ? 2 * n : n);
  // Bls12381G1Impl: the message points stay UNCLEARED (a third of the hash) and the second pair is (sig, -[c] g2), c = h_eff^-1
  // mod r, whose line table is as constant as -g2's: e(h P', pk) e(sig, -g2) = 1  <=>  e(P', pk) e(sig, -[c] g2) = 1
  // (csrc/g2neg_lines.cuh; fixed_g2 = 2 selects that table)
  if (sg == 1)
    KL(KID_PREPARE, k_prepare<1>, dim3(nb), dim3(BLS_BLOCK), n, d_pks, d_sigs, fmt, aug, d_msgs, d_offs, single_msg, dst, d_pairs, d_status, pre_status, two_lanes | 2);
  else
    KL(KID_PREPARE, k_prepare<2>, dim3(nb), dim3(BLS_BLOCK), n, d_pks, d_sigs, fmt, aug, d_msgs, d_offs, single_msg, dst, d_pairs, d_status, pre_status, two_lanes);
  PairTables t = pairs_walked(sg == 1 ? 2 : 0);
  if (sg == 1) t.key = key;
  return run_pairing2(c, n, d_pairs, d_f, d_status, t);
}

// Pairing products, second form (round 3): the product over the items entry by entry, then one Horner chain (kernels.cuh
// k_line_quad).  Chunks of one machine round of lane pairs walk their G2 points (k_linesp pass 1, or k_linesp4 on four lanes per
// item: the plain line values of every item and entry), k_line_quad multiplies four items' values per entry into an Fp12 value,
// k_f12_fold4 folds each entry's values four to one -- chunk by chunk while a level still fills the machine, then over all chunks'
// values together down to 128 per entry -- the engine takes those in two launches (k_f12_tree_seg) and runs the Horner chain over
// the 68 products (k_f12_horner_wide).  What is
// left beyond whole rounds (< 1,024 items) is a small chunk of its own on the tail stream, beside the others.  Leaves the
// Miller product as item 0 of d_f (*outputs = 1).  *done = false: not applicable (too few items,
// no engine, no memory, BLSGPU_PRODUCT_TREE=0) -- the caller falls back to the accumulator kernels.
// last_mode: what item mm - 1 is.  0: an item like the others.  1 / 2: (P, -g2) / (P, -[c] g2), the signature's pair of an
// aggregate verification of Bls12381G1Impl: its line values come from the fixed argument's table (k_lines_fixed), no point walk.
// 3: the signature's pair of Bls12381G2Impl, a general pair.  The pairs proper of an aggregate are counts like 32,768 or 65,536, and
// the line kernels have cliffs exactly there (the 1,025th wave puts two waves on one SIMD, which then take 1.7 times as long; the
// 2,049th runs alone after the others): in modes 1 - 3 the signature's pair is a one-item chunk of its own on the tail stream.
int run_miller_product_tree(Ctx* c, size_t mm, size_t stride, uint32_t* d_pairs, int32_t* d_bad, uint32_t* d_f, size_t* outputs, bool* done, int last_mode) {
  *done = false;
  const int enabled = (int)knobs().product_tree;
  const long local_env = knobs().tree_local;
  const long lines4_env = knobs().lines4_max;   // A/B: 0 = the two-lane line kernel everywhere
  if (!enabled || mm < 64 || !miller_chunk_items() || !(wide_max_items() > 0 && coop_max_items() > 0)) return 0;
  const size_t round = 65536, E = MILLER_ENTRIES;
  const size_t LOCAL = local_env > 16 ? (size_t)local_env : 1024;    // 68 x 1,024 lane pairs: one machine round
  // The line kernel of a chunk.  Four lanes per item (k_linesp4: the doubling step shared by two lane pairs, six multiplier passes
  // on the critical path instead of eleven) while its waves have a SIMD each (16,384 items = 1,024 waves: 0.75 ms against 1.1);
  // two lanes per item beyond (1.2 ms up to 32,768 items = 1,024 waves, 2.05 ms up to 65,536 = two waves per SIMD; the four-lane
  // kernel with two waves per SIMD takes 1.4 ms).  Measured, tools/dbg/r3_agg5.sh.
  const size_t lines4_max = lines4_env >= 0 ? (size_t)lines4_env : 16384;
  // the signature's pair apart?  Always when its lines come from a table; a general one only where it would cost a cliff
  const size_t G = last_mode ? mm - 1 : mm;
  const bool extra = last_mode == 1 || last_mode == 2 || (last_mode == 3 && G % 16384 == 0);
  const size_t M = extra ? G : mm;                                   // items of the chunks proper
  const size_t rem = M % round;
  const size_t left = M >= round && rem < 1024 ? rem : 0, body = M - left;
  const size_t nch = (body + round - 1) / round;
  auto chunk_cnt = [&](size_t k) { return k + 1 < nch ? round : body - k * round; };
  auto quarter = [](size_t q) { return (q + 3) / 4; };
  auto local_out = [&](size_t cnt) {
    size_t q = quarter(cnt);
    while (q > LOCAL) q = quarter(q);
    return q;
  };
  const size_t ql = left ? quarter(left) : 0, qx = extra ? 1 : 0;
  size_t Qmain = 0;
  for (size_t k = 0; k < nch; k++) Qmain += local_out(chunk_cnt(k));
  const size_t Qc = Qmain + ql + qx;
  const size_t q0max = quarter(chunk_cnt(0));
  // two ping-pong buffers: the first takes a chunk's quads and the first level over all chunks' values (fan-in >= 2), the second the levels after them
  const size_t half_qc = (Qc + 1) / 2;
  const size_t capA = E * (q0max > half_qc ? q0max : half_qc), capB = E * (quarter(q0max) > quarter(Qc) + 16 ? quarter(q0max) : quarter(Qc) + 16);
  const size_t lanes_max = row_stride(lanes_for(chunk_cnt(0))), lanes_left = left ? row_stride(lanes_for(left)) : 0, lanes_x = extra ? row_stride(lanes_for(1)) : 0;
  const size_t T_STRIDE = 128;
  if ((capA + E * Qc) * W1 >= ((size_t)1 << 30)) return 0;      // the fold kernels' 32-bit lane offsets (kernels.cuh wsu_ld_hfp6)
  const size_t words = E * LINE3_WORDS_H * (lanes_max + lanes_left + lanes_x) + (size_t)WS_F_WORDS * (capA + capB + E * Qc + T_STRIDE);
  if (lines_reserve(c, words * 4) != 0) return 0;
  uint32_t* lines3 = c->lines_ws;
  uint32_t* lines3_left = lines3 + E * LINE3_WORDS_H * lanes_max;
  uint32_t* lines3_x = lines3_left + E * LINE3_WORDS_H * lanes_left;
  uint32_t* bufA = lines3_x + E * LINE3_WORDS_H * lanes_x;
  uint32_t* bufB = bufA + (size_t)WS_F_WORDS * capA;
  uint32_t* comb = bufB + (size_t)WS_F_WORDS * capB;
  uint32_t* t68 = comb + (size_t)WS_F_WORDS * E * Qc;
  const size_t comb_stride = E * Qc;
  size_t comb_off = 0;
  for (size_t k = 0; k < nch; k++) {
    const size_t lo = k * round, cnt = chunk_cnt(k);
    const size_t nlanes = lanes_for(cnt), lanes = row_stride(nlanes);
    const uint32_t* pw = d_pairs + lo;
    const int32_t* bw = d_bad + lo;
    if (cnt <= lines4_max)
      KL(KID_LINESP4, k_linesp4, dim3(blocks_for(4 * cnt)), dim3(BLS_BLOCK), cnt, stride, pw, bw, lines3, lanes);
    else
      KL(KID_LINESP, k_linesp, dim3((unsigned)(nlanes / BLS_BLOCK)), dim3(BLS_BLOCK), cnt, cnt, stride, pw, bw, lines3, lines3, lanes, (size_t)0, cnt, 1);
    if (k == 0 && (left || extra)) {
      // the leftover items and the signature's pair: chunks of their own on the tail stream, their values straight into the
      // combined level.  They start when the first chunk's line kernel is through -- beside that kernel, whose waves fill the
      // machine's slots exactly, a few extra waves cost a whole chain's time (above) -- and their own chains hide beside the short
      // tasks of the chunk's product kernels
      if (!c->tail) {
        HIPCK(hipStreamCreateWithFlags(&c->tail, hipStreamNonBlocking));
        HIPCK(hipEventCreateWithFlags(&c->ev_tail_fork, hipEventDisableTiming));
        HIPCK(hipEventCreateWithFlags(&c->ev_tail_join, hipEventDisableTiming));
      }
      HIPCK(hipEventRecord(c->ev_tail_fork, c->stream));
      HIPCK(hipStreamWaitEvent(c->tail, c->ev_tail_fork, 0));
      if (extra) {
        const uint32_t* px = d_pairs + (mm - 1);
        const int32_t* bx = d_bad + (mm - 1);
        if (last_mode == 3) KLS(KID_TAIL, c->tail, k_linesp4, dim3(1), dim3(BLS_BLOCK), (size_t)1, stride, px, bx, lines3_x, lanes_x);
        else KLS(KID_TAIL, c->tail, k_lines_fixed, dim3(1), dim3(BLS_BLOCK), stride, px, bx, lines3_x, lanes_x, last_mode);
        KLS(KID_TAIL, c->tail, k_line_quad, dim3(1, (unsigned)E), dim3(BLS_BLOCK), (size_t)1, (size_t)1, bx, (const uint32_t*)lines3_x, lanes_x, comb, comb_stride, Qc,
                           Qmain + ql);
      }
      if (left) {
        KLS(KID_TAIL, c->tail, k_linesp4, dim3(blocks_for(4 * left)), dim3(BLS_BLOCK), left, stride, (const uint32_t*)(d_pairs + body),
                           (const int32_t*)(d_bad + body), lines3_left, lanes_left);
        KLS(KID_TAIL, c->tail, k_line_quad, dim3(blocks_for(2 * ql), (unsigned)E), dim3(BLS_BLOCK), left, ql, (const int32_t*)(d_bad + body),
                           (const uint32_t*)lines3_left, lanes_left, comb, comb_stride, Qc, Qmain);
      }
      const hipError_t e1 = hipGetLastError(), e2 = hipEventRecord(c->ev_tail_join, c->tail);
      if (e1 != hipSuccess || e2 != hipSuccess) {
        (void)hipStreamSynchronize(c->tail);
        return fail(BLSGPU_E_HIP, "tail-stream launch failed");
      }
    }
    size_t q = quarter(cnt);
    if (q <= LOCAL) {
      KL(KID_LINE_QUAD, k_line_quad, dim3(blocks_for(2 * q), (unsigned)E), dim3(BLS_BLOCK), cnt, q, bw, (const uint32_t*)lines3, lanes, comb, comb_stride, Qc, comb_off);
    } else {
      KL(KID_LINE_QUAD, k_line_quad, dim3(blocks_for(2 * q), (unsigned)E), dim3(BLS_BLOCK), cnt, q, bw, (const uint32_t*)lines3, lanes, bufA, E * q, q, (size_t)0);
      uint32_t *src = bufA, *dst = bufB;
      while (q > LOCAL) {
        const size_t qo = quarter(q);
        if (qo <= LOCAL)
          KL(KID_F12_FOLD4, k_f12_fold4, dim3(blocks_for(2 * qo), (unsigned)E), dim3(BLS_BLOCK), q, qo, 4, (const uint32_t*)src, E * q, q, comb, comb_stride, Qc, comb_off);
        else
          KL(KID_F12_FOLD4, k_f12_fold4, dim3(blocks_for(2 * qo), (unsigned)E), dim3(BLS_BLOCK), q, qo, 4, (const uint32_t*)src, E * q, q, dst, E * qo, qo, (size_t)0);
        uint32_t* t = src;
        src = dst;
        dst = t;
        q = qo;
      }
    }
    comb_off += q;
  }
  if (left || extra) HIPCK(hipStreamWaitEvent(c->stream, c->ev_tail_join, 0));
  // all chunks' values together
  {
    const uint32_t* src = comb;
    size_t q = Qc;
    uint32_t *dst = bufA, *other = bufB;
    // Levels that fill the machine on lane pairs (fan-in four, or five where that saves a level), down to at most ENGINE_FROM values
    // per entry; the rest on the engine, sixteen values per workgroup (two launches for up to 256 values): a product there takes
    // 3.7 us against 43 on a lane pair, and a lane-pair level of a few hundred tasks is nothing but its chain of fan - 1 products
    // (~0.13 ms).  1,025 values per entry -- a round of pairs and the signature's -- go 205, 52 on lane pairs, then 4, 1 on the engine.
    const long engine_from_env = knobs().tree_engine_from;
    const size_t ENGINE_FROM = engine_from_env >= 16 && engine_from_env <= 256 ? (size_t)engine_from_env : 128;
    int levels = 0;
    for (size_t cap = ENGINE_FROM; cap < q; cap *= 5) levels++;
    while (q > ENGINE_FROM) {
      size_t fan = 2, reach = ENGINE_FROM;
      for (int l = 1; l < levels; l++) reach *= 4;            // what the remaining levels can take at fan-in four
      while (fan < 5 && (q + fan - 1) / fan > reach) fan++;    // (five always suffices: `levels` was counted for fan-in five)
      levels--;
      const size_t qo = (q + fan - 1) / fan;
      KL(KID_F12_FOLD4, k_f12_fold4, dim3(blocks_for(2 * qo), (unsigned)E), dim3(BLS_BLOCK), q, qo, (int)fan, src, E * q, q, dst, E * qo, qo, (size_t)0);
      src = dst;
      uint32_t* t = dst;
      dst = other;
      other = t;
      q = qo;
    }
    if (q > 16) {
      const size_t qo = (q + 15) / 16;
      KL(KID_F12_TREE, k_f12_tree_seg, dim3((unsigned)qo, (unsigned)E), dim3(WIDE_ENGINE_BLOCK), q, src, E * q, q, dst, E * qo, qo);
      src = dst;
      q = qo;
    }
    KL(KID_F12_TREE, k_f12_tree_seg, dim3(1, (unsigned)E), dim3(WIDE_ENGINE_BLOCK), q, src, E * q, q, t68, T_STRIDE, (size_t)1);
    KL(KID_HORNER, k_f12_horner_wide, dim3(1), dim3(WIDE_ENGINE_BLOCK), (const uint32_t*)t68, T_STRIDE, d_f, stride);
  }
  HIPCK(hipGetLastError());
  *outputs = 1;
  *done = true;
  return 0;
}

// Miller loops of a pairing product over mm one-pair items (workspace stride given; flagged items contribute 1): leaves *outputs
// partial products at the start of the Fp12 workspace.  Round 3: two items share a merged line value (k_linesp, two passes),
// and one accumulator takes the values of `group` such pairs per step (k_millerfp).  The items are cut into chunks of 2 cnt
// items whose lane-pair counts fill whole workgroups -- and whole machine rounds (65,536 lane pairs) when there are that many:
// a single extra wave after a full round costs a lone wave's latency, ~7 ms -- and what is left (< 1,024 items: 262,145 pairs
// leave one) goes through k_miller1s on the context's tail stream BESIDE the chunks.  BLSGPU_MILLER_V1=1, fewer than 4,096
// items, or no memory for the line workspace: k_miller1s for everything.
int run_miller_product(Ctx* c, size_t mm, size_t stride, uint32_t* d_pairs, int32_t* d_bad, uint32_t* d_f, size_t* outputs, int last_mode = 0) {
  {
    bool done = false;
    if (int rc = run_miller_product_tree(c, mm, stride, d_pairs, d_bad, d_f, outputs, &done, last_mode)) return rc;
    if (done) return 0;
  }
  const size_t chunk_max = 2 * miller_chunk_items(), round = 65536;
  const size_t words_per_lane = (size_t)MILLER_ENTRIES * (LINE5_WORDS + LINE3_WORDS_H);
  auto nice = [&](size_t pairs) {          // virtual items of the next chunk when `pairs` virtual items could still be formed
    if (pairs > chunk_max) pairs = chunk_max;
    return pairs >= round ? pairs / round * round : pairs / 32 * 32;
  };
  if (mm >= 64 && mm <= round + 1023 && chunk_max) {
    // at most one machine round of lane pairs: one item per accumulator slot, plain lines (k_linesp pass 1, k_millerfp3); up to 1,023
    // items beyond the round go through k_miller1s on the tail stream beside them
    const size_t cnt = mm >= round ? round : mm, left = mm - cnt;      // below a round: every item gets a lane pair (the last workgroup may be partly idle)
    const size_t nlanes = lanes_for(cnt), lanes = row_stride(nlanes);
    if (lines_reserve(c, (size_t)MILLER_ENTRIES * LINE3_WORDS_H * 4 * lanes) == 0) {
      if (left) {
        if (!c->tail) {
          HIPCK(hipStreamCreateWithFlags(&c->tail, hipStreamNonBlocking));
          HIPCK(hipEventCreateWithFlags(&c->ev_tail_fork, hipEventDisableTiming));
          HIPCK(hipEventCreateWithFlags(&c->ev_tail_join, hipEventDisableTiming));
        }
        HIPCK(hipEventRecord(c->ev_tail_fork, c->stream));
        HIPCK(hipStreamWaitEvent(c->tail, c->ev_tail_fork, 0));
        KLS(KID_TAIL, c->tail, k_miller1s, dim3(blocks_for(2 * MILLER1_OUTPUTS(left))), dim3(BLS_BLOCK), left, stride, (const uint32_t*)(d_pairs + cnt),
                           (const int32_t*)(d_bad + cnt), d_f + cnt);
        const hipError_t e1 = hipGetLastError(), e2 = hipEventRecord(c->ev_tail_join, c->tail);
        if (e1 != hipSuccess || e2 != hipSuccess) {
          (void)hipStreamSynchronize(c->tail);
          return fail(BLSGPU_E_HIP, "tail-stream launch failed");
        }
      }
      const dim3 grid((unsigned)(nlanes / BLS_BLOCK));
      // k_linesp pass 1 on a "chunk" whose partners do not exist (half = cnt): every lane pair walks its own item and stores its lines
      KL(KID_LINESP, k_linesp, grid, dim3(BLS_BLOCK), cnt, cnt, stride, (const uint32_t*)d_pairs, (const int32_t*)d_bad, c->lines_ws, c->lines_ws, lanes, (size_t)0, cnt, 1);
      KL(KID_MILLERFP, k_millerfp3, grid, dim3(BLS_BLOCK), cnt, cnt, 1, (const int32_t*)d_bad, (const uint32_t*)c->lines_ws, lanes, d_f, stride, (size_t)0);
      if (left) HIPCK(hipStreamWaitEvent(c->stream, c->ev_tail_join, 0));
      HIPCK(hipGetLastError());
      *outputs = cnt + (left ? MILLER1_OUTPUTS(left) : 0);
      return 0;
    }
  }
  const size_t first_cnt = mm >= 4096 && chunk_max ? nice(mm / 2) : 0;
  if (first_cnt == 0 || lines_reserve(c, words_per_lane * 4 * row_stride(lanes_for(first_cnt))) != 0) {
    MILLER1_LAUNCH(mm, stride, d_pairs, d_bad, d_f);
    HIPCK(hipGetLastError());
    *outputs = MILLER1_OUTPUTS(mm);
    return 0;
  }
  // the plan: chunks [lo, lo + 2 cnt) until fewer than 1,024 items are left
  struct Chunk { size_t lo, cnt; };
  std::vector<Chunk> plan;
  size_t lo = 0;
  while (mm - lo >= 1024) {
    const size_t cnt = nice((mm - lo) / 2);
    plan.push_back({lo, cnt});
    lo += 2 * cnt;
  }
  size_t out0 = 0;
  for (const Chunk& ch : plan) {
    int group = (int)(ch.cnt / round);              // one machine round of accumulators when the chunk has several rounds of line values
    if (group < 1) group = 1;
    if (group > 4) group = 4;
    out0 += (ch.cnt + group - 1) / group;
  }
  const size_t left = mm - lo, left_out0 = out0;
  if (left) {                                       // first in time: a few waves whose latency hides under the chunks
    if (!c->tail) {
      HIPCK(hipStreamCreateWithFlags(&c->tail, hipStreamNonBlocking));
      HIPCK(hipEventCreateWithFlags(&c->ev_tail_fork, hipEventDisableTiming));
      HIPCK(hipEventCreateWithFlags(&c->ev_tail_join, hipEventDisableTiming));
    }
    HIPCK(hipEventRecord(c->ev_tail_fork, c->stream));
    HIPCK(hipStreamWaitEvent(c->tail, c->ev_tail_fork, 0));
    KLS(KID_TAIL, c->tail, k_miller1s, dim3(blocks_for(2 * MILLER1_OUTPUTS(left))), dim3(BLS_BLOCK), left, stride, (const uint32_t*)(d_pairs + lo),
                       (const int32_t*)(d_bad + lo), d_f + left_out0);
    const hipError_t e1 = hipGetLastError(), e2 = hipEventRecord(c->ev_tail_join, c->tail);
    if (e1 != hipSuccess || e2 != hipSuccess) {
      (void)hipStreamSynchronize(c->tail);
      return fail(BLSGPU_E_HIP, "tail-stream launch failed");
    }
  }
  out0 = 0;
  for (const Chunk& ch : plan) {
    const size_t nlanes = lanes_for(ch.cnt), lanes = row_stride(nlanes);
    uint32_t* lines3 = c->lines_ws + (size_t)MILLER_ENTRIES * LINE5_WORDS * lanes;
    int group = (int)(ch.cnt / round);
    if (group < 1) group = 1;
    if (group > 4) group = 4;
    const size_t q = (ch.cnt + group - 1) / group;
    const dim3 grid((unsigned)(nlanes / BLS_BLOCK));
    // the chunk's items as a workspace of its own: item v pairs with item v + cnt
    const uint32_t* pw = d_pairs + ch.lo;
    const int32_t* bw = d_bad + ch.lo;
    KL(KID_LINESP, k_linesp, grid, dim3(BLS_BLOCK), 2 * ch.cnt, ch.cnt, stride, pw, bw, c->lines_ws, lines3, lanes, (size_t)0, ch.cnt, 1);
    KL(KID_LINESP, k_linesp, grid, dim3(BLS_BLOCK), 2 * ch.cnt, ch.cnt, stride, pw, bw, c->lines_ws, lines3, lanes, (size_t)0, ch.cnt, 2);
    KL(KID_MILLERFP, k_millerfp, dim3(blocks_for(2 * q)), dim3(BLS_BLOCK), ch.cnt, q, group, (const uint32_t*)c->lines_ws, lanes, d_f, stride, out0);
    out0 += q;
  }
  if (left) {
    HIPCK(hipStreamWaitEvent(c->stream, c->ev_tail_join, 0));
    out0 += MILLER1_OUTPUTS(left);
  }
  HIPCK(hipGetLastError());
  *outputs = out0;
  return 0;
}

// product of m Fp12 values in a workspace (stride given) folded into item 0
int run_f12_fold(Ctx* c, uint32_t* d_f, size_t m, size_t stride) {
  // halvings on lane pairs while there are thousands of values (parallel work, 0.15 ms per launch), then sixteen-way products on
  // the engine (k_f12_tree_wide, ~50 us per launch): 65,536 values are one value after 4 + 3 launches instead of 16
  const bool engine = wide_max_items() > 0 && coop_max_items() > 0;
  const size_t ENGINE_FROM = 4096;
  size_t cur = m;
  while (cur > (engine ? ENGINE_FROM : 1)) {
    size_t half = (cur + 1) / 2;
    KL(KID_F12_FOLD, k_f12_fold, dim3(blocks_for(half)), dim3(BLS_BLOCK), cur, half, d_f, stride);
    cur = half;
  }
  if (cur > 1) {
    const size_t cap = ENGINE_FROM / 16;                      // items per ping-pong buffer
    if (!c->fold_ws) HIPCK(hipMalloc((void**)&c->fold_ws, 2 * cap * (size_t)WS_F_WORDS * 4));
    const uint32_t* src = d_f;
    size_t sstride = stride;
    int which = 0;
    while (cur > 1) {
      const size_t outn = (cur + 15) / 16;
      uint32_t* dst = outn == 1 ? d_f : c->fold_ws + (size_t)which * cap * WS_F_WORDS;
      const size_t dstride = outn == 1 ? stride : cap;
      KL(KID_F12_FOLD, k_f12_tree_wide, dim3((unsigned)outn), dim3(WIDE_ENGINE_BLOCK), cur, src, sstride, dst, dstride);
      src = dst;
      sstride = dstride;
      which ^= 1;
      cur = outn;
    }
  }
  HIPCK(hipGetLastError());
  return 0;
}
// ... then the verdict of item 0
int run_f12_product_verdict(Ctx* c, uint32_t* d_f, size_t m, size_t stride, int32_t* d_verdict) {
  int rc = run_f12_fold(c, d_f, m, stride);
  if (rc) return rc;
  if (wide_max_items() > 0 && coop_max_items() > 0) KL(KID_FINALEXP_ONE, k_finalexp_wide_ws, dim3(1), dim3(WIDE_ENGINE_BLOCK), (const uint32_t*)d_f, stride, d_verdict);
  else if (coop_max_items() > 0) KL(KID_FINALEXP_ONE, k_finalexp_coop, dim3(1), dim3(BLS_BLOCK), d_f, stride, d_verdict);
  else KL(KID_FINALEXP_ONE, k_finalexp_ones, dim3(1), dim3(BLS_BLOCK), d_f, stride, d_verdict);
  HIPCK(hipGetLastError());
  return 0;
}

// lanes (lane pairs for G2) of the first stage of a point sum.  The cap leaves a few compute units' worth of wave slots free in
// every XCD: a grid that fills the machine EXACTLY (65,536 lane pairs = 2,048 waves = two per SIMD) takes twice as long as soon
// as other kernels hold a few slots, because some workgroups then wait for a whole round -- and the side streams do hold
// slots: the engine workgroups of the message hash and of the signature's Miller function take a whole CU each (their waves
// use 355 registers), and workgroups go round-robin to the 8 XCDs, so two of them in one XCD cost it 16 slots.  Measured
// (tools/dbg/acc.py, 2^20 keys): 1.15 / 1.17 ms at 58,368 / 57,344 lane pairs, 1.28 at 59,392, 1.48 at 61,440.
size_t accumulate_lanes(size_t n) {
  const long cap = knobs().acc_lanes;                     // default 57,344: 224 of 256 compute units at 256 lane pairs each
  size_t t = n / 4;
  if (t < 64) t = 64;
  if (t > (size_t)cap) t = (size_t)cap;
  return (t + 63) & ~(size_t)63;
}

bool msm_use_pippenger(size_t n);
bool msm_use_v1();
struct msm2_plan {
  int c, W, CH, Q, E;
  size_t nb, nchunks;
};
struct msm2_ws {
  msm2_plan p;
  uint32_t *aff, *cnt, *off, *cur, *idx, *tiles;
  uint64_t* subs;
  uint8_t *inf, *sums, *part;
  uint32_t *tab = nullptr, *jt = nullptr;     // weighted tables (k_msm2_tables) and their Jacobian staging: verify_secure only
};
int msm2_ws_take(Ctx* c, size_t n, int G, msm2_ws& w, bool tables = false);
size_t msm2_tables_bytes(size_t n, int G);
template <int G>
int run_msm2_prep(Ctx* c, const uint8_t* d_pts, int fmt, const uint32_t* d_perm, size_t n, msm2_ws& w);
template <int G>
int run_msm2_rest(Ctx* c, const uint8_t* d_scalars, size_t n, msm2_ws& w, uint8_t* d_out, bool normalize = true);
template <int G>
int run_msm_pippenger(Ctx* c, const uint8_t* d_pts, int fmt, const uint8_t* d_scalars, const uint32_t* d_perm, size_t n, uint8_t* d_out);

// m partial sums (RAW_PROJ, device) -> partials[0].  Wide levels of the tree run on the lane-local / lane-pair fold (one
// addition deep per launch, efficient while there are thousands of additions); the last 4,096 points go through the row-wide
// engine, sixteen per workgroup and launch (k_point_tree_wide), between the partials and a small second buffer.
const size_t POINT_TREE_START = 4096;
template <int G>
int run_point_fold(Ctx* c, uint8_t* d_partials, size_t m) {
  const size_t psz = point_bytes(G, BLSGPU_FMT_RAW_PROJ);
  size_t cur = m;
  const bool wide = wide_max_items() >= 1;               // BLSGPU_WIDE_MAX=0 switches the row-wide engine off everywhere
  while (cur > (wide ? POINT_TREE_START : 1)) {
    size_t half = (cur + 1) / 2;
    if (G == 2) KL(KID_POINT_FOLD, k_point_fold_g2s, dim3(blocks_for(2 * half)), dim3(BLS_BLOCK), cur, half, d_partials);
    else KL(KID_POINT_FOLD, k_point_fold<G>, dim3(blocks_for(half)), dim3(BLS_BLOCK), cur, half, d_partials);
    cur = half;
  }
  if (cur > 1) {
    uint8_t* d_tmp = (uint8_t*)arena_take(c, psz * ((POINT_TREE_START + WIDE_PT_POINTS - 1) / WIDE_PT_POINTS));
    if (!d_tmp) return fail(BLSGPU_E_HIP, "internal: arena too small");
    const uint8_t* src = d_partials;
    while (cur > 1) {
      const size_t nb = (cur + WIDE_PT_POINTS - 1) / WIDE_PT_POINTS;
      uint8_t* dst = (nb == 1 || src != d_partials) ? d_partials : d_tmp;   // one workgroup reads all its inputs before it writes
      KL(KID_POINT_FOLD, k_point_tree_wide<G>, dim3((unsigned)nb), dim3(WIDE_ENGINE_BLOCK), cur, src, dst);
      src = dst;
      cur = nb;
    }
  }
  HIPCK(hipGetLastError());
  return 0;
}

// sum (or sum of scalar multiples) of n points of group G into partials[0] (RAW_PROJ, device)
template <int G>
int run_point_sum(Ctx* c, const uint8_t* d_pts, int fmt, const uint8_t* d_scalars, const uint32_t* d_perm, size_t n,
                  uint8_t* d_partials, size_t T) {
  if (d_scalars && msm_use_pippenger(n)) {
    if (msm_use_v1()) return run_msm_pippenger<G>(c, d_pts, fmt, d_scalars, d_perm, n, d_partials);
    msm2_ws w;
    int rc = msm2_ws_take(c, n, G, w);
    if (rc) return rc;
    if ((rc = run_msm2_prep<G>(c, d_pts, fmt, d_perm, n, w))) return rc;
    return run_msm2_rest<G>(c, d_scalars, n, w, d_partials);
  }
  unsigned nb = blocks_for(T);
  if (d_scalars)
    KL(KID_ACCUM, (k_accumulate<G, 1>), dim3(nb), dim3(BLS_BLOCK), n, d_pts, fmt, d_scalars, d_perm, d_partials, T);
  else
    if (G == 2 && !d_perm) KL(KID_ACCUM, k_accumulate_g2s, dim3(blocks_for(2 * T)), dim3(BLS_BLOCK), n, d_pts, fmt, d_partials, T);
    else KL(KID_ACCUM, (k_accumulate<G, 0>), dim3(nb), dim3(BLS_BLOCK), n, d_pts, fmt, d_scalars, d_perm, d_partials, T);
  return run_point_fold<G>(c, d_partials, T);
}

// Pippenger MSM into out[0] (RAW_PROJ, device, Z = 1).  Workspace comes from the arena (caller reserved msm_ws_bytes).
struct msm_plan {
  int c, W, clast, CH;
  size_t nb, nchunks;
};
msm_plan msm_make_plan(size_t n, int G) {
  msm_plan p;
  // measured at 65,536 points (tools/dbg/msm.py).  The chunk kernel is latency-bound (doubling chains) and the bucket
  // kernel throughput-bound, and a G2 addition costs about three G1 additions: G2 is best with 11-bit windows and 4-bucket
  // chunks (sort 0.4 + buckets 3.3 + chunks 2.9 ms against 0.6 + 2.7 + 3.9 with 12 / 8), G1 with 12 / 8 (0.6 + 1.4 + 2.5)
  p.c = n >= 16384 ? (G == 2 ? 11 : 12) : 8;
  p.CH = (n >= 16384 && G == 2) ? 4 : 8;   // short chunks: the 2^(c w) doublings of the chunk lanes dominate their critical path
  if (knobs().msm_c) p.c = (int)knobs().msm_c;         // tuning overrides (window bits, buckets per chunk lane),
  if (knobs().msm_ch) p.CH = (int)knobs().msm_ch;      // clamped to what the kernels assume
  if (p.c < 4) p.c = 4;
  if (p.c > 16) p.c = 16;
  p.W = 255 / p.c;                      // scalars are < r < 2^255
  p.clast = 255 - p.c * (p.W - 1);      // the last window takes the remainder: c <= clast < 2c ...
  if (p.clast > 16) {                   // ... unless that is above 16 bits (c = 13, 14, 16: 21, 17, 31 bits, up to 2^31 buckets):
    p.W++;                              // one more window, and the last one narrower than c (8, 3, 15 bits)
    p.clast = 255 - p.c * (p.W - 1);
  }
  if (p.CH < 1) p.CH = 1;
  while (p.CH & (p.CH - 1)) p.CH &= p.CH - 1;                       // a power of two, so that it divides 2^c and 2^clast
  if (p.CH > (1 << p.c)) p.CH = 1 << p.c;
  if (p.CH > (1 << p.clast)) p.CH = 1 << p.clast;
  p.nb = ((size_t)(p.W - 1) << p.c) + ((size_t)1 << p.clast);
  p.nchunks = p.nb / p.CH;
  return p;
}
size_t msm2_ws_bytes(size_t n);
size_t msm_ws_bytes(size_t n) {         // callers reserve for either group and for the generation that runs
  size_t need = msm2_ws_bytes(n);
  if (!msm_use_v1()) return need;       // the first generation's plan is sized only when BLSGPU_MSM_V1 selects it
  for (int G = 1; G <= 2; G++) {
    msm_plan p = msm_make_plan(n, G);
    size_t b = 3 * pad256(4 * p.nb) + pad256(4 * n * p.W) + pad256(4 * scan_tiles(p.nb)) + pad256(288 * p.nb) + pad256(288 * p.nchunks) + 4096;
    if (b > need) need = b;
  }
  return need;
}
// ---- second-generation MSM (csrc/msm2.cuh): endomorphism split, signed digits, mixed additions --------------------
msm2_plan msm2_make_plan(size_t n, int G) {
  msm2_plan p;
  const int bits = G == 1 ? 128 : 64;     // width of the sub-scalars (k = a0 + a1 z^2 on G1, base-z digits on G2)
  p.E = G == 1 ? 2 : 4;
  int lg = 0;
  while (((size_t)1 << (lg + 1)) <= n) lg++;
  p.c = lg - 3;                           // target window width: 13 bits at 65,536 points (measured sweep, tools/dbg/msm.py)
  if (p.c < 6) p.c = 6;
  if (p.c > 14) p.c = 14;
  p.CH = 4;                               // short chunks: the chunk lanes are a latency chain (4 / 8 / 16 measured: 1.1 / 1.4 / 2.1 ms)
  if (knobs().msm2_c) p.c = (int)knobs().msm2_c;      // tuning overrides, clamped to what the kernels assume
  if (knobs().msm2_ch) p.CH = (int)knobs().msm2_ch;
  if (p.c < 4) p.c = 4;
  if (p.c > 16) p.c = 16;
  // bits + 1 positions (one spare for the recoding carry) in W windows whose widths differ by at most one (msm2.cuh)
  p.W = (bits + 1 + p.c / 2) / p.c;
  if (p.W < 1) p.W = 1;
  const int base = (bits + 1) / p.W, rem = (bits + 1) % p.W;
  if (p.CH < 1) p.CH = 1;
  while (p.CH & (p.CH - 1)) p.CH &= p.CH - 1;
  if (p.CH > (1 << (base - 1))) p.CH = 1 << (base - 1);             // a chunk never straddles two windows
  p.nb = ((size_t)rem << base) + ((size_t)(p.W - rem) << (base - 1));
  p.nchunks = p.nb / p.CH;
  // parts per bucket: about 130,000 (bucket, part) lanes keep every SIMD busy through the uneven bucket sizes (measured:
  // 1 / 2 / 4 parts at 40,960 bucket lanes: 2.2 / 1.3 / 0.8 ms for G1); a fully parallel pass merges the parts afterwards
  const size_t lanes = p.nb * (G == 1 ? 1 : 2);
  p.Q = (int)((131072 + lanes - 1) / lanes);
  if (knobs().msm2_q) p.Q = (int)knobs().msm2_q;
  if (p.Q < 1) p.Q = 1;
  if (p.Q > 8) p.Q = 8;
  return p;
}
size_t msm2_ws_bytes(size_t n) {          // callers reserve for either group
  size_t need = 0;
  for (int G = 1; G <= 2; G++) {
    const msm2_plan p = msm2_make_plan(n, G);
    const size_t affw = (G == 1 ? 2 : 4) * FP_NL;
    size_t b = pad256(4 * affw * p.E * n) + pad256(n) + pad256(32 * n) + 3 * pad256(4 * p.nb) + pad256(4 * n * p.E * p.W) + pad256(4 * scan_tiles(p.nb)) +
               pad256(288 * p.nb * p.Q) + pad256(288 * p.nchunks) + 4096;
    if (b > need) need = b;
  }
  return need;
}
// the weighted tables of k_msm2_tables: W affine entries per image, and 4 coordinates per window of Jacobian staging
size_t msm2_tables_bytes(size_t n, int G) {
  const msm2_plan p = msm2_make_plan(n, G);
  const size_t affw = (G == 1 ? 2 : 4) * FP_NL;
  return pad256(4 * affw * p.E * p.W * n) + pad256(4 * (affw / 2) * 4 * (p.W > 1 ? p.W - 1 : 1) * n) + 512;
}
int msm2_ws_take(Ctx* c, size_t n, int G, msm2_ws& w, bool tables) {
  w.p = msm2_make_plan(n, G);
  const msm2_plan& p = w.p;
  const size_t affw = (G == 1 ? 2 : 4) * FP_NL;
  Carver mem{c};
  if (tables) {
    w.tab = mem.take<uint32_t>(4 * affw * p.E * p.W * n);
    w.jt = mem.take<uint32_t>(4 * (affw / 2) * 4 * (p.W > 1 ? p.W - 1 : 1) * n);
  }
  w.aff = mem.take<uint32_t>(4 * affw * p.E * n);
  w.inf = mem.take<uint8_t>(n);
  w.subs = mem.take<uint64_t>(32 * n);
  w.cnt = mem.take<uint32_t>(4 * p.nb);
  w.off = mem.take<uint32_t>(4 * p.nb);
  w.cur = mem.take<uint32_t>(4 * p.nb);
  w.idx = mem.take<uint32_t>(4 * n * p.E * p.W);
  w.tiles = mem.take<uint32_t>(4 * scan_tiles(p.nb));
  w.sums = mem.take<uint8_t>(288 * p.nb * p.Q);
  w.part = mem.take<uint8_t>(288 * p.nchunks);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  return 0;
}
// the scalar-independent part: every point to affine, with its endomorphism images
template <int G>
int run_msm2_prep(Ctx* c, const uint8_t* d_pts, int fmt, const uint32_t* d_perm, size_t n, msm2_ws& w) {
  KL(KID_MSM_PREP, k_msm2_prep<G>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_pts, fmt, d_perm, w.aff, w.inf);
  if (w.tab)     // every window's multiple of every image, while the caller's host still hashes (verify_secure)
    KL(KID_MSM_PREP, k_msm2_tables<G>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint32_t*)w.aff, (const uint8_t*)w.inf, w.p.W, w.tab, w.jt);
  HIPCK(hipGetLastError());
  return 0;
}
// ... and the rest: digits, bucket lists, bucket sums, window weights, fold.  d_out[0] = the sum (RAW_PROJ, Z = 1)
template <int G>
int run_msm2_rest(Ctx* c, const uint8_t* d_scalars, size_t n, msm2_ws& w, uint8_t* d_out, bool normalize) {
  const msm2_plan& p = w.p;
  HIPCK(hipMemsetAsync(w.cnt, 0, 4 * p.nb, c->stream));
  HIPCK(hipMemsetAsync(w.cur, 0, 4 * p.nb, c->stream));
  KL(KID_MSM_SORT, k_msm2_count<G>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_scalars, (const uint8_t*)w.inf, p.W, w.cnt, w.subs);
  int rc = run_scan_u32(c, KID_MSM_SORT, p.nb, w.cnt, w.off, w.tiles);
  if (rc) return rc;
  KL(KID_MSM_SORT, k_msm2_fill<G>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint64_t*)w.subs, (const uint8_t*)w.inf, p.W, (const uint32_t*)w.off, w.cur, w.idx);
  const size_t nbq = p.nb * p.Q;
  const uint32_t* pts_ws = w.tab ? w.tab : w.aff;
  const int tabW = w.tab ? p.W : 0, weighted = w.tab ? 1 : 0;
  if (G == 2) KL(KID_MSM_BUCKET, k_msm2_bucket_g2s, dim3(blocks_for(2 * nbq)), dim3(BLS_BLOCK), p.nb, p.Q, pts_ws, (const uint32_t*)w.cnt, (const uint32_t*)w.off, (const uint32_t*)w.idx, w.sums, tabW);
  else KL(KID_MSM_BUCKET, k_msm2_bucket_g1, dim3(blocks_for(nbq)), dim3(BLS_BLOCK), p.nb, p.Q, pts_ws, (const uint32_t*)w.cnt, (const uint32_t*)w.off, (const uint32_t*)w.idx, w.sums, tabW);
  if (p.Q > 1) {
    if (G == 2) KL(KID_MSM_MERGE, k_msm2_merge_g2s, dim3(blocks_for(2 * p.nb)), dim3(BLS_BLOCK), p.nb, p.Q, w.sums);
    else KL(KID_MSM_MERGE, k_msm2_merge_g1, dim3(blocks_for(p.nb)), dim3(BLS_BLOCK), p.nb, p.Q, w.sums);
  }
  if (G == 2) KL(KID_MSM_CHUNK, k_msm2_chunk_g2q, dim3(blocks_for(4 * p.nchunks)), dim3(BLS_BLOCK), p.W, p.CH, p.Q, (const uint8_t*)w.sums, w.part, weighted);
  else KL(KID_MSM_CHUNK, k_msm2_chunk_g1p, dim3(blocks_for(2 * p.nchunks)), dim3(BLS_BLOCK), p.W, p.CH, p.Q, (const uint8_t*)w.sums, w.part, weighted);
  if (int rc = run_point_fold<G>(c, w.part, p.nchunks)) return rc;
  // Z = 1 makes the output bytes independent of the (atomic) bucket fill order; a caller that only feeds the point to the
  // pairing stages skips it
  if (normalize) KL(KID_MSM_NORM, k_normalize<G>, dim3(1), dim3(BLS_BLOCK), w.part);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(d_out, w.part, point_bytes(G, BLSGPU_FMT_RAW_PROJ), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}
bool msm_use_v1() { return knobs().msm_v1 != 0; }   // A/B switch: the first-generation bucket method (unsigned digits, full additions)

bool msm_use_pippenger(size_t n) { return !knobs().msm_naive && n >= 1024; }
template <int G>
int run_msm_pippenger(Ctx* c, const uint8_t* d_pts, int fmt, const uint8_t* d_scalars, const uint32_t* d_perm, size_t n, uint8_t* d_out) {
  msm_plan p = msm_make_plan(n, G);
  Carver mem{c};
  uint32_t* d_cnt = mem.take<uint32_t>(4 * p.nb);
  uint32_t* d_off = mem.take<uint32_t>(4 * p.nb);
  uint32_t* d_cur = mem.take<uint32_t>(4 * p.nb);
  uint32_t* d_idx = mem.take<uint32_t>(4 * n * p.W);
  uint32_t* d_tiles = mem.take<uint32_t>(4 * scan_tiles(p.nb));
  uint8_t* d_sums = mem.take<uint8_t>(288 * p.nb);
  uint8_t* d_part = mem.take<uint8_t>(288 * p.nchunks);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  HIPCK(hipMemsetAsync(d_cnt, 0, 4 * p.nb, c->stream));
  HIPCK(hipMemsetAsync(d_cur, 0, 4 * p.nb, c->stream));
  KL(KID_MSM_SORT, k_msm_count, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_scalars, p.c, p.W, p.clast, d_cnt);
  {
    int rc = run_scan_u32(c, KID_MSM_SORT, p.nb, d_cnt, d_off, d_tiles);
    if (rc) return rc;
  }
  KL(KID_MSM_SORT, k_msm_fill, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_scalars, p.c, p.W, p.clast, d_off, d_cur, d_idx);
  if (G == 2) KL(KID_MSM_BUCKET, k_msm_bucket_g2s, dim3(blocks_for(2 * p.nb)), dim3(BLS_BLOCK), p.nb, d_pts, fmt, d_perm, d_cnt, d_off, d_idx, d_sums);
  else KL(KID_MSM_BUCKET, k_msm_bucket<G>, dim3(blocks_for(p.nb)), dim3(BLS_BLOCK), p.nb, d_pts, fmt, d_perm, d_cnt, d_off, d_idx, d_sums);
  if (G == 2) KL(KID_MSM_CHUNK, k_msm_chunk_g2q, dim3(blocks_for(4 * p.nchunks)), dim3(BLS_BLOCK), p.c, p.W, p.clast, p.CH, d_sums, d_part);
  else KL(KID_MSM_CHUNK, k_msm_chunk_g1p, dim3(blocks_for(2 * p.nchunks)), dim3(BLS_BLOCK), p.c, p.W, p.clast, p.CH, d_sums, d_part);
  if (int rc = run_point_fold<G>(c, d_part, p.nchunks)) return rc;
  KL(KID_MSM_NORM, k_normalize<G>, dim3(1), dim3(BLS_BLOCK), d_part);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(d_out, d_part, point_bytes(G, BLSGPU_FMT_RAW_PROJ), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

// ---- hash_public_keys_with_sorted on the device (reference src/secure_aggregation.rs:41-103,269-335) -----------------
// Workspace of the key sort / coefficient step, carved from the arena.
struct keysort_ws {
  uint32_t *perm_a, *perm_b, *hist, *tiles, *flag;
  uint8_t* sorted;
  size_t ntiles;
};
size_t keysort_ws_bytes(size_t n, size_t width) {
  const size_t nt = (n + UK_SORT_TILE - 1) / UK_SORT_TILE;
  return 2 * pad256(4 * n) + pad256(4 * 256 * nt) + pad256(4 * scan_tiles(256 * nt)) + pad256(width * n) + 5 * 256 + 64;
}
int keysort_ws_take(Ctx* c, size_t n, size_t width, keysort_ws& w) {
  w.ntiles = (n + UK_SORT_TILE - 1) / UK_SORT_TILE;
  Carver mem{c};
  w.perm_a = mem.take<uint32_t>(4 * n);
  w.perm_b = mem.take<uint32_t>(4 * n);
  w.hist = mem.take<uint32_t>(4 * 256 * w.ntiles);
  w.tiles = mem.take<uint32_t>(4 * scan_tiles(256 * w.ntiles));
  w.sorted = mem.take<uint8_t>(width * n);
  w.flag = mem.take<uint32_t>(64);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  return 0;
}
// stable LSD radix sort on key bytes [0, nbytes): the result lands in w.perm_a
int run_key_sort_passes(Ctx* c, const uint8_t* d_kb, size_t n, size_t width, int nbytes, keysort_ws& w) {
  // nbytes passes ping-pong between the two buffers; start so that the last pass writes perm_a
  uint32_t* bufs[2] = {w.perm_a, w.perm_b};
  int dst = (nbytes & 1) ? 0 : 1;
  const uint32_t* src = nullptr;   // identity
  const unsigned nt = (unsigned)w.ntiles;
  for (int b = nbytes - 1; b >= 0; b--) {
    KL(KID_KEY_SORT, k_rs_hist, dim3(nt), dim3(BLS_BLOCK), n, d_kb, width, b, src, w.hist, w.ntiles);
    int rc = run_scan_u32(c, KID_KEY_SORT, 256 * w.ntiles, w.hist, w.hist, w.tiles);
    if (rc) return rc;
    KL(KID_KEY_SORT, k_rs_scatter, dim3(nt), dim3(BLS_BLOCK), n, d_kb, width, b, src, (const uint32_t*)w.hist, w.ntiles, bufs[dst]);
    src = bufs[dst];
    dst ^= 1;
  }
  HIPCK(hipGetLastError());
  return 0;
}
// The keys are compressed curve points, i.e. their leading bytes are as good as random (the first byte carries ~5 bits: the
// flag bits and the top of a 381-bit coordinate): sort on a prefix only and check that no two neighbours tie there; only if
// they do (duplicate keys, adversarial prefixes) sort again on every byte.  A pass per byte, so the prefix is as short as
// keeps a tie among honest keys below 2^-10 per call: 2 log2(n) + 13 bits -- six bytes at 65,536 keys (eight cost 0.17 ms more).
// Leaves the permutation in w.perm_a, the sorted concatenation in the pinned host buffer (c->hpin) and synchronises.
int keysort_prefix(size_t n) {
  int lg = 0;
  while (((size_t)1 << lg) < n) lg++;
  int b = (2 * lg + 13 + 7) / 8;
  if (b < 4) b = 4;
  if (b > 8) b = 8;
  return b;
}
int run_key_sort_to_host(Ctx* c, const uint8_t* d_kb, size_t n, size_t width, keysort_ws& w, hipEvent_t ev_ready, bool* used_full) {
  int rc = pinned_reserve(c, width * n + 64);
  if (rc) return rc;
  uint32_t* h_flag = (uint32_t*)(c->hpin + ((width * n + 63) & ~(size_t)63));
  for (int attempt = 0; attempt < 2; attempt++) {
    const int nbytes = attempt == 0 ? keysort_prefix(n) : (int)width;
    if ((rc = run_key_sort_passes(c, d_kb, n, width, nbytes, w))) return rc;
    HIPCK(hipMemsetAsync(w.flag, 0, 4, c->stream));
    if (attempt == 0)
      KL(KID_KEY_SORT, k_keys_tie_flag, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_kb, width, (size_t)keysort_prefix(n), (const uint32_t*)w.perm_a, w.flag);
    KL(KID_KEY_SORT, k_keys_gather, dim3(blocks_for(n * (width / 4))), dim3(BLS_BLOCK), n, d_kb, width, (const uint32_t*)w.perm_a, w.sorted);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(c->hpin, w.sorted, width * n, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(h_flag, w.flag, 4, hipMemcpyDeviceToHost, c->stream));
    if (ev_ready && attempt == 0) {
      HIPCK(hipEventRecord(ev_ready, c->stream));
      return 0;                       // the caller enqueues more work, then calls run_key_sort_finish
    }
    HIPCK(hipStreamSynchronize(c->stream));
    if (*h_flag == 0) break;
    if (used_full) *used_full = true;
  }
  return 0;
}
// second half of the overlapped form: wait for the prefix-sorted bytes; redo with the full sort when the prefix tied
int run_key_sort_finish(Ctx* c, const uint8_t* d_kb, size_t n, size_t width, keysort_ws& w, hipEvent_t ev_ready, bool* used_full) {
  HIPCK(hipEventSynchronize(ev_ready));
  const uint32_t* h_flag = (const uint32_t*)(c->hpin + ((width * n + 63) & ~(size_t)63));
  if (*h_flag == 0) return 0;
  if (used_full) *used_full = true;
  int rc = run_key_sort_passes(c, d_kb, n, width, (int)width, w);
  if (rc) return rc;
  KL(KID_KEY_SORT, k_keys_gather, dim3(blocks_for(n * (width / 4))), dim3(BLS_BLOCK), n, d_kb, width, (const uint32_t*)w.perm_a, w.sorted);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(c->hpin, w.sorted, width * n, hipMemcpyDeviceToHost, c->stream));
  HIPCK(hipStreamSynchronize(c->stream));
  return 0;
}
// H = SHA-256(sorted key bytes): ONE sequential hash stream (reference :45-59), which is why it runs on a host core
// (SHA-NI: ~2 GB/s; a GPU lane would need ~100 ms for it)
void keys_digest_host(const uint8_t* sorted, size_t bytes, uint8_t H[32]) {
  host_sha256 h;
  h.update(sorted, bytes);
  h.final(H);
}
// t_p for every sorted position p on the device.  sorted_order: d_scal[p]; else d_scal[perm[p] - base] for keys of the shard
int run_coefficients(Ctx* c, const uint8_t* d_H, const uint32_t* d_perm, size_t n, size_t base, size_t count, int sorted_order,
                     uint8_t* d_scal, int32_t* d_zero_flag) {
  KL(KID_COEFF, k_sha256_coeff, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_H, d_perm, base, count, sorted_order, d_scal, d_zero_flag);
  HIPCK(hipGetLastError());
  return 0;
}

// ---- secure aggregation of ONE key set (blsgpu_aggregate_secure, and the large sets of blsgpu_aggregate_secure_batch): from the set's
// serialised keys d_bytes and its signatures d_sigs to sum_p t_p sig[idx_p] in d_part[0] (d_part: T records).  Device sort, host
// SHA-256 of the sorted stream, the coefficients in sorted order, idx_p = the FIRST input position holding the key of sorted
// position p (the reference's `position` search: the sort is stable, so that is the input index at the start of p's run of equal
// keys), one weighted point sum.  A zero coefficient ORs 1 into *d_zero.  Synchronises the stream (the sort); its workspace comes
// from the arena (aggregate_secure_set_bytes).
size_t aggregate_secure_set_bytes(size_t n, size_t width) {
  return 2 * pad256(4 * n) + pad256(4 * scan_tiles(n)) + pad256(32 * n) + 256 + msm_ws_bytes(n) + keysort_ws_bytes(n, width);
}
int run_aggregate_secure_set(Ctx* c, int sig_group, const uint8_t* d_bytes, const uint8_t* d_sigs, size_t n, size_t width, int fmt, int32_t* d_zero,
                             uint8_t* d_part, size_t T) {
  Carver mem{c};
  uint32_t* d_idx = mem.take<uint32_t>(4 * n);
  uint32_t* d_start = mem.take<uint32_t>(4 * n);
  uint32_t* d_tiles = mem.take<uint32_t>(4 * scan_tiles(n));
  uint8_t* d_scal = mem.take<uint8_t>(32 * n);
  uint8_t* d_H = mem.take<uint8_t>(64);
  keysort_ws w;
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  int rc = keysort_ws_take(c, n, width, w);
  if (rc) return rc;
  if ((rc = run_key_sort_to_host(c, d_bytes, n, width, w, nullptr, nullptr))) return rc;
  uint8_t H[32];
  keys_digest_host(c->hpin, width * n, H);
  if ((rc = h2d_small(c, d_H, H, 32))) return rc;
  if ((rc = run_coefficients(c, d_H, w.perm_a, n, 0, n, 1, d_scal, d_zero))) return rc;
  KL(KID_KEY_SORT, k_keys_run_start, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_bytes, width, (const uint32_t*)w.perm_a, d_start);
  if ((rc = run_scan_max_u32(c, KID_KEY_SORT, n, d_start, d_tiles))) return rc;
  KL(KID_KEY_SORT, k_run_first_index, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint32_t*)w.perm_a, (const uint32_t*)d_start, d_idx);
  HIPCK(hipGetLastError());
  return with_group(sig_group, [&](auto G) { return run_point_sum<G()>(c, d_sigs, fmt, d_scal, d_idx, n, d_part, T); });
}

// ---- Basic's duplicate-message rule on device-resident messages (util_kernels.cuh) -> d_out2 = (old, i) or (~0, ~0)
size_t dup_ws_bytes(size_t n) {
  size_t cap = 64;
  while (cap < 2 * n) cap <<= 1;
  return 2 * pad256(4 * cap) + pad256(4 * n) + 1024;
}
int run_first_duplicate(Ctx* c, const uint8_t* d_msgs, const uint64_t* d_offs, size_t n, uint64_t* d_out2) {
  if (n >= 0xffffffffull) return fail(BLSGPU_E_ARG, "more than 2^32 - 2 messages");
  size_t cap = 64;
  while (cap < 2 * n) cap <<= 1;
  Carver mem{c};
  uint32_t* tab = mem.take<uint32_t>(4 * cap);
  uint32_t* minidx = mem.take<uint32_t>(4 * cap);
  uint32_t* slot_of = mem.take<uint32_t>(4 * (n ? n : 1));
  uint32_t* best = mem.take<uint32_t>(64);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  HIPCK(hipMemsetAsync(tab, 0xff, 4 * cap, c->stream));
  HIPCK(hipMemsetAsync(minidx, 0xff, 4 * cap, c->stream));
  HIPCK(hipMemsetAsync(best, 0xff, 4, c->stream));
  if (n) {
    KL(KID_DUP, k_dup_insert, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_msgs, d_offs, (uint32_t)(cap - 1), tab, minidx, slot_of);
    KL(KID_DUP, k_dup_find, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint32_t*)slot_of, (const uint32_t*)minidx, best);
  }
  KL(KID_DUP, k_dup_fin, dim3(1), dim3(BLS_BLOCK), (const uint32_t*)best, (const uint32_t*)slot_of, (const uint32_t*)minidx, d_out2);
  HIPCK(hipGetLastError());
  return 0;
}

template <int G>
size_t keyset_table_bytes_g(size_t n) { return n * (size_t)keyset_shape<G>::POINTS * 2 * G * FP_NL * 4; }
size_t keyset_table_bytes(int group, size_t n) { return group == 1 ? keyset_table_bytes_g<1>(n) : keyset_table_bytes_g<2>(n); }

// ---- registered sets (keyset.cuh, msgset.cuh, sigset.cuh): the records and the registry.  A handle is an id, never a pointer: a
// stale one is simply not found.  The three kinds have a map each and share one mutex and one id counter, so a handle of one kind
// is never found as another.  A call works on a copy of the record taken under the lock (set_find).  An update rewrites entries
// behind unchanged pointers; an append moves the arrays and replaces the record under the lock (set_publish), freeing an old array
// only after a record that no longer names it has been published.  Neither waits for calls that hold a copy: running one while
// another thread updates, appends to or destroys the same set is the caller's error.
struct DevSet {
  int sig_group = 0;
  int flags = 0;                      // BLSGPU_{KEYSET,MSGSET,SIGSET}_* the creator asked for (what is built: table, lines)
  size_t n = 0, devidx = 0;
  int dev = -1;
  uint8_t* aff = nullptr;             // RAW_AFFINE records of the entries
  uint32_t* lines = nullptr;          // their rows (entries in G2, the kind's LINES flag; or none) ...
  int32_t* nolines = nullptr;         // ... and per entry 0 or KEYSET_NOLINES_*
  uint64_t bytes = 0;
};
struct KeySet : DevSet {
  int group = 0;                      // where the keys live
  uint8_t *comp = nullptr, *table = nullptr;     // Modern bytes, fixed-base tables (or none)
  int32_t* status = nullptr;
};
struct MsgSet : DevSet {              // aff: the hashed messages (group sig_group)
  int scheme = 0;
};
struct SigSet : DevSet {              // aff: the signatures (group sig_group)
  uint8_t* tags = nullptr;            // their scheme tags
  int32_t* status = nullptr;          // their creation statuses
};
std::mutex g_sets_mu;
uint64_t g_sets_next = 1;
std::unordered_map<uint64_t, KeySet> g_keysets;       // all three under g_sets_mu
std::unordered_map<uint64_t, MsgSet> g_msgsets;
std::unordered_map<uint64_t, SigSet> g_sigsets;

// what a kind states about itself: its map, its name and its entries' noun in messages, the arrays that hold one record per entry
// (with a record's bytes), the group its rows need to be 2 and the flag that asks for them; a key set alone has tables, which
// share the rows' cap
struct SetArray {
  void** p;
  size_t entry_bytes;
};
std::unordered_map<uint64_t, KeySet>& set_map(const KeySet&) { return g_keysets; }
std::unordered_map<uint64_t, MsgSet>& set_map(const MsgSet&) { return g_msgsets; }
std::unordered_map<uint64_t, SigSet>& set_map(const SigSet&) { return g_sigsets; }
const char* set_name(const KeySet&) { return "key set"; }
const char* set_name(const MsgSet&) { return "message set"; }
const char* set_name(const SigSet&) { return "signature set"; }
const char* set_noun(const KeySet&) { return "keys"; }
const char* set_noun(const MsgSet&) { return "messages"; }
const char* set_noun(const SigSet&) { return "signatures"; }
std::vector<SetArray> set_arrays(KeySet& k) {
  return {{(void**)&k.aff, point_bytes(k.group, BLSGPU_FMT_RAW_AFFINE)}, {(void**)&k.comp, point_bytes(k.group, BLSGPU_FMT_COMPRESSED)}, {(void**)&k.status, 4}};
}
std::vector<SetArray> set_arrays(MsgSet& m) { return {{(void**)&m.aff, point_bytes(m.sig_group, BLSGPU_FMT_RAW_AFFINE)}}; }
std::vector<SetArray> set_arrays(SigSet& s) {
  return {{(void**)&s.aff, point_bytes(s.sig_group, BLSGPU_FMT_RAW_AFFINE)}, {(void**)&s.tags, 1}, {(void**)&s.status, 4}};
}
int set_rows_group(const DevSet& s) { return s.sig_group; }
int set_rows_group(const KeySet& k) { return k.group; }
int set_rows_flag(const KeySet&) { return BLSGPU_KEYSET_LINES; }
int set_rows_flag(const MsgSet&) { return BLSGPU_MSGSET_LINES; }
int set_rows_flag(const SigSet&) { return BLSGPU_SIGSET_LINES; }
void* set_table(const DevSet&) { return nullptr; }
void* set_table(const KeySet& k) { return k.table; }
uint64_t set_other_bytes(const DevSet&, size_t) { return 0; }          // what shares the cap of keyset_lines_fit with n entries' rows
uint64_t set_other_bytes(const KeySet& k, size_t n) { return k.table ? keyset_table_bytes(k.group, n) : 0; }

// device_bytes of a set as it stands: the records, the tables and the rows with their per-entry words
template <class T>
uint64_t set_bytes(const T& s) {
  uint64_t per_entry = s.lines ? KEYSET_LINES_KEY_BYTES + 4 : 0;
  for (const SetArray& a : set_arrays(const_cast<T&>(s))) per_entry += a.entry_bytes;
  return per_entry * s.n + set_other_bytes(s, s.n);
}
template <class T>
void set_free(T& s) {
  if (s.dev >= 0) (void)hipSetDevice(s.dev);
  for (const SetArray& a : set_arrays(s))
    if (*a.p) (void)hipFree(*a.p);
  for (void* p : {(void*)s.lines, (void*)s.nolines, set_table(s)})
    if (p) (void)hipFree(p);
  s = T();
}
template <class T>
void set_release_all() {
  std::lock_guard<std::mutex> lk(g_sets_mu);
  auto& map = set_map(T());
  for (auto& kv : map) set_free(kv.second);
  map.clear();
}
template <class T>
int set_find(uint64_t handle, T& s, bool take = false) {       // take: the record leaves the registry (destroy)
  if (!initialised()) return NOT_INIT();
  std::lock_guard<std::mutex> lk(g_sets_mu);
  auto& map = set_map(s);
  auto it = map.find(handle);
  if (handle == 0 || it == map.end()) return fail(BLSGPU_E_ARG, std::string("unknown ") + set_name(s) + " handle (never issued, or destroyed)");
  s = it->second;
  if (take) map.erase(it);
  return 0;
}
// the record of a live set after an append moved its arrays; a handle destroyed meanwhile (the caller's error) stays gone
template <class T>
void set_publish(uint64_t handle, const T& s) {
  std::lock_guard<std::mutex> lk(g_sets_mu);
  auto& map = set_map(s);
  auto it = map.find(handle);
  if (it != map.end()) it->second = s;
}
template <class T>
uint64_t set_issue(const T& s) {
  std::lock_guard<std::mutex> lk(g_sets_mu);
  const uint64_t id = g_sets_next++;
  set_map(s)[id] = s;
  return id;
}
template <class T>
int set_destroy(uint64_t handle) {
  T s;
  int rc = set_find(handle, s, true);
  if (rc) return rc;
  set_free(s);
  return 0;
}

}  // namespace

// =========================================================================================================
extern "C" {

// binds one device: a pool of contexts on it
static int bind_device(int device, int ndev) {
  if (device >= ndev) return fail(BLSGPU_E_ARG, "device ordinal out of range");
  HIPCK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCK(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    return fail(BLSGPU_E_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 (MI355X) only");
  const int nctx = (int)knobs().contexts;   // contexts per device (BLSGPU_CONTEXTS, default 2, 1..16): concurrent callers beyond this queue up
  Device* d = new Device();
  d->dev = device;
  for (int k = 0; k < nctx; k++) {
    Ctx* c = new Ctx();
    c->dev = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) {
      e = hipHostMalloc((void**)&c->hsmall, HSMALL_BYTES, hipHostMallocDefault);
      if (e != hipSuccess) (void)hipStreamDestroy(c->stream);
    }
    if (e == hipSuccess) {
      // the hand-over flags of the single-verdict kernels (stream_epoch_next): here, not on first use -- an allocation inside a
      // call costs that call a few hundred microseconds
      const size_t fb = (size_t)WPOST2_MAX_ITEMS * WSTREAM_FLAGS * 4;
      e = hipMalloc((void**)&c->stream_flags, fb);
      if (e == hipSuccess) e = hipMemset(c->stream_flags, 0, fb);
      if (e == hipSuccess) c->stream_epoch = 1;         // cleared: the first launch publishes with 2
      if (e != hipSuccess) {
        if (c->stream_flags) (void)hipFree(c->stream_flags);
        (void)hipHostFree(c->hsmall);
        (void)hipStreamDestroy(c->stream);
      }
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      delete c;
      for (Ctx* q : d->pool) {
        (void)hipStreamDestroy(q->stream);
        (void)hipHostFree(q->hsmall);
        (void)hipFree(q->stream_flags);
        delete q;
      }
      delete d;
      return fail(BLSGPU_E_HIP, std::string("creating a context (stream / pinned memory): ") + hipGetErrorString(e));
    }
    d->pool.push_back(c);
  }
  g_devices.push_back(d);
  return 0;
}

static void release_devices() {
  for (Device* d : g_devices) {
    (void)hipSetDevice(d->dev);
    for (Ctx* c : d->pool) {
      std::lock_guard<std::mutex> lk(c->mu);   // waits for a call in flight on this context
      (void)hipStreamSynchronize(c->stream);
      if (c->arena) (void)hipFree(c->arena);
      if (c->lines_ws) (void)hipFree(c->lines_ws);
      if (c->fold_ws) (void)hipFree(c->fold_ws);
      if (c->stream_flags) (void)hipFree(c->stream_flags);
      if (c->ev_tail_fork) (void)hipEventDestroy(c->ev_tail_fork);
      if (c->ev_tail_join) (void)hipEventDestroy(c->ev_tail_join);
      if (c->tail) (void)hipStreamDestroy(c->tail);
      if (c->ev_host) (void)hipEventDestroy(c->ev_host);
      if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
      if (c->ev_join) (void)hipEventDestroy(c->ev_join);
      if (c->ev_join2) (void)hipEventDestroy(c->ev_join2);
      if (c->side2) (void)hipStreamDestroy(c->side2);
      if (c->side) (void)hipStreamDestroy(c->side);
      if (c->hpin) (void)hipHostFree(c->hpin);
      if (c->hsmall) (void)hipHostFree(c->hsmall);
      for (hipEvent_t e : c->prof_pool) (void)hipEventDestroy(e);
      (void)hipStreamDestroy(c->stream);
    }
  }
  for (Device* d : g_devices) {
    for (Ctx* c : d->pool) delete c;
    delete d;
  }
  g_devices.clear();
}

// BLSGPU_STRICT_ENV=1: refuse to start over an environment the knob table does not fully understand (before any device is touched)
static int strict_env_check() {
  if (!initialised()) g_knobs = parse_knobs();
  const Knobs& k = knobs();
  if (k.strict_env && !k.problem.empty()) return fail(BLSGPU_E_ARG, "BLSGPU_STRICT_ENV: " + k.problem);
  return 0;
}
int blsgpu_init(int device) try {
  std::lock_guard<std::mutex> lk(g_init_mu);
  if (int rc = strict_env_check()) return rc;
  if (initialised()) {
    if (device >= 0 && device != g_devices[0]->dev)
      return fail(BLSGPU_E_ARG, "blsgpu_init: the library is already bound to device " + std::to_string(g_devices[0]->dev) +
                                    " (call blsgpu_shutdown first to rebind)");
    return 0;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    return fail(BLSGPU_E_NO_DEVICE, "no HIP device available: libblsgpu has no CPU fallback");
  }
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess) device = 0;
  }
  return bind_device(device, ndev);
}
API_CATCH

/* One process driving several GPUs of the node (the in-library alternative to one process per GPU): binds the
 * first ndev visible devices (ndev <= 0: all of them).  The four verify entry points then shard their items over the
 * bound devices (contiguous ranges, one host thread per device) and fold the per-device partial results -- key sums,
 * Fp12 Miller products, MSM partials -- on device 0, exactly as the one-process-per-GPU path does over RCCL.
 * BLSGPU_FAKE_DEVICES=k (testing on a one-GPU box) binds k logical devices that all map to the one physical GPU. */
int blsgpu_init_devices(int ndev_req) try {
  std::lock_guard<std::mutex> lk(g_init_mu);
  if (int rc = strict_env_check()) return rc;
  if (initialised()) {
    if (ndev_req > 0 && (size_t)ndev_req != g_devices.size())
      return fail(BLSGPU_E_ARG, "blsgpu_init_devices: the library is already bound to " + std::to_string(g_devices.size()) +
                                    " device(s) (call blsgpu_shutdown first to rebind)");
    return (int)g_devices.size();
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    return fail(BLSGPU_E_NO_DEVICE, "no HIP device available: libblsgpu has no CPU fallback");
  }
  const int fake = (int)knobs().fake_devices;
  int want = ndev_req > 0 ? ndev_req : (fake > 0 ? fake : ndev);
  if (fake <= 0 && want > ndev) return fail(BLSGPU_E_ARG, "blsgpu_init_devices: more devices requested than visible");
  if (want > 64) return fail(BLSGPU_E_ARG, "blsgpu_init_devices: at most 64 devices");
  for (int k = 0; k < want; k++) {
    int rc = bind_device(fake > 0 ? k % ndev : k, ndev);
    if (rc) {
      release_devices();
      return rc;
    }
  }
  // peer access so that a device can read a shard that lives on another device's memory (xGMI loads); failures are not
  // fatal: shards of host buffers never need it
  g_peer_ok = true;
  for (size_t a = 0; a < g_devices.size(); a++)
    for (size_t b = 0; b < g_devices.size(); b++) {
      if (g_devices[a]->dev == g_devices[b]->dev) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, g_devices[a]->dev, g_devices[b]->dev) == hipSuccess && can) {
        (void)hipSetDevice(g_devices[a]->dev);
        hipError_t pe = hipDeviceEnablePeerAccess(g_devices[b]->dev, 0);
        if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) g_peer_ok = false;
        if (pe != hipSuccess) (void)hipGetLastError();
      } else {
        g_peer_ok = false;
      }
    }
  (void)hipSetDevice(g_devices[0]->dev);
  return (int)g_devices.size();
}
API_CATCH

int blsgpu_device_count(void) { return (int)g_devices.size(); }

void blsgpu_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_init_mu);
  if (!initialised()) return;
  set_release_all<KeySet>();
  set_release_all<MsgSet>();
  set_release_all<SigSet>();
  release_devices();
}

int blsgpu_profile_enable(int on) try {
  if (!initialised()) return NOT_INIT();
  for (Device* d : g_devices)
    for (Ctx* c : d->pool) {
      std::lock_guard<std::mutex> lk(c->mu);
      c->prof_on = on != 0;
      for (int k = 0; k < KID_COUNT; k++) {
        c->prof_ms[k] = 0;
        c->prof_cnt[k] = 0;
      }
    }
  return 0;
}
API_CATCH
int blsgpu_profile_count(void) { return KID_COUNT; }
int blsgpu_profile_get(int kernel_id, char* name, size_t name_cap, double* total_ms, uint64_t* launches) try {
  if (!initialised()) return NOT_INIT();
  if (kernel_id < 0 || kernel_id >= KID_COUNT) return fail(BLSGPU_E_ARG, "kernel id out of range");
  if (name && name_cap) {
    strncpy(name, KID_NAMES[kernel_id], name_cap - 1);
    name[name_cap - 1] = 0;
  }
  double ms = 0;
  uint64_t cnt = 0;
  for (Device* d : g_devices)
    for (Ctx* c : d->pool) {
      std::lock_guard<std::mutex> lk(c->mu);
      ms += c->prof_ms[kernel_id];
      cnt += c->prof_cnt[kernel_id];
    }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = cnt;
  return 0;
}
API_CATCH

size_t blsgpu_last_error(char* buf, size_t cap) {
  if (buf && cap) {
    size_t k = std::min(cap - 1, t_err.size());
    memcpy(buf, t_err.data(), k);
    buf[k] = 0;
  }
  return t_err.size();
}

int blsgpu_verify_batch(int sig_group, int scheme, const void* pks, const void* sigs, const uint8_t* msgs,
                        const uint64_t* msg_offsets, size_t n, int fmt, int32_t* status) try {
  const bool wire = fmt == BLSGPU_FMT_COMPRESSED || fmt == BLSGPU_FMT_LEGACY;
  int rc = check_common(sig_group, scheme, wire ? BLSGPU_FMT_RAW_PROJ : fmt);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!pks || !sigs || !msg_offsets || !status) return fail(BLSGPU_E_ARG, "null argument");
  if (const size_t D = shard_devices(n, {pks, sigs, msgs, msg_offsets, status}); D > 1) {
    // independent items: contiguous ranges per device, no exchange at all (message offsets are absolute, so every shard
    // passes the whole blob and its own window of the offsets)
    const size_t psz = pk_size(sig_group, fmt), ssz = sig_size(sig_group, fmt);
    return run_on_devices(D, [&](size_t d) {
      const size_t lo = n * d / D, hi = n * (d + 1) / D;
      return blsgpu_verify_batch(sig_group, scheme, (const uint8_t*)pks + lo * psz, (const uint8_t*)sigs + lo * ssz, msgs, msg_offsets + lo, hi - lo,
                                 fmt, status + lo);
    });
  }
  CTX_ACQUIRE(c);
  // total message bytes: last offset (read it from wherever it lives)
  uint64_t total = 0;
  if (is_device_ptr(msg_offsets)) HIPCK(hipMemcpy(&total, msg_offsets + n, 8, hipMemcpyDeviceToHost));
  else total = msg_offsets[n];
  const size_t pkb = pk_size(sig_group, fmt) * n, sgb = sig_size(sig_group, fmt) * n;
  size_t need = pad256(pkb) + pad256(sgb) + pad256(total) + pad256(8 * (n + 1)) + pad256(4 * n) + 2 * pad256((size_t)WS_PAIRS_WORDS * 4 * n) + 4096 +
                (wire ? pad256(288 * n) + pad256(144 * n) : 0);
  rc = arena_reserve(c, need);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_pks, *d_sigs, *d_msgs, *d_offs;
  {
    const void* ptrs[4] = {pks, sigs, msgs, msg_offsets};
    const size_t sizes[4] = {pkb, sgb, (size_t)total, 8 * (n + 1)};
    const void* outs[4];
    if (stage_in_packed(c, ptrs, sizes, outs, 4)) {
      d_pks = outs[0];
      d_sigs = outs[1];
      d_msgs = outs[2];
      d_offs = outs[3];
    } else {
      if ((rc = stage_in(c, pks, pkb, &d_pks))) return rc;
      if ((rc = stage_in(c, sigs, sgb, &d_sigs))) return rc;
      if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
      if ((rc = stage_in(c, msg_offsets, 8 * (n + 1), &d_offs))) return rc;
    }
  }
  Carver mem{c};
  int32_t* d_status = mem.take<int32_t>(4 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIRS_WORDS * 4 * n);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  int pre = 0, kfmt = fmt;
  if (wire) {
    // wire ingest: PublicKey / Signature from_bytes[_with_mode] -- checked decompression incl. subgroup
    // test, reference src/public_key.rs:58-74,158-171, src/signature.rs:231-253, src/impls/legacy.rs:100-170.
    // A decode failure is the item's status (key first, then signature), exactly what a caller that deserialises
    // before verifying would have seen.
    uint8_t* d_pk_raw = (uint8_t*)arena_take(c, pk_size(sig_group, BLSGPU_FMT_RAW_PROJ) * n);
    uint8_t* d_sig_raw = (uint8_t*)arena_take(c, sig_size(sig_group, BLSGPU_FMT_RAW_PROJ) * n);
    if (!d_pk_raw || !d_sig_raw) return fail(BLSGPU_E_HIP, "internal: arena too small");
    const int legacy = fmt == BLSGPU_FMT_LEGACY;
    with_group(key_group(sig_group), [&](auto KG) {
      KL(KID_DECOMPRESS, k_decompress<KG()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_pks, legacy, d_pk_raw, d_status, 0);
      KL(KID_DECOMPRESS, k_decompress<3 - KG()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_sigs, legacy, d_sig_raw, d_status, 1);
    });
    d_pks = d_pk_raw;
    d_sigs = d_sig_raw;
    pre = 1;
    kfmt = BLSGPU_FMT_RAW_PROJ;
  }
  rc = run_verify_items(c, sig_group, scheme == BLSGPU_SCHEME_AUG, (const uint8_t*)d_pks, (const uint8_t*)d_sigs, kfmt,
                        (const uint8_t*)d_msgs, (const uint64_t*)d_offs, 0, scheme_dst(sig_group, scheme), n, d_pairs, d_f, d_status, pre);
  if (rc) return rc;
  if ((rc = status_out_and_sync(c, status, d_status, n))) return rc;
  return 0;
}
API_CATCH

/* Opt-in grouped verification of independent items (Bls12381G1Impl): groups of GROUPED_ITEMS items share one final
 * exponentiation through a random linear combination (csrc/kernels.cuh k_prepare_grouped); every group that fails -- and only
 * those -- is re-verified item by item with the kernels of blsgpu_verify_batch, so the status vector equals that call's except
 * that an invalid item whose group passes the combined check (probability below 2^-64 per group, over the seed) is reported
 * valid.  seed: the generator of the per-item scalars; the same seed gives the same run. */
int blsgpu_verify_batch_grouped(int sig_group, int scheme, const void* pks, const void* sigs, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n,
                                int fmt, uint64_t seed, int32_t* status) try {
  int rc = check_common(sig_group, scheme, fmt);
  if (rc) return rc;
  if (sig_group != 1) return fail(BLSGPU_E_ARG, "grouped verification is built for sig_group 1 (Bls12381G1Impl)");
  if (n == 0) return 0;
  if (!pks || !sigs || !msg_offsets || !status) return fail(BLSGPU_E_ARG, "null argument");
  if (n >= 0xffffffffull) return fail(BLSGPU_E_ARG, "more than 2^32 - 2 items");
  CTX_ACQUIRE(c);
  std::vector<uint64_t> offs_h(n + 1);
  if (is_device_ptr(msg_offsets)) HIPCK(hipMemcpy(offs_h.data(), msg_offsets, 8 * (n + 1), hipMemcpyDeviceToHost));
  else memcpy(offs_h.data(), msg_offsets, 8 * (n + 1));
  const uint64_t total = offs_h[n];
  const size_t psz = pk_size(1, fmt), ssz = sig_size(1, fmt), pkb = psz * n, sgb = ssz * n;
  const size_t ng = (n + GROUPED_ITEMS - 1) / GROUPED_ITEMS, m = (GROUPED_ITEMS + 1) * ng;
  const size_t need = 2 * (pad256(pkb) + pad256(sgb) + pad256(total) + pad256(8 * (n + 1))) + 3 * pad256(4 * n) + pad256(144 * n) +
                      pad256((size_t)WS_PAIR1_WORDS * 4 * m) + pad256((size_t)WS_F_WORDS * 4 * m) + pad256(4 * m) + pad256((size_t)WS_F_WORDS * 4 * ng) +
                      pad256(4 * ng) + 2 * pad256((size_t)WS_PAIRS_WORDS * 4 * n) + 16384;
  if ((rc = arena_reserve(c, need))) return rc;
  c->arena_off = 0;
  const void *d_pks, *d_sigs, *d_msgs, *d_offs;
  if ((rc = stage_in(c, pks, pkb, &d_pks))) return rc;
  if ((rc = stage_in(c, sigs, sgb, &d_sigs))) return rc;
  if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
  if ((rc = stage_in(c, msg_offsets, 8 * (n + 1), &d_offs))) return rc;
  Carver mem{c};
  int32_t* d_status = mem.take<int32_t>(4 * n);
  uint8_t* d_scaled = mem.take<uint8_t>(144 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIR1_WORDS * 4 * m);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * m);
  int32_t* d_skip = mem.take<int32_t>(4 * m);
  uint32_t* d_fg = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * ng);
  int32_t* d_gst = mem.take<int32_t>(4 * ng);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  const int aug = scheme == BLSGPU_SCHEME_AUG;
  const dst_arg dst = scheme_dst(1, scheme);
  HIPCK(hipMemsetAsync(d_skip, 0xff, 4 * m, c->stream));
  HIPCK(hipMemsetAsync(d_gst, 0, 4 * ng, c->stream));
  KL(KID_PREPARE, k_prepare_grouped<1>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_pks, (const uint8_t*)d_sigs, fmt, aug, (const uint8_t*)d_msgs,
     (const uint64_t*)d_offs, dst, (uint64_t)seed, ng, d_pairs, d_skip, d_scaled, d_status);
  KL(KID_ACCUM, k_group_sigsum, dim3(blocks_for(ng)), dim3(BLS_BLOCK), ng, n, (const uint8_t*)d_scaled, d_pairs, d_skip);
  MILLER1_LAUNCH(m, m, d_pairs, d_skip, d_f);
  KL(KID_F12_FOLD, k_f12_mul3, dim3(blocks_for(ng)), dim3(BLS_BLOCK), ng, (const uint32_t*)d_f, m, d_fg);
  KL(KID_FINALEXP_V1, k_finalexps, dim3(blocks_for(2 * ng)), dim3(BLS_BLOCK), ng, (const uint32_t*)d_fg, d_gst);
  HIPCK(hipGetLastError());
  std::vector<int32_t> gst(ng);
  HIPCK(hipMemcpyAsync(gst.data(), d_gst, 4 * ng, hipMemcpyDeviceToHost, c->stream));
  HIPCK(hipStreamSynchronize(c->stream));
  // the groups that failed: their items once more, one by one (identity failures keep the status they already have: the
  // per-item kernels find the same)
  std::vector<uint32_t> idx;
  for (size_t g = 0; g < ng; g++)
    if (gst[g] != BLS_OK)
      for (size_t i = g * GROUPED_ITEMS; i < n && i < (g + 1) * GROUPED_ITEMS; i++) idx.push_back((uint32_t)i);
  if (!idx.empty()) {
    const size_t cnt = idx.size();
    std::vector<uint64_t> offs2(cnt + 1);
    offs2[0] = 0;
    for (size_t j = 0; j < cnt; j++) offs2[j + 1] = offs2[j] + (offs_h[idx[j] + 1] - offs_h[idx[j]]);
    uint32_t* d_idx = mem.take<uint32_t>(4 * cnt);
    uint64_t* d_offs2 = mem.take<uint64_t>(8 * (cnt + 1));
    uint8_t* d_pks2 = mem.take<uint8_t>(psz * cnt);
    uint8_t* d_sigs2 = mem.take<uint8_t>(ssz * cnt);
    uint8_t* d_msgs2 = mem.take<uint8_t>(offs2[cnt] ? offs2[cnt] : 1);
    int32_t* d_st2 = mem.take<int32_t>(4 * cnt);
    uint32_t* d_pairs2 = mem.take<uint32_t>((size_t)WS_PAIRS_WORDS * 4 * cnt);
    uint32_t* d_f2 = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * cnt);
    if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
    HIPCK(hipMemcpyAsync(d_idx, idx.data(), 4 * cnt, hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemcpyAsync(d_offs2, offs2.data(), 8 * (cnt + 1), hipMemcpyHostToDevice, c->stream));
    KL(KID_COMPRESS, k_gather_rows, dim3(blocks_for(cnt * (psz / 4))), dim3(BLS_BLOCK), cnt, (const uint32_t*)d_idx, (const uint32_t*)d_pks, psz / 4, (uint32_t*)d_pks2);
    KL(KID_COMPRESS, k_gather_rows, dim3(blocks_for(cnt * (ssz / 4))), dim3(BLS_BLOCK), cnt, (const uint32_t*)d_idx, (const uint32_t*)d_sigs, ssz / 4, (uint32_t*)d_sigs2);
    KL(KID_COMPRESS, k_gather_ragged, dim3(blocks_for(cnt)), dim3(BLS_BLOCK), cnt, (const uint32_t*)d_idx, (const uint64_t*)d_offs, (const uint64_t*)d_offs2,
       (const uint8_t*)d_msgs, d_msgs2);
    HIPCK(hipGetLastError());
    if ((rc = run_verify_items(c, 1, aug, d_pks2, d_sigs2, fmt, d_msgs2, d_offs2, 0, dst, cnt, d_pairs2, d_f2, d_st2))) {
      (void)hipStreamSynchronize(c->stream);      // idx / offs2 are read by the copies above
      return rc;
    }
    KL(KID_COMPRESS, k_scatter_i32, dim3(blocks_for(cnt)), dim3(BLS_BLOCK), cnt, (const uint32_t*)d_idx, (const int32_t*)d_st2, d_status);
    HIPCK(hipGetLastError());
  }
  if ((rc = status_out_and_sync(c, status, d_status, n))) return rc;
  return 0;
}
API_CATCH

// aug_prefix: MultiSignature::verify under MessageAugmentation prefixes the (aggregated) key bytes
// (reference src/traits/sig_aug.rs:20-24); verify_secure_message_augmentation does NOT, it only switches the DST
// (reference src/secure_aggregation.rs:236-246).
// d_hash != nullptr: H(msg) (RAW_PROJ, device) has already been computed on this stream (verify_secure overlaps it with the
// host's coefficient derivation); msg is then unused.
static int verify_one_tail(Ctx* c, int sig_group, int scheme, int aug_prefix, const uint8_t* d_pk_proj, const void* sig, int fmt,
                           const uint8_t* msg, size_t msg_len, int32_t* status, const uint8_t* d_hash = nullptr) {
  int rc;
  // bring the signature to RAW_PROJ next to the key so one k_prepare call (single fmt) serves both
  const void* d_sig_in;
  if ((rc = stage_in(c, sig, sig_size(sig_group, fmt), &d_sig_in))) return rc;
  const void* d_msg = nullptr;
  if (!d_hash && (rc = stage_in(c, msg, msg_len, &d_msg))) return rc;
  const uint64_t offs_h[2] = {0, (uint64_t)msg_len};
  Carver mem{c};
  uint64_t* d_offs = mem.take<uint64_t>(16);
  int32_t* d_status = mem.take<int32_t>(4);
  uint32_t* d_pairs = mem.take<uint32_t>(WS_PAIRS_WORDS * 4);
  uint32_t* d_f = mem.take<uint32_t>(WS_F_WORDS * 4);
  uint8_t* d_sig_proj = mem.take<uint8_t>(288);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if ((rc = h2d_small(c, d_offs, offs_h, 16))) return rc;
  // normalise the signature to RAW_PROJ with a 1-point "sum"
  rc = with_group(sig_group, [&](auto G) { return run_point_sum<G()>(c, (const uint8_t*)d_sig_in, fmt, nullptr, nullptr, 1, d_sig_proj, 1); });
  if (rc) return rc;
  if (d_hash) {
    with_group(sig_group, [&](auto G) {
      KL(KID_PREPARE, k_prepare_hashed<G()>, dim3(1), dim3(BLS_BLOCK), (size_t)1, d_pk_proj, (const uint8_t*)d_sig_proj, d_hash, d_pairs, d_status, 0);
    });
    rc = run_pairing2(c, 1, d_pairs, d_f, d_status, pairs_walked(sig_group == 1 ? 1 : 0));
  } else {
    rc = run_verify_items(c, sig_group, aug_prefix, d_pk_proj, d_sig_proj, BLSGPU_FMT_RAW_PROJ, (const uint8_t*)d_msg, d_offs, 1,
                          scheme_dst(sig_group, scheme), 1, d_pairs, d_f, d_status);
  }
  if (rc) return rc;
  if ((rc = status_out_and_sync(c, status, d_status, 1))) return rc;
  return 0;
}

// The one core_verify at the end of MultiSignature::verify / verify_secure for Bls12381G1Impl when the message takes no key
// prefix, cut in time (k_pairing_pre / k_pairing_post): BEGIN runs on the side stream, beside the whole key sum -- the hash of
// the message, the signature's identity check, the Miller function of the (signature, -g2) pair; FINISH runs once the summed
// key exists: its identity check and affine form, its line coefficients, the other Miller function, the final exponentiation.
struct CutTail {
  uint32_t* rec = nullptr;
  int32_t* d_status = nullptr;
  int sg = 1;
};
static int cut_tail_begin(Ctx* c, int sig_group, int scheme, const void* sig, int fmt, const uint8_t* msg, size_t msg_len, CutTail& t) {
  int rc;
  const void *d_sig, *d_msg0;
  t.sg = sig_group;
  if ((rc = stage_in(c, sig, sig_size(sig_group, fmt), &d_sig))) return rc;
  if ((rc = stage_in(c, msg, msg_len, &d_msg0))) return rc;
  Carver mem{c};
  uint64_t* d_offs0 = mem.take<uint64_t>(16);
  t.rec = mem.take<uint32_t>((size_t)WREC_WORDS * 4);
  t.d_status = mem.take<int32_t>(4);
  uint8_t* d_hash = mem.take<uint8_t>(288);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  const uint64_t offs0[2] = {0, (uint64_t)msg_len};
  if ((rc = h2d_small(c, d_offs0, offs0, 16))) return rc;
  if ((rc = side_fork(c))) return rc;
  if (sig_group == 1) {
    launch_hash_g1_small(c->side, 1, (const uint8_t*)d_msg0, (const uint64_t*)d_offs0, 1, scheme_dst(1, scheme), (uint8_t*)nullptr, t.rec);
    hipLaunchKernelGGL(k_prepare_keys<1>, dim3(1), dim3(BLS_BLOCK), 0, c->side2, (size_t)1, (const uint8_t*)nullptr, (const uint8_t*)d_sig,
                       (const uint8_t*)nullptr, fmt, 1, t.rec, t.d_status);
    hipLaunchKernelGGL(k_pairing_pre, dim3(1, 1), dim3(WIDE_ENGINE_BLOCK), 0, c->side2, (size_t)1, t.rec, (const int32_t*)t.d_status, 1, 1);
  } else {
    // Bls12381G2Impl: both G2 points are known now (H(m) after its hash, the signature at once): the side stream hashes and
    // derives the lines of H(m); the second one runs the signature's lines and the Miller function of (-g1, signature).  The
    // summed key is a G1 point and only scales lines: it enters in POST.
    hipLaunchKernelGGL(k_prepare_keys<2>, dim3(1), dim3(BLS_BLOCK), 0, c->side2, (size_t)1, (const uint8_t*)nullptr, (const uint8_t*)d_sig,
                       (const uint8_t*)nullptr, fmt, 1, t.rec, t.d_status);
    hipLaunchKernelGGL(k_pairing_pre, dim3(1, 1), dim3(WIDE_ENGINE_BLOCK), 0, c->side2, (size_t)1, t.rec, (const int32_t*)t.d_status, 2, 2);
    const hipError_t ea = hipEventRecord(c->ev_join2, c->side2);
    if (!launch_hash_g2_small(c->side, 1, (const uint8_t*)d_msg0, (const uint64_t*)d_offs0, 1, scheme_dst(2, scheme), d_hash, nullptr, t.rec))
      hipLaunchKernelGGL(k_prepare_keys<2>, dim3(1), dim3(BLS_BLOCK), 0, c->side, (size_t)1, (const uint8_t*)nullptr, (const uint8_t*)nullptr,
                         (const uint8_t*)d_hash, 0, 4, t.rec, t.d_status);
    const hipError_t eb = hipStreamWaitEvent(c->side, c->ev_join2, 0);      // the lines of H(m) read the status the signature part set
    hipLaunchKernelGGL(k_pairing_pre, dim3(1, 1), dim3(WIDE_ENGINE_BLOCK), 0, c->side, (size_t)1, t.rec, (const int32_t*)t.d_status, 0, 0);
    if (ea != hipSuccess || eb != hipSuccess) {
      (void)hipStreamSynchronize(c->side);
      (void)hipStreamSynchronize(c->side2);
      return fail(BLSGPU_E_HIP, "side-stream launch failed");
    }
  }
  const hipError_t e1 = hipGetLastError(), e2 = hipEventRecord(c->ev_join, c->side), e3 = hipEventRecord(c->ev_join2, c->side2);
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
    (void)hipStreamSynchronize(c->side);
    (void)hipStreamSynchronize(c->side2);
    return fail(BLSGPU_E_HIP, "side-stream launch failed");
  }
  return 0;
}
// rc: the caller's error so far (the side streams are joined either way: their kernels read the arena)
static int cut_tail_finish(Ctx* c, int rc, const uint8_t* d_pk_proj, CutTail& t, int32_t* status) {
  const hipError_t e = hipStreamWaitEvent(c->stream, c->ev_join, 0), e2 = hipStreamWaitEvent(c->stream, c->ev_join2, 0);
  if (rc || e != hipSuccess || e2 != hipSuccess) {
    (void)hipStreamSynchronize(c->side);
    (void)hipStreamSynchronize(c->side2);
    return rc ? rc : fail(BLSGPU_E_HIP, "hipStreamWaitEvent failed");
  }
  if (t.sg == 1) {
    KL(KID_PREPARE, k_prepare_keys<1>, dim3(1), dim3(BLS_BLOCK), (size_t)1, d_pk_proj, (const uint8_t*)nullptr, (const uint8_t*)nullptr, BLSGPU_FMT_RAW_PROJ, 2,
       t.rec, t.d_status);
    // the summed key's lines beside the Miller loop that consumes them
    if ((rc = launch_lines_and_post(c, 1, t.rec, t.d_status))) {
      (void)hipStreamSynchronize(c->side);
      (void)hipStreamSynchronize(c->side2);
      return rc;
    }
  } else {
    KL(KID_PREPARE, k_prepare_keys<2>, dim3(1), dim3(BLS_BLOCK), (size_t)1, d_pk_proj, (const uint8_t*)nullptr, (const uint8_t*)nullptr, BLSGPU_FMT_RAW_PROJ, 2,
       t.rec, t.d_status);
    if ((rc = launch_post(c, 1, t.rec, t.d_status))) {
      (void)hipStreamSynchronize(c->side);
      (void)hipStreamSynchronize(c->side2);
      return rc;
    }
  }
  HIPCK(hipGetLastError());
  if ((rc = status_out_and_sync(c, status, t.d_status, 1))) return rc;
  return 0;
}
static bool cut_tail_applies(int sig_group, int scheme) {
  (void)sig_group;
  return scheme != BLSGPU_SCHEME_AUG && wide_max_items() >= 1 && coop_max_items() >= 1;
}

int blsgpu_multi_verify(int sig_group, int scheme, const void* pks, size_t n, const void* sig, const uint8_t* msg,
                        size_t msg_len, int fmt, int32_t* status) try {
  int rc = check_common(sig_group, scheme, fmt);
  if (rc) return rc;
  if (!sig || !status || (n && !pks)) return fail(BLSGPU_E_ARG, "null argument");
  if (const size_t D = shard_devices(n, {pks, sig}); D > 1) {
    // per-device partial key sums (reference src/traits/pk_multi.rs:7-13 cut into ranges), then the fold and the one
    // verification on device 0: MultiSignature::verify over the D partial sums
    const size_t psz = pk_size(sig_group, fmt), osz = pk_size(sig_group, BLSGPU_FMT_RAW_PROJ);
    std::vector<uint8_t> parts(osz * D), sig_proj(288);
    if ((rc = run_on_devices(D, [&](size_t d) {
          const size_t lo = n * d / D, hi = n * (d + 1) / D;
          return (sig_group == 1 ? blsgpu_sum_g2 : blsgpu_sum_g1)((const uint8_t*)pks + lo * psz, hi - lo, fmt, parts.data() + osz * d);
        })))
      return rc;
    NestedScope ns;
    if ((rc = (sig_group == 1 ? blsgpu_sum_g1 : blsgpu_sum_g2)(sig, 1, fmt, sig_proj.data()))) return rc;   // the signature as RAW_PROJ
    return blsgpu_multi_verify(sig_group, scheme, parts.data(), D, sig_proj.data(), msg, msg_len, BLSGPU_FMT_RAW_PROJ, status);
  }
  CTX_ACQUIRE(c);
  const size_t psz = pk_size(sig_group, fmt), T = accumulate_lanes(n);
  size_t need = pad256(psz * n) + pad256(288 * T) + 2 * pad256(msg_len) + 8192;
  if ((rc = arena_reserve(c, need))) return rc;
  c->arena_off = 0;
  const void* d_pks;
  if ((rc = stage_in(c, pks, psz * n, &d_pks))) return rc;
  uint8_t* d_part = (uint8_t*)arena_take(c, 288 * T);
  if (!d_part) return fail(BLSGPU_E_HIP, "internal: arena too small");
  // Unless the scheme prefixes the aggregated key to the message (MessageAugmentation, reference src/traits/sig_aug.rs:20-24),
  // H(msg) does not depend on the keys: hash it on a side stream (one wave) while the main stream sums the keys.
  uint8_t* d_hash = nullptr;
  CutTail cut;
  const bool use_cut = cut_tail_applies(sig_group, scheme) && n > 0;
  if (use_cut) {
    if ((rc = cut_tail_begin(c, sig_group, scheme, sig, fmt, msg, msg_len, cut))) return rc;
  } else if (scheme != BLSGPU_SCHEME_AUG && n > 0) {
    const void* d_msg0;
    if ((rc = stage_in(c, msg, msg_len, &d_msg0))) return rc;
    uint64_t* d_offs0 = (uint64_t*)arena_take(c, 16);
    d_hash = (uint8_t*)arena_take(c, 288);
    if (!d_offs0 || !d_hash) return fail(BLSGPU_E_HIP, "internal: arena too small");
    const uint64_t offs0[2] = {0, (uint64_t)msg_len};
    if ((rc = h2d_small(c, d_offs0, offs0, 16))) return rc;
    if ((rc = side_fork(c))) return rc;
    if (sig_group == 1)   // one wave, the two SSWU maps on two DPP rows in the row-wide field type (csrc/wide.cuh)
      launch_hash_g1_small(c->side, 1, (const uint8_t*)d_msg0, (const uint64_t*)d_offs0, 1, scheme_dst(sig_group, scheme), d_hash, (uint32_t*)nullptr);
    else
      launch_hash_g2_small(c->side, 1, (const uint8_t*)d_msg0, (const uint64_t*)d_offs0, 1, scheme_dst(sig_group, scheme), d_hash);
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(c->ev_join, c->side));
  }
  // MultiPublicKey::from_public_keys: the serial `g += key` of reference src/traits/pk_multi.rs:7-13 as a tree sum
  rc = with_group(key_group(sig_group), [&](auto G) { return run_point_sum<G()>(c, (const uint8_t*)d_pks, fmt, nullptr, nullptr, n, d_part, T); });
  if (use_cut) return cut_tail_finish(c, rc, d_part, cut, status);
  if (d_hash) {
    hipError_t e = hipStreamWaitEvent(c->stream, c->ev_join, 0);    // also on the error path: the side kernel reads the arena
    if (rc) (void)hipStreamSynchronize(c->side);
    if (e != hipSuccess) return fail(BLSGPU_E_HIP, "hipStreamWaitEvent failed");
  }
  if (rc) return rc;
  return verify_one_tail(c, sig_group, scheme, scheme == BLSGPU_SCHEME_AUG, d_part, sig, fmt, msg, msg_len, status, d_hash);
}
API_CATCH

// The device part of core_aggregate_verify (reference src/traits/sig_core.rs:149-178) for n (pk, msg) pairs [plus the
// (sig, -g) pair when d_sig != nullptr], enqueued without a host round trip: hash-to-curve + identity flags, the first
// identity key reduced on the device (d_first: index, n when the signature is the identity, -1 when none), Miller loops
// (flagged pairs contribute 1), product tree; then either the final exponentiation's verdict (d_verdict) or the product
// before the final exponentiation as a 576-byte record (d_rec).
static int aggregate_enqueue(Ctx* c, int sig_group, int scheme, const uint8_t* d_pks, const uint8_t* d_sig, int fmt, const uint8_t* d_msgs,
                             const uint64_t* d_offs, size_t n, int64_t* d_first, int32_t* d_verdict, uint8_t* d_rec) {
  int rc;
  const size_t m = n + 1, mm = d_sig ? m : n;
  const int has_sig = d_sig ? 1 : 0;
  Carver mem{c};
  int32_t* d_bad = mem.take<int32_t>(4 * m);
  unsigned long long* d_min = mem.take<unsigned long long>(64);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIR1_WORDS * 4 * m);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * m);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  HIPCK(hipMemsetAsync(d_min, 0xff, 8, c->stream));
  HIPCK(hipMemsetAsync(d_bad, 0, 4 * m, c->stream));
  const dst_arg dst = scheme_dst(sig_group, scheme);
  const int aug = scheme == BLSGPU_SCHEME_AUG;
  // Bls12381G1Impl: the messages are hashed to E1(Fp) WITHOUT the cofactor clearing (a third of the hash) and the signature's
  // pair is (sig, -[c] g2) instead of (sig, -g2): the same verdict (csrc/g2neg_lines.cuh), also shard by shard -- only the
  // product of all records is ever exponentiated
  // ... on two lanes per item (the two SSWU maps of the hash side by side) while that fits one machine round of lanes: the kernel is a
  // latency chain there (1.75 -> 1.1 ms at 32,768 pairs, 1.63 -> 0.96 at 4,096); beyond a round the redundant rest of the two-lane form costs more
  // than the shorter chains save (5.9 against 5.3 ms at 262,144).  BLSGPU_AGG_LANES=1 / 2 forces a form (A/B)
  const int agg_lanes_env = (int)knobs().agg_lanes;
  const int agg_one_lane = agg_lanes_env == 1 || (agg_lanes_env != 2 && mm > 65536 + 1024);
  const int agg_flags = sig_group == 1 ? (agg_one_lane ? 2 : 3) : 1;
  if (mm > 0) {
    // the workspace stride is always n + 1 (k_prepare_agg's layout); without a signature lane n stays idle
    if (sig_group == 1)
      KL(KID_PREPARE_AGG, k_prepare_agg<1>, dim3(blocks_for(agg_one_lane ? mm : 2 * mm)), dim3(BLS_BLOCK), n, d_pks, d_sig, fmt, aug, d_msgs, d_offs, dst, d_pairs, d_bad, agg_flags, has_sig);
    else
      KL(KID_PREPARE_AGG, k_prepare_agg<2>, dim3(blocks_for(2 * mm)), dim3(BLS_BLOCK), n, d_pks, d_sig, fmt, aug, d_msgs, d_offs, dst, d_pairs, d_bad, agg_flags, has_sig);
    if (n) KL(KID_FIRST_BAD, k_first_bad, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const int32_t*)d_bad, d_min);
  }
  KL(KID_FIRST_BAD, k_first_bad_fin, dim3(1), dim3(BLS_BLOCK), n, (const int32_t*)d_bad, has_sig, (const unsigned long long*)d_min, d_first);
  HIPCK(hipGetLastError());
  if (mm == 0) {                   // an empty shard: the neutral record
    if (d_rec) {
      uint8_t one[576];
      memset(one, 0, sizeof one);
      memcpy(one, FP_ONE_HOST, 48);
      if ((rc = h2d_small(c, d_rec, one, 576))) return rc;
    }
    if (d_verdict) HIPCK(hipMemsetAsync(d_verdict, 0, 4, c->stream));   // the empty product is one
    return 0;
  }
  size_t outputs = 0;
  // the signature's pair (item n, when present): its G2 member is the constant -[c] g2 for Bls12381G1Impl, the signature itself otherwise
  if ((rc = run_miller_product(c, mm, m, d_pairs, d_bad, d_f, &outputs, has_sig ? (sig_group == 1 ? ((agg_flags & 2) ? 2 : 1) : 3) : 0))) return rc;
  if (d_verdict) {
    if ((rc = run_f12_product_verdict(c, d_f, outputs, m, d_verdict))) return rc;
  } else {
    if ((rc = run_f12_fold(c, d_f, outputs, m))) return rc;
    KL(KID_F12_IO, k_f12_export, dim3(1), dim3(BLS_BLOCK), d_f, m, d_rec);
    HIPCK(hipGetLastError());
  }
  return 0;
}

// reference src/traits/sig_basic.rs:46-58 on host-resident messages: first i whose message equals an earlier one.
// Open-addressing table of message indices keyed by a 64-bit hash (computed on all host cores), equality verified on the
// bytes; the scan is sequential so that the FIRST such i is reported, as the reference does.  Returns true on a duplicate.
static bool duplicate_check_host(const uint8_t* mh, const uint64_t* offs_h, size_t n, uint64_t aux_h[2]) {
  std::vector<uint64_t> hs(n);
  {
    unsigned nthr = std::thread::hardware_concurrency();
    if (nthr > 16) nthr = 16;
    if (nthr < 1 || n < 16384) nthr = 1;
    auto work = [&](unsigned t) {
      for (size_t i = n * t / nthr; i < n * (t + 1) / nthr; i++) {
        const uint8_t* p = mh + offs_h[i];
        size_t len = (size_t)(offs_h[i + 1] - offs_h[i]);
        uint64_t h = 0x9e3779b97f4a7c15ull ^ (len * 0xff51afd7ed558ccdull);
        while (len >= 8) {
          uint64_t w;
          memcpy(&w, p, 8);
          h = (h ^ w) * 0xc4ceb9fe1a85ec53ull;
          h ^= h >> 29;
          p += 8;
          len -= 8;
        }
        uint64_t w = 0;
        memcpy(&w, p, len);
        h = (h ^ w) * 0xff51afd7ed558ccdull;
        h ^= h >> 32;
        hs[i] = h;
      }
    };
    if (nthr == 1) {
      work(0);
    } else {
      std::vector<JoinedThread> pool;
      pool.reserve(nthr);
      for (unsigned t = 0; t < nthr; t++) pool.emplace_back([&work, t] { work(t); });
      for (auto& th : pool) th.join();
    }
  }
  size_t cap = 16;
  while (cap < 2 * n) cap <<= 1;
  std::vector<uint32_t> tab(cap, 0);          // index + 1, 0 = empty
  for (size_t i = 0; i < n; i++) {
    const size_t len = (size_t)(offs_h[i + 1] - offs_h[i]);
    size_t slot = (size_t)hs[i] & (cap - 1);
    while (tab[slot]) {
      const size_t j = tab[slot] - 1;
      if (hs[j] == hs[i] && (size_t)(offs_h[j + 1] - offs_h[j]) == len && memcmp(mh + offs_h[j], mh + offs_h[i], len) == 0) {
        aux_h[0] = j;
        aux_h[1] = i;
        return true;
      }
      slot = (slot + 1) & (cap - 1);
    }
    tab[slot] = (uint32_t)(i + 1);
  }
  return false;
}

int blsgpu_aggregate_verify(int sig_group, int scheme, const void* pks, const uint8_t* msgs, const uint64_t* msg_offsets,
                            size_t n, const void* sig, int fmt, int32_t* status, uint64_t* aux) try {
  int rc = check_common(sig_group, scheme, fmt);
  if (rc) return rc;
  if (!sig || !status || !msg_offsets || (n && !pks)) return fail(BLSGPU_E_ARG, "null argument");
  if (const size_t D = shard_devices(n, {pks, msgs, msg_offsets, sig}); D > 1) {
    // every device: hash-to-curve + Miller loops of its range -> one Fp12 record (blsgpu_aggregate_partial; device 0 also
    // takes the signature pair); meanwhile this thread applies Basic's duplicate rule to the whole list; then the D records
    // are multiplied and exponentiated once on device 0 -- the exchange that the one-process-per-GPU path does over RCCL
    const size_t psz = pk_size(sig_group, fmt);
    std::vector<uint8_t> recs(576 * D);
    std::vector<int64_t> fbs(D, -1);
    uint64_t dup[2] = {~0ull, ~0ull};
    int dup_rc = 0;
    std::string dup_err;
    JoinedThread dup_thread;
    if (scheme == BLSGPU_SCHEME_BASIC)
      dup_thread = JoinedThread([&] {
        t_nested = true;
        if (is_device_ptr(msgs)) {
          dup_rc = blsgpu_first_duplicate_message(msgs, msg_offsets, n, dup);
        } else {
          std::vector<uint64_t> oh;
          const uint64_t* offs = msg_offsets;
          if (is_device_ptr(msg_offsets)) {
            oh.resize(n + 1);
            if (hipMemcpy(oh.data(), msg_offsets, 8 * (n + 1), hipMemcpyDeviceToHost) != hipSuccess) dup_rc = fail(BLSGPU_E_HIP, "copying the message offsets");
            offs = oh.data();
          }
          uint64_t a2[2] = {0, 0};
          if (!dup_rc && duplicate_check_host(msgs, offs, n, a2)) {
            dup[0] = a2[0];
            dup[1] = a2[1];
          }
        }
        dup_err = t_err;
      });
    rc = run_on_devices(D, [&](size_t d) {
      const size_t lo = n * d / D, hi = n * (d + 1) / D;
      return blsgpu_aggregate_partial(sig_group, scheme, (const uint8_t*)pks + lo * psz, msgs, msg_offsets + lo, hi - lo, d == 0 ? sig : nullptr, fmt,
                                      recs.data() + 576 * d, &fbs[d]);
    });
    dup_thread.join();
    if (rc) return rc;
    if (dup_rc) {
      t_err = dup_err;
      return dup_rc;
    }
    int32_t st = BLSGPU_OK;
    uint64_t aux_h[2] = {0, 0};
    if (dup[1] != ~0ull) {
      st = BLSGPU_DUPLICATE_MESSAGE;
      aux_h[0] = dup[0];
      aux_h[1] = dup[1];
    } else if (fbs[0] == (int64_t)(n * 1 / D)) {          // device 0 saw the identity signature (its local index n)
      st = BLSGPU_SIG_IDENTITY;
    } else {
      for (size_t d = 0; d < D && st == BLSGPU_OK; d++)
        if (fbs[d] >= 0) {
          st = BLSGPU_PK_IDENTITY;
          aux_h[0] = n * d / D + (uint64_t)fbs[d] + 1;
        }
      if (st == BLSGPU_OK) {
        NestedScope ns;
        int32_t one = 0;
        if ((rc = blsgpu_fp12_product_is_one(recs.data(), D, &one))) return rc;
        st = one ? BLSGPU_OK : BLSGPU_INVALID_SIGNATURE;
      }
    }
    if (int e = put_i32(status, st)) return e;
    if (aux) {
      if (is_device_ptr(aux)) HIPCK(hipMemcpy(aux, aux_h, 16, hipMemcpyHostToDevice));
      else memcpy(aux, aux_h, 16);
    }
    return 0;
  }
  CTX_ACQUIRE(c);
  uint64_t aux_h[2] = {0, 0};
  const bool trace = knobs().host_trace != 0;
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_start = now();
  const bool basic = scheme == BLSGPU_SCHEME_BASIC;
  // Basic's duplicate-message rule (reference src/traits/sig_basic.rs:46-58) runs where the messages live: on the device for
  // device-resident messages (k_dup_*), on the host (overlapped with the device's hashing) for host buffers.  In the
  // reference it runs to completion before anything else; here the verdict keeps that precedence.
  const bool dev_msgs = is_device_ptr(msgs), dev_offs = is_device_ptr(msg_offsets);
  const bool dup_on_device = basic && dev_msgs;
  std::vector<uint64_t> offs_h;
  uint64_t total = 0;
  if (basic && !dev_msgs && dev_offs) {   // host messages with device offsets: the host check needs the offsets
    offs_h.resize(n + 1);
    HIPCK(hipMemcpy(offs_h.data(), msg_offsets, 8 * (n + 1), hipMemcpyDeviceToHost));
    total = offs_h[n];
  } else if (dev_offs) {
    HIPCK(hipMemcpy(&total, msg_offsets + n, 8, hipMemcpyDeviceToHost));
  } else {
    total = msg_offsets[n];
  }
  const size_t m = n + 1, psz = pk_size(sig_group, fmt);
  size_t need = pad256(psz * n) + pad256(sig_size(sig_group, fmt)) + pad256(total) + pad256(8 * m) + pad256(4 * m) +
                2 * pad256((size_t)WS_PAIRS_WORDS * 4 * m) + 8192 + (dup_on_device ? dup_ws_bytes(n) : 0);
  if ((rc = arena_reserve(c, need))) return rc;
  c->arena_off = 0;
  const void *d_pks, *d_sig, *d_msgs, *d_offs;
  if ((rc = stage_in(c, pks, psz * n, &d_pks))) return rc;
  if ((rc = stage_in(c, sig, sig_size(sig_group, fmt), &d_sig))) return rc;
  if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
  if ((rc = stage_in(c, msg_offsets, 8 * m, &d_offs))) return rc;
  const double t_staged = now();
  Carver mem{c};
  int64_t* d_first = mem.take<int64_t>(64);
  int32_t* d_verdict = mem.take<int32_t>(64);
  uint64_t* d_dup = mem.take<uint64_t>(64);
  struct results { int64_t first; int32_t verdict; int32_t pad; uint64_t dup[2]; };
  results* h = (results*)hsmall_take(c, sizeof(results));
  if (!mem.ok || !h) return fail(BLSGPU_E_HIP, "internal: arena too small");
  h->dup[0] = h->dup[1] = ~0ull;
  // everything is enqueued at once; the identity index, the verdict and the duplicate pair come back together and the
  // host applies the reference's precedence afterwards
  if ((rc = aggregate_enqueue(c, sig_group, scheme, (const uint8_t*)d_pks, (const uint8_t*)d_sig, fmt, (const uint8_t*)d_msgs,
                              (const uint64_t*)d_offs, n, d_first, d_verdict, nullptr)))
    return rc;
  if (dup_on_device) {
    if ((rc = run_first_duplicate(c, (const uint8_t*)d_msgs, (const uint64_t*)d_offs, n, d_dup))) return rc;
    HIPCK(hipMemcpyAsync(h->dup, d_dup, 16, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCK(hipMemcpyAsync(&h->first, d_first, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCK(hipMemcpyAsync(&h->verdict, d_verdict, 4, hipMemcpyDeviceToHost, c->stream));
  bool dup = false;
  if (basic && !dev_msgs) {       // on the host, while the device works
    dup = duplicate_check_host(msgs, offs_h.empty() ? msg_offsets : offs_h.data(), n, aux_h);
    if (trace) fprintf(stderr, "[blsgpu] aggregate_verify n=%zu: host duplicate check %.2f ms (overlapped)\n", n, now() - t_staged);
  }
  SYNC_FLUSH(c);
  if (trace) fprintf(stderr, "[blsgpu] aggregate_verify n=%zu: staging %.2f ms, total %.2f ms\n", n, t_staged - t_start, now() - t_start);
  if (dup_on_device && h->dup[1] != ~0ull) {
    dup = true;
    aux_h[0] = h->dup[0];
    aux_h[1] = h->dup[1];
  }
  int32_t st;
  if (dup) {
    st = BLSGPU_DUPLICATE_MESSAGE;   // reported before any identity check (sig_basic.rs:46-58 precedes core_aggregate_verify)
  } else if (h->first == (int64_t)n) {
    st = BLSGPU_SIG_IDENTITY;        // reference src/traits/sig_core.rs:155-167: signature identity first, ...
  } else if (h->first >= 0) {
    st = BLSGPU_PK_IDENTITY;         // ... then the first identity key (1-based)
    aux_h[0] = (uint64_t)h->first + 1;
  } else {
    st = h->verdict;
  }
  if (int e = put_i32(status, st)) return e;
  if (aux) {
    if (is_device_ptr(aux)) HIPCK(hipMemcpy(aux, aux_h, 16, hipMemcpyHostToDevice));
    else memcpy(aux, aux_h, 16);
  }
  return 0;
}
API_CATCH

// sig is the identity <=> Ok for an empty key list (reference src/secure_aggregation.rs:189-195)
static int empty_list_verdict(Ctx* c, int sig_group, const void* sig, int fmt, int32_t* st) {
  int rc;
  const void* d_sig;
  if ((rc = stage_in(c, sig, sig_size(sig_group, fmt), &d_sig))) return rc;
  uint8_t* d_proj = (uint8_t*)arena_take(c, 288);
  uint8_t* h = (uint8_t*)hsmall_take(c, 288);
  if (!d_proj || !h) return fail(BLSGPU_E_HIP, "internal: arena too small");
  rc = with_group(sig_group, [&](auto G) { return run_point_sum<G()>(c, (const uint8_t*)d_sig, fmt, nullptr, nullptr, 1, d_proj, 1); });
  if (rc) return rc;
  HIPCK(hipMemcpyAsync(h, d_proj, 288, hipMemcpyDeviceToHost, c->stream));
  SYNC_FLUSH(c);
  const size_t zoff = sig_size(sig_group, BLSGPU_FMT_RAW_AFFINE), zlen = sig_size(sig_group, BLSGPU_FMT_RAW_PROJ) - zoff;   // Z follows X and Y
  bool inf = true;
  for (size_t k = 0; k < zlen; k++) inf = inf && h[zoff + k] == 0;
  *st = inf ? BLSGPU_OK : BLSGPU_INVALID_SIGNATURE;
  return 0;
}

int blsgpu_verify_secure(int sig_group, int scheme, const void* pks, size_t n, const void* sig, const uint8_t* msg,
                         size_t msg_len, int ser_format, int fmt, int32_t* status) try {
  int rc = check_common(sig_group, scheme, fmt);
  if (rc) return rc;
  if (!sig || !status || (n && !pks)) return fail(BLSGPU_E_ARG, "null argument");
  if ((rc = check_ser_format(sig_group, ser_format))) return rc;
  if (n >= 0xffffffffull) return fail(BLSGPU_E_ARG, "more than 2^32 - 2 keys");
  if (const size_t D = shard_devices(n, {pks, sig}); D > 1) {
    // every device serialises its range of the keys; device 0 sorts all of them and a host core hashes the sorted stream
    // (the one sequential step, reference src/secure_aggregation.rs:45-59); every device derives the coefficients of its
    // own keys and adds up its share of sum t_i pk_i; device 0 folds the D partial sums and runs the one verification
    const int pk_group = key_group(sig_group);
    const size_t psz = pk_size(sig_group, fmt), width = pk_size(sig_group, BLSGPU_FMT_COMPRESSED), osz = pk_size(sig_group, BLSGPU_FMT_RAW_PROJ);
    std::vector<uint8_t> kb(width * n), parts(osz * D), apk(288), sig_proj(288), hm(288), digest(32);
    std::vector<uint32_t> perm(n);
    std::vector<int32_t> sts(D, 0);
    const char* dsts = DST_TABLE[sig_group - 1][scheme];
    const uint64_t offs1[2] = {0, (uint64_t)msg_len};
    int hash_rc = 0;
    std::string hash_err;
    JoinedThread hash_thread([&] {           // H(msg) beside everything else (a second context of device 0)
      t_nested = true;
      hash_rc = (sig_group == 1 ? blsgpu_hash_to_g1 : blsgpu_hash_to_g2)(msg, offs1, 1, (const uint8_t*)dsts, strlen(dsts), hm.data());
      hash_err = t_err;
    });
    rc = run_on_devices(D, [&](size_t d) {
      const size_t lo = n * d / D, hi = n * (d + 1) / D;
      return blsgpu_serialize(pk_group, (const uint8_t*)pks + lo * psz, hi - lo, fmt, ser_format ? BLSGPU_FMT_LEGACY : BLSGPU_FMT_COMPRESSED,
                              kb.data() + width * lo, nullptr);
    });
    if (!rc) {
      NestedScope ns;
      rc = blsgpu_sort_keys(kb.data(), n, width, perm.data());
      if (!rc) rc = blsgpu_sorted_keys_digest(kb.data(), perm.data(), n, width, digest.data());
    }
    if (!rc)
      rc = run_on_devices(D, [&](size_t d) {
        const size_t lo = n * d / D, hi = n * (d + 1) / D;
        std::vector<uint8_t> scal(32 * (hi - lo));
        int r2 = blsgpu_coefficients_for_range(digest.data(), perm.data(), n, lo, hi - lo, scal.data(), &sts[d]);
        if (r2) return r2;
        return (pk_group == 1 ? blsgpu_msm_g1 : blsgpu_msm_g2)((const uint8_t*)pks + lo * psz, scal.data(), hi - lo, fmt, parts.data() + osz * d);
      });
    hash_thread.join();
    if (rc) return rc;
    if (hash_rc) {
      t_err = hash_err;
      return hash_rc;
    }
    int32_t st = BLSGPU_OK;
    for (size_t d = 0; d < D; d++)
      if (sts[d] != BLSGPU_OK) st = BLSGPU_INVALID_COEFFICIENT;
    if (st == BLSGPU_OK) {
      NestedScope ns;
      if ((rc = (pk_group == 1 ? blsgpu_sum_g1 : blsgpu_sum_g2)(parts.data(), D, BLSGPU_FMT_RAW_PROJ, apk.data()))) return rc;
      if ((rc = (sig_group == 1 ? blsgpu_sum_g1 : blsgpu_sum_g2)(sig, 1, fmt, sig_proj.data()))) return rc;
      if ((rc = blsgpu_core_verify_hashed(sig_group, apk.data(), sig_proj.data(), hm.data(), 1, &st))) return rc;
    }
    return put_i32(status, st);
  }
  CTX_ACQUIRE(c);
  const bool trace = knobs().host_trace != 0;
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const size_t psz = pk_size(sig_group, fmt), width = pk_size(sig_group, BLSGPU_FMT_COMPRESSED), T = accumulate_lanes(n);
  // weighted MSM tables (csrc/kernels.cuh k_msm2_tables): built while the host hashes the key stream; BLSGPU_MSM2_TABLES=0 switches them off
  // (up to 262,144 keys: the tables are 4.5 KB per G2 key -- 1.2 GB there -- and stay in the context's arena; beyond that size the sum
  // is throughput-bound and its chunk lanes' latency no longer shows)
  const bool msm_tables = knobs().msm2_tables != 0 && msm_use_pippenger(n) && !msm_use_v1() && n <= ((size_t)1 << 18);
  size_t need = pad256(psz * n) + pad256(width * n) + pad256(32 * n) + pad256(288 * T) + pad256(msg_len) + 16384 + msm_ws_bytes(n) +
                keysort_ws_bytes(n, width) + (msm_tables ? msm2_tables_bytes(n, key_group(sig_group)) : 0);
  if ((rc = arena_reserve(c, need))) return rc;
  c->arena_off = 0;
  int32_t st = BLSGPU_OK;
  if (n == 0) {
    if ((rc = empty_list_verdict(c, sig_group, sig, fmt, &st))) return rc;
    return put_i32(status, st);
  }
  const void* d_pks;
  if ((rc = stage_in(c, pks, psz * n, &d_pks))) return rc;
  Carver mem{c};
  uint8_t* d_bytes = mem.take<uint8_t>(width * n);
  uint8_t* d_scal = mem.take<uint8_t>(32 * n);
  uint8_t* d_part = mem.take<uint8_t>(288 * T);
  uint8_t* d_H = mem.take<uint8_t>(64);
  int32_t* d_zero = mem.take<int32_t>(64);
  int32_t* h_zero = (int32_t*)hsmall_take(c, 64);
  keysort_ws w;
  if (!mem.ok || !h_zero) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if ((rc = keysort_ws_take(c, n, width, w))) return rc;
  const double t0 = now();
  // PublicKey::to_bytes / to_bytes_with_mode of every key (reference src/secure_aggregation.rs:42,47; public_key.rs:146-151)
  with_group(key_group(sig_group), [&](auto G) {
    KL(KID_COMPRESS, k_compress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_pks, fmt, ser_format, d_bytes);
  });
  HIPCK(hipGetLastError());
  // stable byte-lexicographic sort on the device; the sorted bytes travel to the host for the one sequential SHA-256
  if (!c->ev_host) HIPCK(hipEventCreateWithFlags(&c->ev_host, hipEventDisableTiming));
  bool full_sort = false;
  if ((rc = run_key_sort_to_host(c, d_bytes, n, width, w, c->ev_host, &full_sort))) return rc;
  // H(msg) does not depend on the keys (verify_secure never prefixes them, reference src/secure_aggregation.rs:236-246): the
  // hash-to-curve of the final core_verify -- one wave, 1 ms for G1 and 4 ms for G2 of pure latency -- runs on the side
  // stream beside everything up to the pairing: the key sort, the host's hash of the key stream and the whole key sum; for
  // Bls12381G1Impl the signature's half of the pairing check goes with it (cut_tail_begin).
  uint8_t* d_hash = nullptr;
  CutTail cut;
  const bool use_cut = cut_tail_applies(sig_group, scheme);
  if (use_cut) {
    if ((rc = cut_tail_begin(c, sig_group, scheme, sig, fmt, msg, msg_len, cut))) return rc;
  } else {
    const void* d_msg0;
    if ((rc = stage_in(c, msg, msg_len, &d_msg0))) return rc;
    uint64_t* d_offs0 = (uint64_t*)arena_take(c, 16);
    d_hash = (uint8_t*)arena_take(c, 288);
    if (!d_offs0 || !d_hash) return fail(BLSGPU_E_HIP, "internal: arena too small");
    const uint64_t offs0[2] = {0, (uint64_t)msg_len};
    if ((rc = h2d_small(c, d_offs0, offs0, 16))) return rc;
    if ((rc = side_fork(c))) return rc;
    if (sig_group == 1)
      launch_hash_g1_small(c->side, 1, (const uint8_t*)d_msg0, (const uint64_t*)d_offs0, 1, scheme_dst(sig_group, scheme), d_hash, (uint32_t*)nullptr);
    else
      launch_hash_g2_small(c->side, 1, (const uint8_t*)d_msg0, (const uint64_t*)d_offs0, 1, scheme_dst(sig_group, scheme), d_hash);
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(c->ev_join, c->side));
  }
  // ... and so does the scalar-independent part of the key sum (every key to affine, with its endomorphism images)
  const bool msm2 = msm_use_pippenger(n) && !msm_use_v1();
  msm2_ws mw;
  if (msm2) {
    if ((rc = msm2_ws_take(c, n, key_group(sig_group), mw, msm_tables))) return rc;
    rc = with_group(key_group(sig_group), [&](auto G) { return run_msm2_prep<G()>(c, (const uint8_t*)d_pks, fmt, nullptr, n, mw); });
    if (rc) return rc;
  }
  if ((rc = run_key_sort_finish(c, d_bytes, n, width, w, c->ev_host, &full_sort))) return rc;
  const double t1 = now();
  uint8_t H[32];
  keys_digest_host(c->hpin, width * n, H);
  const double t2 = now();
  if ((rc = h2d_small(c, d_H, H, 32))) return rc;
  HIPCK(hipMemsetAsync(d_zero, 0, 4, c->stream));
  // t_i on the device, written to the INPUT slot of the key that sorted to position i: the sum below needs no permutation
  if ((rc = run_coefficients(c, d_H, w.perm_a, n, 0, n, 0, d_scal, d_zero))) return rc;
  HIPCK(hipMemcpyAsync(h_zero, d_zero, 4, hipMemcpyDeviceToHost, c->stream));
  // aggregated_pk = sum t_i * pk_sorted[i]   (reference src/secure_aggregation.rs:201-204)
  if (msm2) {
    rc = with_group(key_group(sig_group), [&](auto G) { return run_msm2_rest<G()>(c, d_scal, n, mw, d_part, false); });
  } else {
    rc = with_group(key_group(sig_group), [&](auto G) { return run_point_sum<G()>(c, (const uint8_t*)d_pks, fmt, d_scal, nullptr, n, d_part, T); });
  }
  if (use_cut) {
    if ((rc = cut_tail_finish(c, rc, d_part, cut, status))) return rc;
  } else {
    if (rc) return rc;
    HIPCK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    if ((rc = verify_one_tail(c, sig_group, scheme, 0, d_part, sig, fmt, msg, msg_len, status, d_hash))) return rc;
  }
  if (trace)
    fprintf(stderr, "[blsgpu] verify_secure n=%zu: compress + key sort%s + D2H %.2f ms (message hash on the side stream), key-stream SHA-256 on the host %.2f ms, rest %.2f ms\n",
            n, full_sort ? " (full-width)" : "", t1 - t0, t2 - t1, now() - t2);
  if (*h_zero) {                   // a zero coefficient: BlsError::InvalidCoefficient before any verification (:97-100)
    st = BLSGPU_INVALID_COEFFICIENT;
    if (int e = put_i32(status, st)) return e;
  }
  return 0;
}
API_CATCH

int blsgpu_secure_coefficients(const uint8_t* key_bytes, size_t n, size_t width, uint32_t* out_perm, uint8_t* out_scalars,
                               int32_t* status) try {
  if (!initialised()) return NOT_INIT();
  if (width != 48 && width != 96) return fail(BLSGPU_E_ARG, "width must be 48 or 96");
  if (!status || (n && (!key_bytes || !out_perm || !out_scalars))) return fail(BLSGPU_E_ARG, "null argument");
  if (n >= 0xffffffffull) return fail(BLSGPU_E_ARG, "more than 2^32 - 2 keys");
  int32_t st = BLSGPU_OK;
  if (n) {
    CTX_ACQUIRE(c);
    int rc = arena_reserve(c, pad256(width * n) + pad256(32 * n) + keysort_ws_bytes(n, width) + 4096);
    if (rc) return rc;
    c->arena_off = 0;
    const void* d_kb;
    if ((rc = stage_in(c, key_bytes, width * n, &d_kb))) return rc;
    Carver mem{c};
    uint8_t* d_scal = mem.take<uint8_t>(32 * n);
    uint8_t* d_H = mem.take<uint8_t>(64);
    int32_t* d_zero = mem.take<int32_t>(64);
    int32_t* h_zero = (int32_t*)hsmall_take(c, 64);
    keysort_ws w;
    if (!mem.ok || !h_zero) return fail(BLSGPU_E_HIP, "internal: arena too small");
    if ((rc = keysort_ws_take(c, n, width, w))) return rc;
    if ((rc = run_key_sort_to_host(c, (const uint8_t*)d_kb, n, width, w, nullptr, nullptr))) return rc;
    uint8_t H[32];
    keys_digest_host(c->hpin, width * n, H);
    if ((rc = h2d_small(c, d_H, H, 32))) return rc;
    HIPCK(hipMemsetAsync(d_zero, 0, 4, c->stream));
    if ((rc = run_coefficients(c, d_H, w.perm_a, n, 0, n, 1, d_scal, d_zero))) return rc;
    HIPCK(hipMemcpyAsync(h_zero, d_zero, 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = copy_out(c, out_perm, w.perm_a, 4 * n))) return rc;
    if ((rc = copy_out(c, out_scalars, d_scal, 32 * n))) return rc;
    SYNC_FLUSH(c);
    if (*h_zero) st = BLSGPU_INVALID_COEFFICIENT;
  }
  return put_i32(status, st);
}
API_CATCH

/* The three steps of hash_public_keys_with_sorted as separate calls, for callers that shard the keys over several GPUs
 * (agora-blsful_amd/dist.py): every rank sorts the gathered key bytes (cheap, on its device), ONE rank hashes the sorted
 * stream and broadcasts the 32-byte digest, every rank derives the coefficients of its own keys.
 * blsgpu_sort_keys: out_perm[i] = input index of the i-th key in stable byte-lexicographic order. */
int blsgpu_sort_keys(const uint8_t* key_bytes, size_t n, size_t width, uint32_t* out_perm) try {
  if (!initialised()) return NOT_INIT();
  if (width != 48 && width != 96) return fail(BLSGPU_E_ARG, "width must be 48 or 96");
  if (n == 0) return 0;
  if (!key_bytes || !out_perm) return fail(BLSGPU_E_ARG, "null argument");
  if (n >= 0xffffffffull) return fail(BLSGPU_E_ARG, "more than 2^32 - 2 keys");
  CTX_ACQUIRE(c);
  int rc = arena_reserve(c, pad256(width * n) + keysort_ws_bytes(n, width) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void* d_kb;
  if ((rc = stage_in(c, key_bytes, width * n, &d_kb))) return rc;
  keysort_ws w;
  if ((rc = keysort_ws_take(c, n, width, w))) return rc;
  uint32_t* h_flag = (uint32_t*)hsmall_take(c, 64);
  if (!h_flag) return fail(BLSGPU_E_HIP, "internal: pinned record buffer exhausted");
  for (int attempt = 0; attempt < 2; attempt++) {
    if ((rc = run_key_sort_passes(c, (const uint8_t*)d_kb, n, width, attempt == 0 ? keysort_prefix(n) : (int)width, w))) return rc;
    if (attempt == 1) break;
    HIPCK(hipMemsetAsync(w.flag, 0, 4, c->stream));
    KL(KID_KEY_SORT, k_keys_tie_flag, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_kb, width, (size_t)keysort_prefix(n), (const uint32_t*)w.perm_a, w.flag);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(h_flag, w.flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (*h_flag == 0) break;
  }
  if ((rc = copy_out(c, out_perm, w.perm_a, 4 * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* out_digest[32] = SHA-256 over the keys concatenated in the order of perm (reference src/secure_aggregation.rs:45-59). */
int blsgpu_sorted_keys_digest(const uint8_t* key_bytes, const uint32_t* perm, size_t n, size_t width, uint8_t* out_digest) try {
  if (!initialised()) return NOT_INIT();
  if (width != 48 && width != 96) return fail(BLSGPU_E_ARG, "width must be 48 or 96");
  if (!out_digest || (n && (!key_bytes || !perm))) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  int rc = arena_reserve(c, 2 * pad256(width * n) + pad256(4 * n) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  if ((rc = pinned_reserve(c, width * n + 64))) return rc;
  if (n) {
    const void *d_kb, *d_perm;
    if ((rc = stage_in(c, key_bytes, width * n, &d_kb))) return rc;
    if ((rc = stage_in(c, perm, 4 * n, &d_perm))) return rc;
    uint8_t* d_sorted = (uint8_t*)arena_take(c, width * n);
    if (!d_sorted) return fail(BLSGPU_E_HIP, "internal: arena too small");
    KL(KID_KEY_SORT, k_keys_gather, dim3(blocks_for(n * (width / 4))), dim3(BLS_BLOCK), n, (const uint8_t*)d_kb, width, (const uint32_t*)d_perm, d_sorted);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(c->hpin, d_sorted, width * n, hipMemcpyDeviceToHost, c->stream));
    SYNC_FLUSH(c);
  }
  uint8_t H[32];
  keys_digest_host(c->hpin, width * n, H);
  HIPCK(hipMemcpy(out_digest, H, 32, is_device_ptr(out_digest) ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
  return 0;
}
API_CATCH

/* t_i = SHA-256(BE32(i) || digest) mod r for the keys of the shard [base, base + count) of the n sorted keys, written in the
 * shard's INPUT order: out_scalars[g - base] belongs to input key g (32 B little-endian each).  *status: BLSGPU_OK or
 * BLSGPU_INVALID_COEFFICIENT (reference src/secure_aggregation.rs:61-100). */
int blsgpu_coefficients_for_range(const uint8_t* digest, const uint32_t* perm, size_t n, size_t base, size_t count,
                                  uint8_t* out_scalars, int32_t* status) try {
  if (!initialised()) return NOT_INIT();
  if (!digest || !status || (n && !perm) || (count && !out_scalars)) return fail(BLSGPU_E_ARG, "null argument");
  if (base + count > n) return fail(BLSGPU_E_ARG, "shard range exceeds the key count");
  int32_t st = BLSGPU_OK;
  if (n) {
    CTX_ACQUIRE(c);
    int rc = arena_reserve(c, pad256(4 * n) + pad256(32 * count) + 4096);
    if (rc) return rc;
    c->arena_off = 0;
    const void *d_perm, *d_H;
    if ((rc = stage_in(c, perm, 4 * n, &d_perm))) return rc;
    if ((rc = stage_in(c, digest, 32, &d_H))) return rc;
    Carver mem{c};
    uint8_t* d_scal = mem.stage_out<uint8_t>(out_scalars, 32 * count);
    int32_t* d_zero = mem.take<int32_t>(64);
    int32_t* h_zero = (int32_t*)hsmall_take(c, 64);
    if (!mem.ok || !h_zero) return fail(BLSGPU_E_HIP, "internal: arena too small");
    HIPCK(hipMemsetAsync(d_zero, 0, 4, c->stream));
    if ((rc = run_coefficients(c, (const uint8_t*)d_H, (const uint32_t*)d_perm, n, base, count, 0, d_scal, d_zero))) return rc;
    HIPCK(hipMemcpyAsync(h_zero, d_zero, 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = stage_back(c, out_scalars, d_scal, 32 * count))) return rc;
    SYNC_FLUSH(c);
    if (*h_zero) st = BLSGPU_INVALID_COEFFICIENT;
  }
  return put_i32(status, st);
}
API_CATCH

/* out_idx[p] = input index of the FIRST key equal to the p-th sorted key (perm from blsgpu_sort_keys: stable, so that is
 * the input index at the start of p's run of equal keys) -- the `position` search of aggregate_secure, reference
 * src/secure_aggregation.rs:150-162. */
int blsgpu_first_occurrence(const uint8_t* key_bytes, const uint32_t* perm, size_t n, size_t width, uint32_t* out_idx) try {
  if (!initialised()) return NOT_INIT();
  if (width != 48 && width != 96) return fail(BLSGPU_E_ARG, "width must be 48 or 96");
  if (n == 0) return 0;
  if (!key_bytes || !perm || !out_idx) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  int rc = arena_reserve(c, pad256(width * n) + 3 * pad256(4 * n) + pad256(4 * scan_tiles(n)) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_kb, *d_perm;
  if ((rc = stage_in(c, key_bytes, width * n, &d_kb))) return rc;
  if ((rc = stage_in(c, perm, 4 * n, &d_perm))) return rc;
  Carver mem{c};
  uint32_t* d_start = mem.take<uint32_t>(4 * n);
  uint32_t* d_tiles = mem.take<uint32_t>(4 * scan_tiles(n));
  uint32_t* d_idx = mem.stage_out<uint32_t>(out_idx, 4 * n);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  KL(KID_KEY_SORT, k_keys_run_start, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_kb, width, (const uint32_t*)d_perm, d_start);
  if ((rc = run_scan_max_u32(c, KID_KEY_SORT, n, d_start, d_tiles))) return rc;
  KL(KID_KEY_SORT, k_run_first_index, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint32_t*)d_perm, (const uint32_t*)d_start, d_idx);
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out_idx, d_idx, 4 * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* Basic's duplicate-message rule on its own (reference src/traits/sig_basic.rs:46-58), for sharded callers that gathered the
 * messages: out2 = (index of the earlier equal message, first index i whose message was seen before), or (~0, ~0). */
int blsgpu_first_duplicate_message(const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, uint64_t* out2) try {
  if (!initialised()) return NOT_INIT();
  if (!out2 || !msg_offsets) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  uint64_t total = 0;
  if (is_device_ptr(msg_offsets)) HIPCK(hipMemcpy(&total, msg_offsets + n, 8, hipMemcpyDeviceToHost));
  else total = msg_offsets[n];
  int rc = arena_reserve(c, pad256(total) + pad256(8 * (n + 1)) + dup_ws_bytes(n) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_msgs, *d_offs;
  if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
  if ((rc = stage_in(c, msg_offsets, 8 * (n + 1), &d_offs))) return rc;
  uint64_t* d_out = (uint64_t*)arena_take(c, 64);
  if (!d_out) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if ((rc = run_first_duplicate(c, (const uint8_t*)d_msgs, (const uint64_t*)d_offs, n, d_out))) return rc;
  if ((rc = copy_out(c, out2, d_out, 16))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

// H(msg_i) into `group` for n messages on the device (RAW_PROJ out, cofactor-cleared), stream-ordered: the launch plan of
// blsgpu_hash_to_g1 / blsgpu_hash_to_g2.  May take 768 n bytes from the arena (129 .. BLSGPU_WIDE_MAX messages into G2).
// uncleared (group 1 only): the points stay in E1(Fp) before the cofactor clearing, what a Bls12381G1Impl verification pairs with
// -[c] g2 -- one wave per message up to 1,024 messages, two lanes per message beyond (the measured split of run_verify_items)
static int run_hash_group(Ctx* c, int group, size_t n, const uint8_t* d_msgs, const uint64_t* d_offs, const dst_arg& d, uint8_t* d_out, bool uncleared = false) {
  if (uncleared && group == 1) {
    if (n <= 1024 && wide_max_items() > 0) KL(KID_HASH, k_hash_to_g1_wide<false>, dim3((unsigned)n), dim3(BLS_BLOCK), n, d_msgs, d_offs, 2, d, d_out, (uint32_t*)nullptr);
    else KL(KID_HASH, k_hash_to_g1<false>, dim3(blocks_for(2 * n)), dim3(BLS_BLOCK), n, d_msgs, d_offs, d, d_out, 1 | 2);
    HIPCK(hipGetLastError());
    return 0;
  }
  // two lanes per message: always for G2; for G1 up to the cooperative threshold (a full hash-only batch is faster with one lane per message)
  const int two = (group == 2 || n <= coop_max_items()) ? 1 : 0;
  if (group == 1 && n <= wide_max_items())   // a few messages: one wave each in the row-wide field type (0.98 ms against 1.6 ms of latency)
  {
    prof_pre(c, KID_HASH);
    launch_hash_g1_small(c->stream, n, d_msgs, d_offs, 0, d, d_out, (uint32_t*)nullptr);
    prof_post(c);
  }
  else if (group == 1) KL(KID_HASH, k_hash_to_g1<false>, dim3(blocks_for(two ? 2 * n : n)), dim3(BLS_BLOCK), n, d_msgs, d_offs, d, d_out, two);
  else if (n <= wide_max_items() && hash_phase_stop() == 0) {   // a few messages: row-wide maps and the engine (one workgroup per message up to 128)
    prof_pre(c, KID_HASH);
    launch_hash_g2_small(c->stream, n, d_msgs, d_offs, 0, d, d_out, n > 128 ? (uint32_t*)arena_take(c, 768 * n) : nullptr);
    prof_post(c);
  } else if (n <= wide_max_items() && hash_phase_stop() != 8) {   // measurement aids (BLSGPU_HASH_STOP=8: clearing in the lane-pair kernel; 9: none)
    KL(KID_HASH, k_hash_to_g2<false>, dim3(blocks_for(2 * n)), dim3(BLS_BLOCK), n, d_msgs, d_offs, d, d_out, 3);
    if (hash_phase_stop() != 9) KL(KID_HASH, k_g2_clear_wide, dim3((unsigned)n), dim3(WIDE_ENGINE_BLOCK), n, d_out);   // 9: measurement aid, no clearing
  } else
    KL(KID_HASH, k_hash_to_g2<false>, dim3(blocks_for(two ? 2 * n : n)), dim3(BLS_BLOCK), n, d_msgs, d_offs, d, d_out, two);
  HIPCK(hipGetLastError());
  return 0;
}
static int hash_to_group(int group, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, const uint8_t* dst, size_t dst_len, void* out) {
  if (!initialised()) return NOT_INIT();
  if (n == 0) return 0;
  if (!msg_offsets || !out || !dst) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  uint64_t total = 0;
  if (is_device_ptr(msg_offsets)) HIPCK(hipMemcpy(&total, msg_offsets + n, 8, hipMemcpyDeviceToHost));
  else total = msg_offsets[n];
  const size_t osz = point_bytes(group, BLSGPU_FMT_RAW_PROJ);
  int rc = arena_reserve(c, pad256(total) + pad256(8 * (n + 1)) + pad256(osz * n) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_msgs, *d_offs;
  if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
  if ((rc = stage_in(c, msg_offsets, 8 * (n + 1), &d_offs))) return rc;
  uint8_t* d_out = stage_out<uint8_t>(c, out, osz * n);
  if (!d_out) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if ((rc = run_hash_group(c, group, n, (const uint8_t*)d_msgs, (const uint64_t*)d_offs, make_dst(dst, dst_len), d_out))) return rc;
  if ((rc = stage_back(c, out, d_out, osz * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
int blsgpu_hash_to_g1(const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, const uint8_t* dst, size_t dst_len, void* out) try {
  return hash_to_group(1, msgs, msg_offsets, n, dst, dst_len, out);
}
API_CATCH
int blsgpu_hash_to_g2(const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, const uint8_t* dst, size_t dst_len, void* out) try {
  return hash_to_group(2, msgs, msg_offsets, n, dst, dst_len, out);
}
API_CATCH

static int point_sum_entry(int group, const void* pts, const uint8_t* scalars, size_t n, int fmt, void* out) {
  if (!initialised()) return NOT_INIT();
  if (fmt != BLSGPU_FMT_RAW_PROJ && fmt != BLSGPU_FMT_RAW_AFFINE) return fail(BLSGPU_E_ARG, "fmt must be RAW_PROJ or RAW_AFFINE");
  if (!out || (n && !pts)) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  const size_t psz = point_bytes(group, fmt), osz = point_bytes(group, BLSGPU_FMT_RAW_PROJ), T = accumulate_lanes(n);
  int rc = arena_reserve(c, pad256(psz * n) + pad256(32 * n) + pad256(288 * T) + 4096 + (scalars ? msm_ws_bytes(n) : 0));
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_pts, *d_scal = nullptr;
  if ((rc = stage_in(c, pts, psz * n, &d_pts))) return rc;
  if (scalars && (rc = stage_in(c, scalars, 32 * n, &d_scal))) return rc;
  uint8_t* d_part = (uint8_t*)arena_take(c, 288 * T);
  if (!d_part) return fail(BLSGPU_E_HIP, "internal: arena too small");
  rc = with_group(group, [&](auto G) { return run_point_sum<G()>(c, (const uint8_t*)d_pts, fmt, (const uint8_t*)d_scal, nullptr, n, d_part, T); });
  if (rc) return rc;
  if ((rc = copy_out(c, out, d_part, osz))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
int blsgpu_sum_g1(const void* pts, size_t n, int fmt, void* out) { return point_sum_entry(1, pts, nullptr, n, fmt, out); }
int blsgpu_sum_g2(const void* pts, size_t n, int fmt, void* out) { return point_sum_entry(2, pts, nullptr, n, fmt, out); }
int blsgpu_msm_g1(const void* pts, const uint8_t* scalars, size_t n, int fmt, void* out) try {
  if (n && !scalars) return fail(BLSGPU_E_ARG, "null scalars");
  return point_sum_entry(1, pts, scalars, n, fmt, out);
}
API_CATCH
int blsgpu_msm_g2(const void* pts, const uint8_t* scalars, size_t n, int fmt, void* out) try {
  if (n && !scalars) return fail(BLSGPU_E_ARG, "null scalars");
  return point_sum_entry(2, pts, scalars, n, fmt, out);
}
API_CATCH

int blsgpu_pairing_product_is_one(const void* g1s, const void* g2s, size_t n, int fmt, int32_t* is_one) try {
  if (!initialised()) return NOT_INIT();
  if (fmt != BLSGPU_FMT_RAW_PROJ && fmt != BLSGPU_FMT_RAW_AFFINE) return fail(BLSGPU_E_ARG, "fmt must be RAW_PROJ or RAW_AFFINE");
  if (!is_one || (n && (!g1s || !g2s))) return fail(BLSGPU_E_ARG, "null argument");
  int32_t verdict = BLSGPU_OK;
  if (n > 0) {
    CTX_ACQUIRE(c);
    int rc = arena_reserve(c, pad256(point_bytes(1, fmt) * n) + pad256(point_bytes(2, fmt) * n) + pad256(4 * n) + 2 * pad256((size_t)WS_F_WORDS * 4 * n) + 4096);
    if (rc) return rc;
    c->arena_off = 0;
    const void *d1, *d2;
    if ((rc = stage_in(c, g1s, point_bytes(1, fmt) * n, &d1))) return rc;
    if ((rc = stage_in(c, g2s, point_bytes(2, fmt) * n, &d2))) return rc;
    Carver mem{c};
    int32_t* d_skip = mem.take<int32_t>(4 * n + 4);
    uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIR1_WORDS * 4 * n);
    uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n);
    if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
    KL(KID_PAIRS_AFF, k_pairs_to_affine, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d1, (const uint8_t*)d2, fmt, d_pairs, d_skip);
    size_t outputs = 0;
    if ((rc = run_miller_product(c, n, n, d_pairs, d_skip, d_f, &outputs))) return rc;
    if ((rc = run_f12_product_verdict(c, d_f, outputs, n, d_skip + n))) return rc;
    HIPCK(hipMemcpyAsync(&verdict, d_skip + n, 4, hipMemcpyDeviceToHost, c->stream));
    SYNC_FLUSH(c);
  }
  int32_t one = verdict == BLSGPU_OK ? 1 : 0;
  return put_i32(is_one, one);
}
API_CATCH

int blsgpu_serialize(int group, const void* pts, size_t n, int fmt_in, int fmt_out, void* out, int32_t* status) try {
  if (!initialised()) return NOT_INIT();
  if (group != 1 && group != 2) return fail(BLSGPU_E_ARG, "group must be 1 or 2");
  if ((fmt_in != BLSGPU_FMT_RAW_PROJ && fmt_in != BLSGPU_FMT_RAW_AFFINE) || (fmt_out != BLSGPU_FMT_COMPRESSED && fmt_out != BLSGPU_FMT_LEGACY))
    return fail(BLSGPU_E_ARG, "supported conversions: RAW_PROJ/RAW_AFFINE -> COMPRESSED/LEGACY");
  if (n == 0) return 0;
  if (!pts || !out) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  const size_t psz = point_bytes(group, fmt_in), osz = point_bytes(group, BLSGPU_FMT_COMPRESSED);
  int rc = arena_reserve(c, pad256(psz * n) + pad256(osz * n) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void* d_pts;
  if ((rc = stage_in(c, pts, psz * n, &d_pts))) return rc;
  uint8_t* d_out = stage_out<uint8_t>(c, out, osz * n);
  if (!d_out) return fail(BLSGPU_E_HIP, "internal: arena too small");
  int legacy = fmt_out == BLSGPU_FMT_LEGACY;
  with_group(group, [&](auto G) { KL(KID_COMPRESS, k_compress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_pts, fmt_in, legacy, d_out); });
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out, d_out, osz * n))) return rc;
  SYNC_FLUSH(c);
  if (status) {
    std::vector<int32_t> z(n, 0);
    HIPCK(hipMemcpy(status, z.data(), 4 * n, is_device_ptr(status) ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
  }
  return 0;
}
API_CATCH

/* ProofOfPossession::verify for n (pk, proof) pairs: pop_verify(pk, sig) = core_verify(pk, sig, pk.to_bytes(), POP_DST)
 * (reference src/proof_of_possession.rs:79-81, src/traits/sig_pop.rs:67-70; POP_DST src/impls/g1.rs:119, g2.rs:117). */
int blsgpu_pop_verify_batch(int sig_group, const void* pks, const void* proofs, size_t n, int fmt, int32_t* status) try {
  int rc = check_common(sig_group, 0, fmt);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!pks || !proofs || !status) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  const size_t pkb = pk_size(sig_group, fmt) * n, sgb = sig_size(sig_group, fmt) * n;
  size_t need = pad256(pkb) + pad256(sgb) + pad256(4 * n) + 2 * pad256((size_t)WS_PAIRS_WORDS * 4 * n) + 4096;
  if ((rc = arena_reserve(c, need))) return rc;
  c->arena_off = 0;
  const void *d_pks, *d_sigs;
  if ((rc = stage_in(c, pks, pkb, &d_pks))) return rc;
  if ((rc = stage_in(c, proofs, sgb, &d_sigs))) return rc;
  Carver mem{c};
  uint64_t* d_offs = mem.take<uint64_t>(16);
  int32_t* d_status = mem.take<int32_t>(4 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIRS_WORDS * 4 * n);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  HIPCK(hipMemsetAsync(d_offs, 0, 16, c->stream));
  const char* pd = sig_group == 1 ? "BLS_POP_BLS12381G1_XMD:SHA-256_SSWU_RO_POP_" : "BLS_POP_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";
  // mode 2: the message is the compressed key (single_msg = 1 keeps the unused message indexing in bounds)
  rc = run_verify_items(c, sig_group, 2, (const uint8_t*)d_pks, (const uint8_t*)d_sigs, fmt, (const uint8_t*)d_offs, d_offs, 1,
                        make_dst((const uint8_t*)pd, strlen(pd)), n, d_pairs, d_f, d_status);
  if (rc) return rc;
  if ((rc = status_out_and_sync(c, status, d_status, n))) return rc;
  return 0;
}
API_CATCH

/* Sign-side secure aggregation: aggregate_secure[_with_mode] / AggregateSignature::from_signatures_secure
 * (reference src/secure_aggregation.rs:110-169,338-352, src/aggregate_signature.rs:191-227): sig_agg = sum t_i * sig[idx_i]
 * over the keys in sorted order, where idx_i is the FIRST input position whose serialised key equals the i-th sorted key
 * (the reference's `position` search, so duplicate keys pick the first matching signature).  n == 0: the identity. */
int blsgpu_aggregate_secure(int sig_group, const void* pks, const void* sigs, size_t n, int ser_format, int fmt, void* out_sig,
                            int32_t* status) try {
  int rc = check_common(sig_group, 0, fmt);
  if (rc) return rc;
  if (!out_sig || !status || (n && (!pks || !sigs))) return fail(BLSGPU_E_ARG, "null argument");
  if ((rc = check_ser_format(sig_group, ser_format, false))) return rc;
  if (n >= 0xffffffffull) return fail(BLSGPU_E_ARG, "more than 2^32 - 2 keys");
  CTX_ACQUIRE(c);
  const size_t psz = pk_size(sig_group, fmt), ssz = sig_size(sig_group, fmt), width = pk_size(sig_group, BLSGPU_FMT_COMPRESSED), T = accumulate_lanes(n);
  const size_t osz = sig_size(sig_group, BLSGPU_FMT_RAW_PROJ);
  size_t need = pad256(psz * n) + pad256(ssz * n) + pad256(width * n) + pad256(288 * T) + 8192 + aggregate_secure_set_bytes(n, width);
  if ((rc = arena_reserve(c, need))) return rc;
  c->arena_off = 0;
  int32_t st = BLSGPU_OK;
  uint8_t* d_part = (uint8_t*)arena_take(c, 288 * T);
  int32_t* h_zero = (int32_t*)hsmall_take(c, 64);
  if (!d_part || !h_zero) return fail(BLSGPU_E_HIP, "internal: arena too small");
  *h_zero = 0;
  if (n == 0) {
    rc = with_group(sig_group, [&](auto G) { return run_point_sum<G()>(c, nullptr, fmt, nullptr, nullptr, 0, d_part, T); });
    if (rc) return rc;
  } else {
    const void *d_pks, *d_sigs;
    if ((rc = stage_in(c, pks, psz * n, &d_pks))) return rc;
    if ((rc = stage_in(c, sigs, ssz * n, &d_sigs))) return rc;
    Carver mem{c};
    uint8_t* d_bytes = mem.take<uint8_t>(width * n);
    int32_t* d_zero = mem.take<int32_t>(64);
    if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
    with_group(key_group(sig_group), [&](auto G) {
      KL(KID_COMPRESS, k_compress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_pks, fmt, ser_format, d_bytes);
    });
    HIPCK(hipGetLastError());
    HIPCK(hipMemsetAsync(d_zero, 0, 4, c->stream));
    if ((rc = run_aggregate_secure_set(c, sig_group, d_bytes, (const uint8_t*)d_sigs, n, width, fmt, d_zero, d_part, T))) return rc;
    HIPCK(hipMemcpyAsync(h_zero, d_zero, 4, hipMemcpyDeviceToHost, c->stream));
  }
  SYNC_FLUSH(c);
  if (*h_zero) st = BLSGPU_INVALID_COEFFICIENT;
  if (st == BLSGPU_OK) {
    if ((rc = copy_out(c, out_sig, d_part, osz))) return rc;
    SYNC_FLUSH(c);
  }
  return put_i32(status, st);
}
API_CATCH

int blsgpu_deserialize(int group, const uint8_t* bytes, size_t n, int fmt_in, void* out, int32_t* status) try {
  if (!initialised()) return NOT_INIT();
  if (group != 1 && group != 2) return fail(BLSGPU_E_ARG, "group must be 1 or 2");
  if (fmt_in != BLSGPU_FMT_COMPRESSED && fmt_in != BLSGPU_FMT_LEGACY) return fail(BLSGPU_E_ARG, "fmt_in must be COMPRESSED or LEGACY");
  if (n == 0) return 0;
  if (!bytes || !out || !status) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  const size_t isz = point_bytes(group, BLSGPU_FMT_COMPRESSED), osz = point_bytes(group, BLSGPU_FMT_RAW_PROJ);
  int rc = arena_reserve(c, pad256(isz * n) + pad256(osz * n) + pad256(4 * n) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void* d_in;
  if ((rc = stage_in(c, bytes, isz * n, &d_in))) return rc;
  uint8_t* d_out = stage_out<uint8_t>(c, out, osz * n);
  int32_t* d_st = stage_out<int32_t>(c, status, 4 * n);
  if (!d_out || !d_st) return fail(BLSGPU_E_HIP, "internal: arena too small");
  const int legacy = fmt_in == BLSGPU_FMT_LEGACY;
  with_group(group, [&](auto G) { KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_in, legacy, d_out, d_st, 0); });
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out, d_out, osz * n))) return rc;
  if ((rc = stage_back(c, status, d_st, 4 * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* Signature::<C>::try_from(&[u8]) / Vec<u8>::from(&Signature<C>) for n signatures (reference src/signature.rs:112-126): the
 * serde_bare form is the scheme as one byte (enum variant index 0 / 1 / 2) followed by the compressed point, 49 bytes
 * (Bls12381G1Impl) or 97 bytes (Bls12381G2Impl) per record -- the lengths asserted at src/signature.rs:285-286.
 * from_tagged: out_schemes[i] = tag, out = RAW_PROJ points (checked decompression on the device), status[i] = OK or
 * BAD_ENCODING (unknown tag or invalid point; the reference maps every serde error to InvalidInputs(..)). */
int blsgpu_signatures_from_tagged(int sig_group, const uint8_t* bytes, size_t n, uint8_t* out_schemes, void* out, int32_t* status) try {
  int rc = check_common(sig_group, 0, BLSGPU_FMT_RAW_PROJ);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!bytes || !out_schemes || !out || !status) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  const size_t width = sig_size(sig_group, BLSGPU_FMT_COMPRESSED), osz = sig_size(sig_group, BLSGPU_FMT_RAW_PROJ);
  if ((rc = arena_reserve(c, pad256((width + 1) * n) + pad256(width * n) + pad256(n) + pad256(osz * n) + pad256(4 * n) + 4096))) return rc;
  c->arena_off = 0;
  const void* d_in;
  if ((rc = stage_in(c, bytes, (width + 1) * n, &d_in))) return rc;
  Carver mem{c};
  uint8_t* d_bytes = mem.take<uint8_t>(width * n);
  uint8_t* d_tags = mem.stage_out<uint8_t>(out_schemes, n);
  uint8_t* d_out = mem.stage_out<uint8_t>(out, osz * n);
  int32_t* d_st = mem.stage_out<int32_t>(status, 4 * n);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  KL(KID_DECOMPRESS, k_untag, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, width, (const uint8_t*)d_in, d_bytes, d_tags, d_st);
  HIPCK(hipMemsetAsync(d_out, 0, osz * n, c->stream));      // records with a bad tag are not decoded: leave the identity encoding
  with_group(sig_group, [&](auto G) { KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_bytes, 0, d_out, d_st, 1); });
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out_schemes, d_tags, n))) return rc;
  if ((rc = stage_back(c, out, d_out, osz * n))) return rc;
  if ((rc = stage_back(c, status, d_st, 4 * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH
int blsgpu_signatures_to_tagged(int sig_group, const uint8_t* schemes, const void* sigs, size_t n, int fmt, uint8_t* out) try {
  int rc = check_common(sig_group, 0, fmt);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!schemes || !sigs || !out) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  const size_t width = sig_size(sig_group, BLSGPU_FMT_COMPRESSED), psz = sig_size(sig_group, fmt);
  if ((rc = arena_reserve(c, pad256(psz * n) + pad256(n) + pad256(width * n) + pad256((width + 1) * n) + 4096))) return rc;
  c->arena_off = 0;
  const void *d_pts, *d_tags;
  if ((rc = stage_in(c, sigs, psz * n, &d_pts))) return rc;
  if ((rc = stage_in(c, schemes, n, &d_tags))) return rc;
  uint8_t* d_bytes = (uint8_t*)arena_take(c, width * n);
  uint8_t* d_out = stage_out<uint8_t>(c, out, (width + 1) * n);
  if (!d_bytes || !d_out) return fail(BLSGPU_E_HIP, "internal: arena too small");
  with_group(sig_group, [&](auto G) { KL(KID_COMPRESS, k_compress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_pts, fmt, 0, d_bytes); });
  KL(KID_COMPRESS, k_tag, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, width, (const uint8_t*)d_tags, (const uint8_t*)d_bytes, d_out);
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out, d_out, (width + 1) * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* Self-test / measurement hook of the row-wide Fp multiplier (csrc/wide.cuh): out[i] = a[i] * b[i]^reps in Fp, 48-byte Montgomery
 * words per element (the Fp coordinate format of RAW_PROJ).  reps > 1 chains the multiplications: with n <= 4 (one wave) the
 * call's device time / reps is the latency of one multiplication of a dependent chain. */
int blsgpu_debug_wide_mul(const uint8_t* a, const uint8_t* b, size_t n, int reps, uint8_t* out) try {
  if (!initialised()) return NOT_INIT();
  if (n == 0) return 0;
  if (!a || !b || !out || reps < 1) return fail(BLSGPU_E_ARG, "bad argument");
  CTX_ACQUIRE(c);
  int rc = arena_reserve(c, 3 * pad256(48 * n) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_a, *d_b;
  if ((rc = stage_in(c, a, 48 * n, &d_a))) return rc;
  if ((rc = stage_in(c, b, 48 * n, &d_b))) return rc;
  uint8_t* d_out = stage_out<uint8_t>(c, out, 48 * n);
  if (!d_out) return fail(BLSGPU_E_HIP, "internal: arena too small");
  // BLSGPU_WIDE_TEST_BLOCK=256: sixteen items per 256-thread workgroup (the engine's shape) instead of four per wave
  const unsigned tb = knobs().wide_test_block == 256 ? 256 : 64, per = tb / 16;
  KL(KID_WIDE, k_wide_mul_test, dim3((unsigned)((n + per - 1) / per)), dim3(tb), n, (const uint8_t*)d_a, (const uint8_t*)d_b, d_out, reps);
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out, d_out, 48 * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* Self-test / measurement hook of the row-wide engine (csrc/wide_engine.cuh): runs a caller-supplied program (two words per
 * step, the format of csrc/wide_tables.cuh) `reps` times on one workgroup with F = U = W = ACC = the Fp12 at f_in (twelve
 * 48-byte Montgomery elements, coefficient order of the tables) and T = 0, and returns T.  Steps may only name the Fp12
 * arrays F, T, U, W, ACC. */
int blsgpu_debug_wide_program(const uint32_t* prog, size_t len, int reps, const uint8_t* f_in, uint8_t* t_out) try {
  if (!initialised()) return NOT_INIT();
  if (!prog || !f_in || !t_out || reps < 1 || len < 1 || is_device_ptr(prog)) return fail(BLSGPU_E_ARG, "bad argument");
  if (!wide_prog_is_fp12(prog, len)) return fail(BLSGPU_E_ARG, "program: too long, or a step is not an Fp12 operation on F, T, U, W, ACC");
  CTX_ACQUIRE(c);
  int rc = arena_reserve(c, pad256(8 * len) + 2 * pad256(576) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_prog, *d_in;
  if ((rc = stage_in(c, prog, 8 * len, &d_prog))) return rc;
  if ((rc = stage_in(c, f_in, 576, &d_in))) return rc;
  uint8_t* d_out = stage_out<uint8_t>(c, t_out, 576);
  if (!d_out) return fail(BLSGPU_E_HIP, "internal: arena too small");
  KL(KID_WIDE, k_wide_prog_test, dim3(1), dim3(WIDE_ENGINE_BLOCK), (const uint32_t*)d_prog, (int)len, reps, (const uint8_t*)d_in, d_out);
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, t_out, d_out, 576))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* Self-test hook of the row-wide engine, operation by operation (include/blsgpu.h): k_wide_steps_test on n workgroups.  The program
 * is validated here -- wide_steps_ok: table operations and FPINV only, every reference inside the store -- so that nothing a caller
 * passes can make a workgroup wait on a partner or address LDS outside its value store. */
int blsgpu_debug_wide_steps(int set, const uint32_t* prog, size_t len, int reps, size_t n, const uint32_t* in_idx, size_t n_in, const int32_t* in,
                            int32_t fill, const uint32_t* out_idx, size_t n_out, int32_t* out) try {
  if (!initialised()) return NOT_INIT();
  if ((set != 0 && set != 1) || !prog || reps < 1 || reps > 4096 || n < 1 || n > 4096 || n_out < 1 || !out_idx || !out || (n_in && (!in_idx || !in)) ||
      is_device_ptr(prog) || is_device_ptr(in_idx) || is_device_ptr(out_idx))
    return fail(BLSGPU_E_ARG, "bad argument");
  if (!wide_steps_ok(set, prog, len)) return fail(BLSGPU_E_ARG, "program: empty, too long, not a table operation of the set, or a reference past the value store");
  const size_t nv = (size_t)wide_steps_nv(set);
  if (n_in > nv || n_out > nv) return fail(BLSGPU_E_ARG, "more values than the store holds");
  for (size_t k = 0; k < n_in; k++)
    if (in_idx[k] >= nv) return fail(BLSGPU_E_ARG, "input value index past the value store");
  for (size_t k = 0; k < n_out; k++)
    if (out_idx[k] >= nv) return fail(BLSGPU_E_ARG, "output value index past the value store");
  CTX_ACQUIRE(c);
  const size_t in_bytes = 64 * n_in * n, out_bytes = 64 * n_out * n;
  int rc = arena_reserve(c, pad256(8 * len) + pad256(4 * n_in + 4) + pad256(4 * n_out) + pad256(in_bytes + 4) + pad256(out_bytes) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_prog, *d_ii = nullptr, *d_oi, *d_in = nullptr;
  if ((rc = stage_in(c, prog, 8 * len, &d_prog))) return rc;
  if (n_in && (rc = stage_in(c, in_idx, 4 * n_in, &d_ii))) return rc;
  if ((rc = stage_in(c, out_idx, 4 * n_out, &d_oi))) return rc;
  if (n_in && (rc = stage_in(c, in, in_bytes, &d_in))) return rc;
  int32_t* d_out = stage_out<int32_t>(c, out, out_bytes);
  if (!d_out) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if (set == 0)
    KL(KID_WIDE, k_wide_steps_test<0>, dim3((unsigned)n), dim3(WIDE_ENGINE_BLOCK), (const uint32_t*)d_prog, (int)len, reps, (int)n_in, (const uint32_t*)d_ii,
       (const int32_t*)d_in, (uint32_t)fill, (int)n_out, (const uint32_t*)d_oi, d_out);
  else
    KL(KID_WIDE, k_wide_steps_test<1>, dim3((unsigned)n), dim3(WIDE_ENGINE_BLOCK), (const uint32_t*)d_prog, (int)len, reps, (int)n_in, (const uint32_t*)d_ii,
       (const int32_t*)d_in, (uint32_t)fill, (int)n_out, (const uint32_t*)d_oi, d_out);
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out, d_out, out_bytes))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* Self-test hook of the batch final exponentiation + verdict (run_pairing2's two-lane forms) on caller-supplied Fp12 records (576
 * bytes, the record format of blsgpu_fp12_product_is_one).  form 0: k_finalexp2s, 1: k_finalexp_seg + k_cyc_run4, both chunk by
 * chunk through launch_finalexp_chunk with the line workspace as the value store, as the verify path runs them; 2: k_finalexps.
 * chunk: items per chunk of forms 0 and 1 (0: the library's).  status is in/out: an entry that is not BLSGPU_OK on entry is
 * skipped and left as it is. */
int blsgpu_debug_finalexp_batch(const void* f12s, size_t n, int form, size_t chunk, int32_t* status) try {
  if (!initialised()) return NOT_INIT();
  if (n == 0) return 0;
  if (!f12s || !status || form < 0 || form > 2) return fail(BLSGPU_E_ARG, "bad argument");
  CTX_ACQUIRE(c);
  int rc = arena_reserve(c, pad256(576 * n) + pad256(4 * n) + pad256((size_t)WS_F_WORDS * 4 * n) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_in, *d_st;
  if ((rc = stage_in(c, f12s, 576 * n, &d_in))) return rc;
  if ((rc = stage_in(c, status, 4 * n, &d_st))) return rc;
  int32_t* d_status = (int32_t*)d_st;
  uint32_t* d_f = (uint32_t*)arena_take(c, (size_t)WS_F_WORDS * 4 * n);
  if (!d_f) return fail(BLSGPU_E_HIP, "internal: arena too small");
  KL(KID_F12_IO, k_f12_import, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_in, d_f, n);
  if (form == 2) {
    KL(KID_FINALEXP_V1, k_finalexps, dim3(blocks_for(2 * n)), dim3(BLS_BLOCK), n, d_f, d_status);
  } else {
    if (chunk == 0) chunk = miller_chunk_items() ? miller_chunk_items() : n;
    if (chunk > n) chunk = n;
    if (lines_reserve(c, (size_t)FX_STORE_WORDS * 4 * row_stride(lanes_for(chunk)))) return fail(BLSGPU_E_HIP, "no room for the value store");
    for (size_t first = 0; first < n; first += chunk) launch_finalexp_chunk(c, n, first, n - first < chunk ? n - first : chunk, d_f, d_status, form == 1);
  }
  HIPCK(hipGetLastError());
  if (d_status != status) return copy_out_and_sync(c, status, d_status, 4 * n);
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* Self-test hook of the field leaves and the lane-split tower, one operation at a time on caller-supplied limb vectors (fourteen
 * signed 32-bit limbs per Fp, the internal form of fp.cuh): the operation table is csrc/debug_ops.h.  Host pointers only. */
namespace {
struct dbg_shape {
  int op, lanes, n_in, n_out, n_par, chain;
};
const dbg_shape DBG_SHAPES[] = {
#define X(name, id, lanes, nin, nout, npar, chain) {id, lanes, nin, nout, npar, chain},
    BLS_DEBUG_OPS(X)
#undef X
};
const dbg_shape* dbg_find(int op) {
  for (const dbg_shape& s : DBG_SHAPES)
    if (s.op == op) return &s;
  return nullptr;
}
}  // namespace
int blsgpu_debug_field_op_shape(int op, int* lanes, int* n_in, int* n_out, int* n_par, int* chain) {
  const dbg_shape* s = dbg_find(op);
  if (!s || !lanes || !n_in || !n_out || !n_par || !chain) return fail(BLSGPU_E_ARG, "unknown operation");
  *lanes = s->lanes;
  *n_in = s->n_in;
  *n_out = s->n_out;
  *n_par = s->n_par;
  *chain = s->chain;
  return 0;
}
int blsgpu_debug_field_op(int op, const int32_t* in, size_t n, int reps, int32_t* out) try {
  if (!initialised()) return NOT_INIT();
  const dbg_shape* s = dbg_find(op);
  if (!s) return fail(BLSGPU_E_ARG, "unknown operation");
  if (n == 0) return 0;
  if (!in || !out || reps < 1 || (reps > 1 && !s->chain) || n > ((size_t)1 << 20) || is_device_ptr(in) || is_device_ptr(out)) return fail(BLSGPU_E_ARG, "bad argument");
  CTX_ACQUIRE(c);
  const int rec_in = s->n_in * DBG_NL + s->n_par, rec_out = s->n_out * DBG_NL;
  int rc = arena_reserve(c, pad256((size_t)4 * rec_in * n) + pad256((size_t)4 * rec_out * n) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void* d_in;
  if ((rc = stage_in(c, in, (size_t)4 * rec_in * n, &d_in))) return rc;
  int32_t* d_out = stage_out<int32_t>(c, out, (size_t)4 * rec_out * n);
  if (!d_out) return fail(BLSGPU_E_HIP, "internal: arena too small");
  const dim3 grid(blocks_for((size_t)s->lanes * n)), block(BLS_BLOCK);
#define DBG_LAUNCH(kern) KL(KID_DEBUG_OPS, kern, grid, block, op, n, reps, (const int32_t*)d_in, rec_in, d_out, rec_out)
  if (s->lanes == 64) DBG_LAUNCH(k_dbg_coop);      // one workgroup per item: blocks_for(64 n) = n
  else if (op >= DBG_MILLER1_DBL) {                // the Miller steps, the merges and the row evaluation
    if (s->lanes == 1) DBG_LAUNCH(k_dbg_miller1);
    else DBG_LAUNCH(k_dbg_miller2s);
  } else if (op >= DBG_G1_DBL) {                   // the curve layer
    if (s->lanes == 1) DBG_LAUNCH(k_dbg_pt1);
    else if (s->lanes == 2) DBG_LAUNCH(k_dbg_pt2s);
    else DBG_LAUNCH(k_dbg_g2q);
  } else if (s->lanes == 1) DBG_LAUNCH(k_dbg_fp1);
  else if (op < DBG_F12_SH_SQR) DBG_LAUNCH(k_dbg_fp2s);
  else if (op < DBG_CYC_C_SQR) DBG_LAUNCH(k_dbg_f12acc);
  else if (op < DBG_F12_POW_X) DBG_LAUNCH(k_dbg_cyc);
  else DBG_LAUNCH(k_dbg_f12misc);
#undef DBG_LAUNCH
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out, d_out, (size_t)4 * rec_out * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* Self-test hook of hash-to-curve behind expand_message_xmd (include/blsgpu.h): the kernels of run_hash_group, launch_hash_g1_small and
 * launch_hash_g2_small in their UB = true form (tu_debug_h2c.hip, tu_debug_h2c_wide.hip), launched with the grids and flags those
 * functions use, on caller-supplied uniform bytes. */
int blsgpu_debug_map_to_curve(int group, int path, int uncleared, const uint8_t* uniform, size_t n, void* out) try {
  if (!initialised()) return NOT_INIT();
  bool known = false;
  if (group == 1) {
    known = ((path == BLSGPU_H2C_LANE || path == BLSGPU_H2C_PAIR || path == BLSGPU_H2C_WIDE || path == BLSGPU_H2C_ENGINE) && (uncleared == 0 || uncleared == 1)) ||
            (path == BLSGPU_H2C_WIDE_REC && uncleared == 1);
  } else if (group == 2) {
    known = ((path == BLSGPU_H2C_LANE || path == BLSGPU_H2C_ENGINE || path == BLSGPU_H2C_MAPS_TAIL || path == BLSGPU_H2C_PAIR_CLEAR_WIDE) && uncleared == 0) ||
            (path == BLSGPU_H2C_PAIR && (uncleared == 0 || uncleared == 1));
  }
  if (!known) return fail(BLSGPU_E_ARG, "no launch of the library uses this (group, path, uncleared)");
  if (n == 0) return 0;
  if (!uniform || !out || n > 4096 || is_device_ptr(uniform) || is_device_ptr(out)) return fail(BLSGPU_E_ARG, "bad argument");
  CTX_ACQUIRE(c);
  const size_t ubytes = group == 1 ? 128 : 256, osz = point_bytes(group, BLSGPU_FMT_RAW_PROJ);
  const bool record = group == 1 && (path == BLSGPU_H2C_WIDE_REC || (path == BLSGPU_H2C_ENGINE && uncleared));
  const size_t rec_bytes = record ? (size_t)WREC_WORDS * 4 * n : 0, maps_bytes = path == BLSGPU_H2C_MAPS_TAIL ? 768 * n : 0;
  int rc = arena_reserve(c, pad256(ubytes * n) + pad256(osz * n) + pad256(rec_bytes) + pad256(maps_bytes) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void* d_in;
  if ((rc = stage_in(c, uniform, ubytes * n, &d_in))) return rc;
  uint8_t* d_out = stage_out<uint8_t>(c, out, osz * n);
  uint32_t* d_rec = record ? (uint32_t*)arena_take(c, rec_bytes) : nullptr;
  uint32_t* d_maps = maps_bytes ? (uint32_t*)arena_take(c, maps_bytes) : nullptr;
  if (!d_out || (record && !d_rec) || (maps_bytes && !d_maps)) return fail(BLSGPU_E_HIP, "internal: arena too small");
  const uint8_t* d_ub = (const uint8_t*)d_in;
  const uint64_t* no_offs = nullptr;
  dst_arg d;
  memset(&d, 0, sizeof d);
  const dim3 one(BLS_BLOCK), wg(WIDE_ENGINE_BLOCK), per_item((unsigned)n);
  const int two = path == BLSGPU_H2C_LANE ? 0 : 1;
  if (group == 1) {
    if (path == BLSGPU_H2C_LANE || path == BLSGPU_H2C_PAIR)
      KL(KID_DEBUG_OPS, k_hash_to_g1<true>, dim3(blocks_for(two ? 2 * n : n)), one, n, d_ub, no_offs, d, d_out, two | (uncleared ? 2 : 0));
    else if (path == BLSGPU_H2C_WIDE)
      KL(KID_DEBUG_OPS, k_hash_to_g1_wide<true>, per_item, one, n, d_ub, no_offs, uncleared ? 2 : 0, d, d_out, (uint32_t*)nullptr);
    else if (path == BLSGPU_H2C_WIDE_REC)
      KL(KID_DEBUG_OPS, k_hash_to_g1_wide<true>, per_item, one, n, d_ub, no_offs, 0, d, (uint8_t*)nullptr, d_rec);
    else if (uncleared)
      KL(KID_DEBUG_OPS, k_hash_to_g1_engine<true>, per_item, wg, n, d_ub, no_offs, 0, d, (uint8_t*)nullptr, d_rec);
    else
      KL(KID_DEBUG_OPS, k_hash_to_g1_engine<true>, per_item, wg, n, d_ub, no_offs, 0, d, d_out, (uint32_t*)nullptr);
    if (record) KL(KID_DEBUG_OPS, k_dbg_rec_g1_to_raw, dim3(blocks_for(n)), one, n, (const uint32_t*)d_rec, d_out);
  } else {
    if (path == BLSGPU_H2C_LANE || path == BLSGPU_H2C_PAIR)
      KL(KID_DEBUG_OPS, k_hash_to_g2<true>, dim3(blocks_for(two ? 2 * n : n)), one, n, d_ub, no_offs, d, d_out, two | (uncleared ? 2 : 0));
    else if (path == BLSGPU_H2C_PAIR_CLEAR_WIDE) {
      KL(KID_DEBUG_OPS, k_hash_to_g2<true>, dim3(blocks_for(2 * n)), one, n, d_ub, no_offs, d, d_out, 3);
      KL(KID_DEBUG_OPS, k_g2_clear_wide, per_item, wg, n, d_out);
    } else if (path == BLSGPU_H2C_ENGINE)
      KL(KID_DEBUG_OPS, k_hash_to_g2_engine<true>, per_item, wg, n, d_ub, no_offs, 0, d, d_out, (uint32_t*)nullptr);
    else {
      KL(KID_DEBUG_OPS, k_hash_to_g2_maps<true>, per_item, one, n, d_ub, no_offs, 0, d, d_maps);
      KL(KID_DEBUG_OPS, k_g2_hash_tail_wide, per_item, wg, n, (const uint32_t*)d_maps, d_out, (uint32_t*)nullptr);
    }
  }
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out, d_out, osz * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* Self-test hook of the accumulator's kernel: k_millerf2s, launched as run_pairing2 launches it, on a caller-supplied line table.
 * lines: n x 68 entries x five Fp2 coefficients (c0, c2, c4, c3, c5 of tower.cuh line5_t; c0 and c1 of each, fourteen limbs
 * each), written into the context's line workspace in the library's word-major layout.  status: n entries; an item that is not
 * BLSGPU_OK is skipped, as the verify path skips it, and its output is left zero.  out_f12: n x twelve limb vectors, tower order. */
int blsgpu_debug_millerf(const int32_t* lines, size_t n, const int32_t* status, int32_t* out_f12) try {
  if (!initialised()) return NOT_INIT();
  if (n == 0) return 0;
  if (!lines || !status || !out_f12 || n > 4096 || is_device_ptr(lines) || is_device_ptr(status) || is_device_ptr(out_f12)) return fail(BLSGPU_E_ARG, "bad argument");
  CTX_ACQUIRE(c);
  const size_t nlanes = lanes_for(n), lanes = row_stride(nlanes);
  const size_t line_words = (size_t)MILLER_ENTRIES * LINE5_WORDS * lanes;
  int rc = arena_reserve(c, pad256(4 * n) + 2 * pad256((size_t)WS_F_WORDS * 4 * n) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  if (lines_reserve(c, line_words * 4)) return fail(BLSGPU_E_HIP, "no room for the line workspace");
  // lines[(e * LINE5_WORDS + w) * lanes + t]: word w = 14 * (coefficient number) + limb, lane t = 2 * item + component
  std::vector<uint32_t> h(line_words, 0u);
  for (size_t i = 0; i < n; i++)
    for (size_t e = 0; e < MILLER_ENTRIES; e++)
      for (size_t k = 0; k < 5; k++)
        for (size_t comp = 0; comp < 2; comp++)
          for (size_t l = 0; l < FP_NL; l++)
            h[(e * LINE5_WORDS + k * FP_NL + l) * lanes + 2 * i + comp] = (uint32_t)lines[(((i * MILLER_ENTRIES + e) * 5 + k) * 2 + comp) * FP_NL + l];
  HIPCK(hipMemcpyAsync(c->lines_ws, h.data(), line_words * 4, hipMemcpyHostToDevice, c->stream));
  HIPCK(hipStreamSynchronize(c->stream));           // h leaves scope after the call; pageable memory
  const void* d_st;
  if ((rc = stage_in(c, status, 4 * n, &d_st))) return rc;
  uint32_t* d_f = (uint32_t*)arena_take(c, (size_t)WS_F_WORDS * 4 * n);
  if (!d_f) return fail(BLSGPU_E_HIP, "internal: arena too small");
  HIPCK(hipMemsetAsync(d_f, 0, (size_t)WS_F_WORDS * 4 * n, c->stream));
  KL(KID_MILLER2, k_millerf2s, dim3((unsigned)(nlanes / BLS_BLOCK)), dim3(BLS_BLOCK), n, (size_t)0, n, (const int32_t*)d_st, (const uint32_t*)c->lines_ws, lanes, d_f);
  HIPCK(hipGetLastError());
  std::vector<uint32_t> f((size_t)WS_F_WORDS * n);
  HIPCK(hipMemcpyAsync(f.data(), d_f, f.size() * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCK(hipStreamSynchronize(c->stream));
  // Fp12 workspace: word w of item i at fws[w * n + i], w = 28 * (Fp2 in tower order) + 14 * component + limb
  for (size_t i = 0; i < n; i++)
    for (size_t w = 0; w < WS_F_WORDS; w++) out_f12[i * WS_F_WORDS + w] = (int32_t)f[w * n + i];
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* Self-test hook of the wave-cooperative pairing kernels on caller-supplied pairs (include/blsgpu.h).  pairs: n x twelve limb vectors
 * (P.x, P.y, Q.x.c0, Q.x.c1, Q.y.c0, Q.y.c1 of pair 0, then of pair 1; reduced form), written into a pair workspace in the layout
 * run_pairing2 reads: word w = 14 * vector + limb of item i at pairs_ws[w * n + i].  Modes 0 and 1 go through
 * launch_pairing_coop, the launch of run_pairing2 (debug_pairing_coop); mode 2 launches k_finalexp_coop as run_f12_product_verdict does. */
int blsgpu_debug_coop_pairing(int mode, int fixed_g2, const int32_t* in, size_t n, int32_t* status, int32_t* out_f12) try {
  if (!initialised()) return NOT_INIT();
  if (n == 0) return 0;
  if (!in || !status || mode < 0 || mode > 2 || fixed_g2 < 0 || fixed_g2 > 2 || n > 4096 || (mode == 0 && !out_f12) || is_device_ptr(in) || is_device_ptr(status) ||
      is_device_ptr(out_f12))
    return fail(BLSGPU_E_ARG, "bad argument");
  CTX_ACQUIRE(c);
  const size_t rec = mode == 2 ? WS_F_WORDS : WS_PAIRS_WORDS;       // words per item of the input workspace
  int rc = arena_reserve(c, pad256(rec * 4 * n) + pad256(4 * n) + pad256((size_t)WIDE_EASY_WORDS * 4 * n) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  DebugStaged s;
  if ((rc = debug_stage(c, in, rec, n, status, &s))) return rc;
  if (mode != 2) return debug_pairing_coop(c, mode, pairs_walked(fixed_g2), s, n, status, out_f12);
  for (size_t i = 0; i < n; i++)          // one launch per live item: the item's column is slot 0 of a workspace of stride n
    if (status[i] == BLS_OK) KL(KID_FINALEXP_ONE, k_finalexp_coop, dim3(1), dim3(BLS_BLOCK), s.pairs + i, n, s.status + i);
  HIPCK(hipGetLastError());
  return copy_out_and_sync(c, status, s.status, 4 * n);
}
API_CATCH

int blsgpu_sign_batch(int sig_group, int scheme, const uint8_t* sks, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n,
                      void* out_pks, void* out_sigs) try {
  int rc = check_common(sig_group, scheme, BLSGPU_FMT_RAW_PROJ);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!sks || !msg_offsets || !out_pks || !out_sigs) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  uint64_t total = 0;
  if (is_device_ptr(msg_offsets)) HIPCK(hipMemcpy(&total, msg_offsets + n, 8, hipMemcpyDeviceToHost));
  else total = msg_offsets[n];
  const size_t pkb = pk_size(sig_group, 0) * n, sgb = sig_size(sig_group, 0) * n;
  if ((rc = arena_reserve(c, pad256(32 * n) + pad256(total) + pad256(8 * (n + 1)) + pad256(pkb) + pad256(sgb) + 4096))) return rc;
  c->arena_off = 0;
  const void *d_sks, *d_msgs, *d_offs;
  if ((rc = stage_in(c, sks, 32 * n, &d_sks))) return rc;
  if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
  if ((rc = stage_in(c, msg_offsets, 8 * (n + 1), &d_offs))) return rc;
  uint8_t* d_pks = stage_out<uint8_t>(c, out_pks, pkb);
  uint8_t* d_sigs = stage_out<uint8_t>(c, out_sigs, sgb);
  if (!d_pks || !d_sigs) return fail(BLSGPU_E_HIP, "internal: arena too small");
  dst_arg dst = scheme_dst(sig_group, scheme);
  int aug = scheme == BLSGPU_SCHEME_AUG;
  with_group(sig_group, [&](auto G) {
    KL(KID_SIGN, k_sign<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_sks, aug, (const uint8_t*)d_msgs, (const uint64_t*)d_offs, dst, d_pks, d_sigs);
  });
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out_pks, d_pks, pkb))) return rc;
  if ((rc = stage_back(c, out_sigs, d_sigs, sgb))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* ---- sharded aggregate verify: the local part of core_aggregate_verify (reference
 * src/traits/sig_core.rs:149-178) for a contiguous shard of the (pk, msg) pairs.  out_f12 = product of the Miller
 * values of the shard's pairs [times the (sig, -g) pair when sig != NULL] BEFORE the final exponentiation, as a
 * 576-byte record; *first_bad = local index of the first identity public key, n when the signature is the identity,
 * or -1.  Duplicate-message detection is global and stays with the caller. */
int blsgpu_aggregate_partial(int sig_group, int scheme, const void* pks, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n,
                             const void* sig, int fmt, void* out_f12, int64_t* first_bad) try {
  int rc = check_common(sig_group, scheme, fmt);
  if (rc) return rc;
  if (!out_f12 || !first_bad || !msg_offsets || (n && !pks)) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  uint64_t total = 0;
  if (is_device_ptr(msg_offsets)) HIPCK(hipMemcpy(&total, msg_offsets + n, 8, hipMemcpyDeviceToHost));
  else total = msg_offsets[n];
  const size_t m = n + 1, psz = pk_size(sig_group, fmt);
  size_t need = pad256(psz * n) + pad256(sig_size(sig_group, fmt)) + pad256(total) + pad256(8 * m) + pad256(4 * m) +
                2 * pad256((size_t)WS_PAIRS_WORDS * 4 * m) + 8192;
  if ((rc = arena_reserve(c, need))) return rc;
  c->arena_off = 0;
  const void *d_pks, *d_sig = nullptr, *d_msgs, *d_offs;
  if ((rc = stage_in(c, pks, psz * n, &d_pks))) return rc;
  if (sig && (rc = stage_in(c, sig, sig_size(sig_group, fmt), &d_sig))) return rc;
  if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
  if ((rc = stage_in(c, msg_offsets, 8 * m, &d_offs))) return rc;
  // outputs may be device pointers (the sharded caller hands them to RCCL as they are): nothing crosses to the host then
  uint8_t* d_rec = stage_out<uint8_t>(c, out_f12, 576);
  int64_t* d_first = stage_out<int64_t>(c, first_bad, 64);
  if (!d_rec || !d_first) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if ((rc = aggregate_enqueue(c, sig_group, scheme, (const uint8_t*)d_pks, (const uint8_t*)d_sig, fmt, (const uint8_t*)d_msgs,
                              (const uint64_t*)d_offs, n, d_first, nullptr, d_rec)))
    return rc;
  if ((rc = stage_back(c, out_f12, d_rec, 576))) return rc;
  if ((rc = stage_back(c, first_bad, d_first, 8))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* BlsSignatureCore::core_verify(pk, sig, msg, dst) with an explicit DST (reference src/traits/sig_core.rs:120-146):
 * n items share one DST; no message augmentation.  Used by the sharded verify_secure tail and by PoP checks
 * (pop_verify = core_verify(pk, sig, pk_bytes, POP_DST), src/traits/sig_pop.rs:67-70). */
static int core_verify_entry(int sig_group, const dst_arg& dst, int aug, const void* pks, const void* sigs, const uint8_t* msgs,
                             const uint64_t* msg_offsets, size_t n, int fmt, int32_t* status) {
  int rc = 0;
  if (n == 0) return 0;
  if (!pks || !sigs || !msg_offsets || !status) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  uint64_t total = 0;
  if (is_device_ptr(msg_offsets)) HIPCK(hipMemcpy(&total, msg_offsets + n, 8, hipMemcpyDeviceToHost));
  else total = msg_offsets[n];
  const size_t pkb = pk_size(sig_group, fmt) * n, sgb = sig_size(sig_group, fmt) * n;
  size_t need = pad256(pkb) + pad256(sgb) + pad256(total) + pad256(8 * (n + 1)) + pad256(4 * n) + 2 * pad256((size_t)WS_PAIRS_WORDS * 4 * n) + 4096;
  if ((rc = arena_reserve(c, need))) return rc;
  c->arena_off = 0;
  const void *d_pks, *d_sigs, *d_msgs, *d_offs;
  if ((rc = stage_in(c, pks, pkb, &d_pks))) return rc;
  if ((rc = stage_in(c, sigs, sgb, &d_sigs))) return rc;
  if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
  if ((rc = stage_in(c, msg_offsets, 8 * (n + 1), &d_offs))) return rc;
  Carver mem{c};
  int32_t* d_status = mem.take<int32_t>(4 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIRS_WORDS * 4 * n);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  rc = run_verify_items(c, sig_group, aug, (const uint8_t*)d_pks, (const uint8_t*)d_sigs, fmt, (const uint8_t*)d_msgs, (const uint64_t*)d_offs, 0,
                        dst, n, d_pairs, d_f, d_status);
  if (rc) return rc;
  if ((rc = status_out_and_sync(c, status, d_status, n))) return rc;
  return 0;
}
int blsgpu_core_verify(int sig_group, const uint8_t* dst, size_t dst_len, const void* pks, const void* sigs, const uint8_t* msgs,
                       const uint64_t* msg_offsets, size_t n, int fmt, int32_t* status) try {
  int rc = check_common(sig_group, 0, fmt);
  if (rc) return rc;
  if (!dst && dst_len) return fail(BLSGPU_E_ARG, "null dst with a non-zero length");
  return core_verify_entry(sig_group, make_dst(dst, dst_len), 0, pks, sigs, msgs, msg_offsets, n, fmt, status);
}
API_CATCH

/* core_verify for n items whose message points H(m_i) are already known (RAW_PROJ, from blsgpu_hash_to_g1/g2 under the
 * scheme's DST): the identity checks of reference src/traits/sig_core.rs:126-135 in the reference's order, then
 * e(H(m), pk) * e(sig, -g) == 1 (:137-145).  Lets a caller hash the message while it is still adding up or exchanging the
 * keys (the sharded MultiSignature::verify / verify_secure of agora-blsful_amd/dist.py do). */
int blsgpu_core_verify_hashed(int sig_group, const void* pks, const void* sigs, const void* hashes, size_t n, int32_t* status) try {
  int rc = check_common(sig_group, 0, BLSGPU_FMT_RAW_PROJ);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!pks || !sigs || !hashes || !status) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  const size_t pkb = pk_size(sig_group, 0) * n, sgb = sig_size(sig_group, 0) * n;
  size_t need = pad256(pkb) + 2 * pad256(sgb) + pad256(4 * n) + 2 * pad256((size_t)WS_PAIRS_WORDS * 4 * n) + 4096;
  if ((rc = arena_reserve(c, need))) return rc;
  c->arena_off = 0;
  const void *d_pks, *d_sigs, *d_h;
  if ((rc = stage_in(c, pks, pkb, &d_pks))) return rc;
  if ((rc = stage_in(c, sigs, sgb, &d_sigs))) return rc;
  if ((rc = stage_in(c, hashes, sgb, &d_h))) return rc;
  Carver mem{c};
  int32_t* d_status = mem.take<int32_t>(4 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIRS_WORDS * 4 * n);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  with_group(sig_group, [&](auto G) {
    KL(KID_PREPARE, k_prepare_hashed<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_pks, (const uint8_t*)d_sigs, (const uint8_t*)d_h, d_pairs, d_status, 0);
  });
  if ((rc = run_pairing2(c, n, d_pairs, d_f, d_status, pairs_walked(sig_group == 1 ? 1 : 0)))) return rc;
  if ((rc = status_out_and_sync(c, status, d_status, n))) return rc;
  return 0;
}
API_CATCH

/* SignCryptCiphertext::is_valid for n ciphertexts (reference src/sign_crypt_ciphertext.rs:86-101 -> BlsSignCrypt::valid,
 * src/traits/sign_crypt.rs:69-77): W' = H(U.to_bytes() || V) under the scheme's DST, then e(W, -g) * e(W', U) == 1 with
 * U and W not the identity.  That is core_verify(pk := U, sig := W, msg := U.to_bytes() || V, dst): the key-prefixed hash is
 * the augmentation path of k_prepare.  status[i] == 0 <=> valid (Choice 1); any other status <=> Choice 0. */
int blsgpu_signcrypt_valid_batch(int sig_group, int scheme, const void* us, const void* ws, const uint8_t* vs,
                                 const uint64_t* v_offsets, size_t n, int fmt, int32_t* status) try {
  int rc = check_common(sig_group, scheme, fmt);
  if (rc) return rc;
  return core_verify_entry(sig_group, scheme_dst(sig_group, scheme), 1, us, ws, vs, v_offsets, n, fmt, status);
}
API_CATCH

// The proof-of-knowledge check of n items, shared by blsgpu_sig_proof_verify_batch (ys given, raw formats) and
// blsgpu_sig_proof_timestamp_verify_batch (stamped: the challenges are carved from the arena and derived on the device from
// (commitment, timestamp); all four point formats; the timeout rule on top).  Launch sequence of the timestamp form:
// k_decompress x 3 (wire formats only), k_proof_challenge, k_prepare_proof, k_proof_timeout, run_pairing2.
int sig_proof_entry(bool stamped, int sig_group, int scheme, const void* commitments, const void* proofs, const void* pks, const uint8_t* ys,
                    const uint64_t* timestamps, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, int fmt, uint64_t now_ms,
                    int64_t timeout_ms, int32_t* status) {
  const bool wire = stamped && (fmt == BLSGPU_FMT_COMPRESSED || fmt == BLSGPU_FMT_LEGACY);
  int rc = check_common(sig_group, scheme, wire ? BLSGPU_FMT_RAW_PROJ : fmt);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!commitments || !proofs || !pks || (stamped ? !timestamps : !ys) || !msg_offsets || !status) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  uint64_t total = 0;
  if (is_device_ptr(msg_offsets)) HIPCK(hipMemcpy(&total, msg_offsets + n, 8, hipMemcpyDeviceToHost));
  else total = msg_offsets[n];
  // a batch whose every item trips the timeout rule needs no hash and no pairing: the host reads the timestamps to know
  bool all_late = false;
  if (stamped && timeout_ms >= 0) {
    std::vector<uint64_t> ts(n);
    if (is_device_ptr(timestamps)) HIPCK(hipMemcpy(ts.data(), timestamps, 8 * n, hipMemcpyDeviceToHost));
    else memcpy(ts.data(), timestamps, 8 * n);
    all_late = true;
    for (size_t i = 0; i < n && all_late; i++) all_late = pok_timeout_status(ts[i], now_ms, timeout_ms) != 0;
  }
  const size_t pkb = pk_size(sig_group, fmt) * n, sgb = sig_size(sig_group, fmt) * n;
  const size_t pk_raw = pk_size(sig_group, BLSGPU_FMT_RAW_PROJ) * n, sig_raw = sig_size(sig_group, BLSGPU_FMT_RAW_PROJ) * n;
  size_t need = pad256(pkb) + 2 * pad256(sgb) + pad256(32 * n) + pad256(total) + pad256(8 * (n + 1)) + pad256(4 * n) +
                2 * pad256((size_t)WS_PAIRS_WORDS * 4 * n) + 4096;
  if (stamped) need += pad256(8 * n) + (wire ? pad256(pk_raw) + 2 * pad256(sig_raw) + pad256(4 * n) : 0);
  if ((rc = arena_reserve(c, need))) return rc;
  c->arena_off = 0;
  const void *d_u, *d_v, *d_pks, *d_ys = nullptr, *d_ts = nullptr, *d_msgs, *d_offs;
  if (stamped && (rc = stage_in(c, timestamps, 8 * n, &d_ts))) return rc;
  if (all_late) {
    int32_t* d_status = (int32_t*)arena_take(c, 4 * n);
    if (!d_status) return fail(BLSGPU_E_HIP, "internal: arena too small");
    KL(KID_PROOF_TIMEOUT, k_proof_timeout, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint64_t*)d_ts, now_ms, timeout_ms, (const int32_t*)nullptr, d_status);
    HIPCK(hipGetLastError());
    return status_out_and_sync(c, status, d_status, n);
  }
  if ((rc = stage_in(c, commitments, sgb, &d_u))) return rc;
  if ((rc = stage_in(c, proofs, sgb, &d_v))) return rc;
  if ((rc = stage_in(c, pks, pkb, &d_pks))) return rc;
  if (!stamped && (rc = stage_in(c, ys, 32 * n, &d_ys))) return rc;
  if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
  if ((rc = stage_in(c, msg_offsets, 8 * (n + 1), &d_offs))) return rc;
  Carver mem{c};
  int32_t* d_status = mem.take<int32_t>(4 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIRS_WORDS * 4 * n);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n);
  uint8_t* d_y = stamped ? mem.take<uint8_t>(32 * n) : nullptr;
  int32_t* d_dec = wire ? mem.take<int32_t>(4 * n) : nullptr;
  uint8_t* d_u_raw = wire ? mem.take<uint8_t>(sig_raw) : nullptr;
  uint8_t* d_v_raw = wire ? mem.take<uint8_t>(sig_raw) : nullptr;
  uint8_t* d_pk_raw = wire ? mem.take<uint8_t>(pk_raw) : nullptr;
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  int kfmt = fmt;
  if (wire) {
    // ProofOfKnowledgeTimestamp's points from their wire bytes, checked (subgroup test included): the first failure of
    // commitment, proof, key is the item's decode status; a point that was not decoded stays the identity
    const int legacy = fmt == BLSGPU_FMT_LEGACY;
    HIPCK(hipMemsetAsync(d_v_raw, 0, sig_raw, c->stream));
    HIPCK(hipMemsetAsync(d_pk_raw, 0, pk_raw, c->stream));
    with_group(sig_group, [&](auto G) {
      KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_u, legacy, d_u_raw, d_dec, 0);
      KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_v, legacy, d_v_raw, d_dec, 1);
      KL(KID_DECOMPRESS, k_decompress<3 - G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_pks, legacy, d_pk_raw, d_dec, 1);
    });
    d_u = d_u_raw;
    d_v = d_v_raw;
    d_pks = d_pk_raw;
    kfmt = BLSGPU_FMT_RAW_PROJ;
  }
  if (stamped) {
    with_group(sig_group, [&](auto G) {
      KL(KID_PROOF_CHALLENGE, k_proof_challenge<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_u, kfmt, (const uint64_t*)d_ts, (const int32_t*)d_dec, d_y);
    });
    d_ys = d_y;
  }
  const dst_arg dst = scheme_dst(sig_group, scheme);
  with_group(sig_group, [&](auto G) {
    KL(KID_PREPARE, k_prepare_proof<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_u, (const uint8_t*)d_v, (const uint8_t*)d_pks,
       (const uint8_t*)d_ys, kfmt, (const uint8_t*)d_msgs, (const uint64_t*)d_offs, dst, d_pairs, d_status);
  });
  if (stamped && (timeout_ms >= 0 || d_dec))
    KL(KID_PROOF_TIMEOUT, k_proof_timeout, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint64_t*)d_ts, now_ms, timeout_ms, (const int32_t*)d_dec, d_status);
  if ((rc = run_pairing2(c, n, d_pairs, d_f, d_status, pairs_walked(sig_group == 1 ? 1 : 0)))) return rc;
  if ((rc = status_out_and_sync(c, status, d_status, n))) return rc;
  return 0;
}
/* ProofOfKnowledge::verify for n proofs (reference src/proof_of_knowledge.rs:132-164 -> BlsSignatureProof::verify,
 * src/traits/sig_proof.rs:102-142; verify_timestamp_proof :145-175 derives y and calls the same check): status[i] in
 * {OK, COMMITMENT_IDENTITY, PROOF_IDENTITY, PK_IDENTITY, ZERO_CHALLENGE, INVALID_SIGNATURE (= BlsError::InvalidProof)}.
 * The message is hashed as given under the scheme's DST (the reference does not prefix the key here, even for
 * MessageAugmentation). */
int blsgpu_sig_proof_verify_batch(int sig_group, int scheme, const void* commitments, const void* proofs, const void* pks,
                                  const uint8_t* ys, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, int fmt,
                                  int32_t* status) try {
  return sig_proof_entry(false, sig_group, scheme, commitments, proofs, pks, ys, nullptr, msgs, msg_offsets, n, fmt, 0, -1, status);
}
API_CATCH

/* ProofOfKnowledgeTimestamp::verify(pk, msg, timeout_ms) for n proofs (reference src/proof_of_knowledge.rs:287-326 ->
 * verify_timestamp_proof, src/traits/sig_proof.rs:145-166): the timeout rule first (:154-161; the library reads no clock, now_ms
 * is the caller's; timeout_ms < 0 is None), then y = compute_y(u, t) on the device (:163, k_proof_challenge) and the check of
 * blsgpu_sig_proof_verify_batch (:165).  With a timeout, t > now_ms puts BLSGPU_E_ARG into the item's slot (the reference panics). */
int blsgpu_sig_proof_timestamp_verify_batch(int sig_group, int scheme, const void* commitments, const void* proofs, const void* pks,
                                            const uint64_t* timestamps, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n,
                                            int fmt, uint64_t now_ms, int64_t timeout_ms, int32_t* status) try {
  return sig_proof_entry(true, sig_group, scheme, commitments, proofs, pks, nullptr, timestamps, msgs, msg_offsets, n, fmt, now_ms, timeout_ms, status);
}
API_CATCH

/* BlsSignatureProof::compute_y(u, t) for n commitments (reference src/traits/sig_proof.rs:38-46): HashToScalar over the modern
 * compressed commitment and LE64(t) under the proof salt, whatever format the point came in.  out_ys: n x 32 B little-endian
 * canonical.  A wire-format commitment that does not decode gets y = 0. */
int blsgpu_sig_proof_challenge_batch(int sig_group, const void* commitments, const uint64_t* timestamps, size_t n, int fmt, uint8_t* out_ys) try {
  const bool wire = fmt == BLSGPU_FMT_COMPRESSED || fmt == BLSGPU_FMT_LEGACY;
  int rc = check_common(sig_group, 0, wire ? BLSGPU_FMT_RAW_PROJ : fmt);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!commitments || !timestamps || !out_ys) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  const size_t sgb = sig_size(sig_group, fmt) * n, sig_raw = sig_size(sig_group, BLSGPU_FMT_RAW_PROJ) * n;
  if ((rc = arena_reserve(c, pad256(sgb) + pad256(8 * n) + pad256(32 * n) + (wire ? pad256(sig_raw) + pad256(4 * n) : 0) + 4096))) return rc;
  c->arena_off = 0;
  const void *d_u, *d_ts;
  if ((rc = stage_in(c, commitments, sgb, &d_u))) return rc;
  if ((rc = stage_in(c, timestamps, 8 * n, &d_ts))) return rc;
  Carver mem{c};
  uint8_t* d_y = mem.stage_out<uint8_t>(out_ys, 32 * n);
  int32_t* d_dec = wire ? mem.take<int32_t>(4 * n) : nullptr;
  uint8_t* d_u_raw = wire ? mem.take<uint8_t>(sig_raw) : nullptr;
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  int kfmt = fmt;
  if (wire) {
    with_group(sig_group, [&](auto G) {
      KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_u, (int)(fmt == BLSGPU_FMT_LEGACY), d_u_raw, d_dec, 0);
    });
    d_u = d_u_raw;
    kfmt = BLSGPU_FMT_RAW_PROJ;
  }
  with_group(sig_group, [&](auto G) {
    KL(KID_PROOF_CHALLENGE, k_proof_challenge<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_u, kfmt, (const uint64_t*)d_ts, (const int32_t*)d_dec, d_y);
  });
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out_ys, d_y, 32 * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* HashToScalar::hash_to_scalar(m, salt) for n inputs (reference src/impls/g1.rs:25-27, g2.rs:23-25 -> scalar_from_hkdf_bytes,
 * src/helpers.rs:9-26; ProofCommitmentChallenge::from_hash and SecretKey::from_hash with KEYGEN_SALT, proof_commitment.rs:256-261,
 * secret_key.rs:276-281).  out: n x 32 B little-endian canonical; a zero result is written as zero (hkdf.cuh).  Not constant
 * time: public inputs only. */
int blsgpu_hash_to_scalar(const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, const uint8_t* salt, size_t salt_len, uint8_t* out) try {
  if (!initialised()) return NOT_INIT();
  if (n == 0) return 0;
  if (!msg_offsets || !out || (!salt && salt_len)) return fail(BLSGPU_E_ARG, "null argument");
  if (salt_len >> 32) return fail(BLSGPU_E_ARG, "salt longer than 2^32 - 1 bytes");
  CTX_ACQUIRE(c);
  std::vector<uint64_t> offs;
  int rc = read_offsets(msg_offsets, n, "msg_offsets", offs);
  if (rc) return rc;
  const uint64_t total = offs[n];
  if (!msgs && total) return fail(BLSGPU_E_ARG, "null argument");
  for (size_t i = 0; i < n; i++)
    if ((offs[i + 1] - offs[i]) >> 29) return fail(BLSGPU_E_ARG, "message of 512 MiB or more");
  if ((rc = arena_reserve(c, pad256(total) + pad256(8 * (n + 1)) + pad256(salt_len) + pad256(32 * n) + 4096))) return rc;
  c->arena_off = 0;
  const void *d_msgs, *d_offs, *d_salt;
  if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
  if ((rc = stage_in(c, msg_offsets, 8 * (n + 1), &d_offs))) return rc;
  if ((rc = stage_in(c, salt, salt_len, &d_salt))) return rc;
  uint8_t* d_out = stage_out<uint8_t>(c, out, 32 * n);
  if (!d_out) return fail(BLSGPU_E_HIP, "internal: arena too small");
  KL(KID_HASH_TO_SCALAR, k_hash_to_scalar, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_msgs, (const uint64_t*)d_offs, (const uint8_t*)d_salt,
     (uint32_t)salt_len, d_out);
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out, d_out, 32 * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* n independent two-pair checks  e(g1a[i], g2a[i]) * e(g1b[i], g2b[i]) == 1  -- Pairing::pairing(&[(..), (..)]).is_identity()
 * per item (reference src/traits/pairings.rs:50, glue src/helpers.rs:41-63), the shape of BlsSignCrypt::verify_share
 * (src/traits/sign_crypt.rs:192-207) and the ElGamal / time-lock share checks.  is_one[i] = 1 / 0.  Points must be in the
 * prime-order subgroups (every reference type guarantees it): a pair with an identity member contributes 1. */
int blsgpu_pairing2_check_batch(const void* g1a, const void* g2a, const void* g1b, const void* g2b, size_t n, int fmt,
                                int32_t* is_one) try {
  int rc = check_common(1, 0, fmt);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!g1a || !g2a || !g1b || !g2b || !is_one) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  const size_t b1 = point_bytes(1, fmt) * n, b2 = point_bytes(2, fmt) * n;
  size_t need = 2 * pad256(b1) + 2 * pad256(b2) + pad256(4 * n) + 2 * pad256((size_t)WS_PAIRS_WORDS * 4 * n) + 4096;
  if ((rc = arena_reserve(c, need))) return rc;
  c->arena_off = 0;
  const void *d1a, *d2a, *d1b, *d2b;
  if ((rc = stage_in(c, g1a, b1, &d1a))) return rc;
  if ((rc = stage_in(c, g2a, b2, &d2a))) return rc;
  if ((rc = stage_in(c, g1b, b1, &d1b))) return rc;
  if ((rc = stage_in(c, g2b, b2, &d2b))) return rc;
  Carver mem{c};
  int32_t* d_status = mem.take<int32_t>(4 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIRS_WORDS * 4 * n);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  KL(KID_PAIRS_AFF, k_pairs2_to_affine, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d1a, (const uint8_t*)d2a, (const uint8_t*)d1b,
     (const uint8_t*)d2b, fmt, d_pairs, d_status);
  if ((rc = run_pairing2(c, n, d_pairs, d_f, d_status, pairs_walked(0)))) return rc;
  KL(KID_PAIRS_AFF, k_status_to_flag, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_status);
  if ((rc = copy_out(c, is_one, d_status, 4 * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* Pairing::pairing(&[(g1s[i], g2s[i])]) for n independent single pairs (reference src/helpers.rs:41-63), the VALUE: out_gt = n x 576
 * bytes, Gt::to_bytes() as include/blsgpu.h states the assumption.  All four point formats; a COMPRESSED / LEGACY pair that does not
 * decode gets its decode status (the G1 member's first) and 576 zero bytes; a pair with an identity member gets Gt one and BLSGPU_OK,
 * as multi_miller_loop skips it.  Launch sequence: k_decompress x 2 (wire formats only), k_pairing_value_prepare, then
 * run_pairing_values. */
const size_t PAIRING_VALUE_CHUNK = 4096;
// does a call of n items take the lane-split plan?  (BLSGPU_VALUE_SPLIT_MIN: the smallest such n, 0 = never; its callers size the
// arena by the answer -- the plan needs an Fp12 workspace of WS_F_WORDS words per item)
bool value_split_wanted(size_t n) {
  const size_t from = (size_t)knobs().value_split_min;
  return from != 0 && n >= from && miller_chunk_items() != 0;
}
// The lane-split plan of items [0, n), `chunk` items at a time (the caller has reserved the line workspace for a chunk): per chunk
// the Miller value of every PV_RUN item into the Fp12 workspace d_f (stride n) -- d_pairs != nullptr; from the set's rows
// (k_millerf_rows1) or, walked, k_linesp pass 1 on the one-pair workspace with the flags as its `bad` array and k_millerfp3 with one
// item per accumulator --, then k_finalexp2s_value with the line workspace, now consumed, as its value store (as run_pairing2).
// (k_linesp reads P at word 0 and Q at words W2, 2 W2 of its workspace: all inside WS_PAIR1_WORDS.  k_lines2s would not do: it also
// loads P1 at word 3 W2.)  k_linesp4 is not used: it pays below a machine round of lane pairs, where the one-wave plan runs anyway.
void launch_value_split(Ctx* c, size_t n, size_t chunk, const uint32_t* d_pairs, const int32_t* d_flag, uint8_t* d_out, uint32_t* d_f, const uint32_t* rows,
                        const uint32_t* d_ent) {
  for (size_t first = 0; first < n; first += chunk) {
    const size_t cnt = std::min(chunk, n - first), nlanes = lanes_for(cnt), lanes = row_stride(nlanes);
    const dim3 grid((unsigned)(nlanes / BLS_BLOCK));
    if (d_pairs && rows) {
      KL(KID_MILLERF_ROWS1, k_millerf_rows1, grid, dim3(BLS_BLOCK), n, first, cnt, d_pairs, d_flag, rows, d_ent, d_f);
    } else if (d_pairs) {
      KL(KID_LINESP, k_linesp, grid, dim3(BLS_BLOCK), cnt, cnt, n, d_pairs + first, d_flag + first, c->lines_ws, c->lines_ws, lanes, (size_t)0, cnt, 1);
      KL(KID_MILLERFP, k_millerfp3, grid, dim3(BLS_BLOCK), cnt, cnt, 1, d_flag + first, (const uint32_t*)c->lines_ws, lanes, d_f + first, n, (size_t)0);
    }
    KL(KID_FINALEXP_VALUE, k_finalexp2s_value, grid, dim3(BLS_BLOCK), n, first, cnt, (const uint32_t*)d_f, c->lines_ws, lanes, d_flag, d_out);
  }
}
size_t value_split_ws_bytes(size_t chunk, bool walked) {
  const size_t lanes = row_stride(lanes_for(chunk));
  return std::max(walked ? (size_t)MILLER_ENTRIES * LINE3_WORDS_H * 4 * lanes : (size_t)0, (size_t)FX_STORE_WORDS * 4 * lanes);
}
// The pairing-value step of the four calls: the one-pair workspace d_pairs (stride n) and the flags d_flag (PV_*) -> d_out, 576 bytes
// per item.  rows / d_ent (a Bls12381G2Impl signature set whose named entries all have rows): the G2 member of item i is entry
// d_ent[i], its rows in `rows`; null: every pair is walked.  d_f: an Fp12 workspace of n items when value_split_wanted(n), else unused.
// Below BLSGPU_VALUE_SPLIT_MIN items, or when the line workspace cannot be had (lines_reserve notes it once per process): one wave per
// item, k_pairing_value_rows / k_pairing_value over chunks of at most 4,096 items.  From it up: launch_value_split in chunks of
// miller_chunk_items().  Either plan writes the same bytes.  (Rows need the item's and the table's 32-bit offsets: a call of 2^30
// items or a table of 2^32 bytes walks on the lane-split plan.)
void run_pairing_values(Ctx* c, size_t n, const uint32_t* d_pairs, const int32_t* d_flag, uint8_t* d_out, uint32_t* d_f, const uint32_t* rows,
                        const uint32_t* d_ent, size_t table_bytes) {
  if (d_f && value_split_wanted(n)) {
    const size_t chunk = std::min(n, miller_chunk_items());
    const uint32_t* split_rows = rows && n < ((size_t)1 << 30) && table_bytes <= 0xffffffffull ? rows : nullptr;
    if (lines_reserve(c, value_split_ws_bytes(chunk, !split_rows)) == 0) {
      launch_value_split(c, n, chunk, d_pairs, d_flag, d_out, d_f, split_rows, d_ent);
      return;
    }
  }
  for (size_t first = 0; first < n; first += PAIRING_VALUE_CHUNK) {
    const size_t count = std::min(PAIRING_VALUE_CHUNK, n - first);
    if (rows) KL(KID_PAIRING_VALUE_ROWS, k_pairing_value_rows, dim3((unsigned)count), dim3(BLS_BLOCK), n, first, count, d_pairs, d_flag, rows, d_ent, d_out);
    else KL(KID_PAIRING_VALUE, k_pairing_value, dim3((unsigned)count), dim3(BLS_BLOCK), n, first, count, d_pairs, d_flag, d_out);
  }
}

/* Self-test hook of k_finalexp2s_value on caller-supplied Fp12 records (576 bytes each, the record format of
 * blsgpu_fp12_product_is_one): k_f12_import, then the kernel chunk by chunk through launch_value_split with the line workspace as the
 * value store, as the pairing-value calls run it.  chunk: items per chunk (0: the library's).  status[i] on entry is the item's flag:
 * 0 runs the chain, 1 gives Gt one, anything else 576 zero bytes; it is not written.  out_gt: n x 576 bytes. */
int blsgpu_debug_finalexp_value(const void* f12s, size_t n, size_t chunk, uint8_t* out_gt, const int32_t* status) try {
  if (!initialised()) return NOT_INIT();
  if (n == 0) return 0;
  if (!f12s || !status || !out_gt) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  int rc = arena_reserve(c, pad256(576 * n) + pad256(4 * n) + pad256((size_t)GT_BYTES * n) + pad256((size_t)WS_F_WORDS * 4 * n) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_in, *d_st;
  if ((rc = stage_in(c, f12s, 576 * n, &d_in))) return rc;
  if ((rc = stage_in(c, status, 4 * n, &d_st))) return rc;
  Carver mem{c};
  uint8_t* d_out = mem.stage_out<uint8_t>(out_gt, (size_t)GT_BYTES * n);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  KL(KID_F12_IO, k_f12_import, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_in, d_f, n);
  if (chunk == 0) chunk = miller_chunk_items() ? miller_chunk_items() : n;
  if (chunk > n) chunk = n;
  if (lines_reserve(c, value_split_ws_bytes(chunk, false))) return fail(BLSGPU_E_HIP, "no room for the value store");
  launch_value_split(c, n, chunk, nullptr, (const int32_t*)d_st, d_out, d_f, nullptr, nullptr);
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out_gt, d_out, (size_t)GT_BYTES * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

int blsgpu_pairing_batch(const void* g1s, const void* g2s, size_t n, int fmt, uint8_t* out_gt, int32_t* status) try {
  if (!initialised()) return NOT_INIT();
  if (fmt != BLSGPU_FMT_RAW_PROJ && fmt != BLSGPU_FMT_RAW_AFFINE && fmt != BLSGPU_FMT_COMPRESSED && fmt != BLSGPU_FMT_LEGACY)
    return fail(BLSGPU_E_ARG, "fmt must be one of the four BLSGPU_FMT_* point formats");
  if (n == 0) return 0;
  if (!g1s || !g2s || !out_gt || !status) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  const bool wire = fmt == BLSGPU_FMT_COMPRESSED || fmt == BLSGPU_FMT_LEGACY;
  const size_t b1 = point_bytes(1, fmt) * n, b2 = point_bytes(2, fmt) * n;
  const size_t r1 = point_bytes(1, BLSGPU_FMT_RAW_PROJ) * n, r2 = point_bytes(2, BLSGPU_FMT_RAW_PROJ) * n;
  size_t need = pad256(b1) + pad256(b2) + pad256((size_t)GT_BYTES * n) + 2 * pad256(4 * n) + pad256((size_t)WS_PAIR1_WORDS * 4 * n) + 4096;
  if (wire) need += pad256(r1) + pad256(r2);
  const bool split = value_split_wanted(n);
  if (split) need += pad256((size_t)WS_F_WORDS * 4 * n);
  int rc = arena_reserve(c, need);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d1, *d2;
  if ((rc = stage_in(c, g1s, b1, &d1))) return rc;
  if ((rc = stage_in(c, g2s, b2, &d2))) return rc;
  Carver mem{c};
  uint8_t* d_out = mem.stage_out<uint8_t>(out_gt, (size_t)GT_BYTES * n);
  int32_t* d_status = mem.stage_out<int32_t>(status, 4 * n);
  int32_t* d_flag = mem.take<int32_t>(4 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIR1_WORDS * 4 * n);
  uint8_t* d_r1 = wire ? mem.take<uint8_t>(r1) : nullptr;
  uint8_t* d_r2 = wire ? mem.take<uint8_t>(r2) : nullptr;
  uint32_t* d_f = split ? mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n) : nullptr;
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  int kfmt = fmt;
  if (wire) {
    // checked decompression (subgroup test included): the first failure of the G1 member, then of the G2 member, is the pair's status
    const int legacy = fmt == BLSGPU_FMT_LEGACY;
    KL(KID_DECOMPRESS, k_decompress<1>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d1, legacy, d_r1, d_status, 0);
    KL(KID_DECOMPRESS, k_decompress<2>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d2, legacy, d_r2, d_status, 1);
    d1 = d_r1;
    d2 = d_r2;
    kfmt = BLSGPU_FMT_RAW_PROJ;
  } else {
    HIPCK(hipMemsetAsync(d_status, 0, 4 * n, c->stream));   // BLSGPU_OK: raw points are taken as they come
  }
  KL(KID_PAIRING_VALUE_PREP, k_pairing_value_prepare, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d1, (const uint8_t*)d2, kfmt,
     wire ? (const int32_t*)d_status : (const int32_t*)nullptr, d_pairs, d_flag);
  run_pairing_values(c, n, d_pairs, d_flag, d_out, d_f, nullptr, nullptr, 0);
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out_gt, d_out, (size_t)GT_BYTES * n))) return rc;
  if ((rc = stage_back(c, status, d_status, 4 * n))) return rc;
  SYNC_FLUSH(c);
  return 0;
}
API_CATCH

/* TimeCryptCiphertext::decrypt(sig) for many ciphertexts grouped under one signature each (reference src/time_crypt_ciphertext.rs:38-50
 * -> BlsTimeCrypt::unseal, src/traits/time_crypt.rs:76-116); include/blsgpu.h has the contract.  Launch sequence: k_decompress x 2
 * (wire formats only: the u of every item, the signature of every group), k_timecrypt_prepare (statuses up to the identity checks,
 * the pair of every item that passes them), run_pairing_values (K = e(sig, u) as 576 bytes per item, in the arena: one wave per
 * item below BLSGPU_VALUE_SPLIT_MIN items, the lane-split kernels from it up), k_timecrypt_open (SHA-256, SHAKE128, the frame, the scalar and g r == u, one item per lane). */
int blsgpu_timecrypt_open_batch(int sig_group, const void* sigs, const uint8_t* sig_schemes, const uint64_t* item_offsets, size_t n_groups, const void* us,
                                const uint8_t* vs, const uint8_t* ws, const uint64_t* w_offsets, const uint8_t* ct_schemes, int fmt, uint8_t* frames,
                                uint64_t* pt_range, int32_t* status) try {
  if (!initialised()) return NOT_INIT();
  if (sig_group != 1 && sig_group != 2) return fail(BLSGPU_E_ARG, "sig_group must be 1 (Bls12381G1Impl) or 2 (Bls12381G2Impl)");
  if (fmt != BLSGPU_FMT_RAW_PROJ && fmt != BLSGPU_FMT_RAW_AFFINE && fmt != BLSGPU_FMT_COMPRESSED && fmt != BLSGPU_FMT_LEGACY)
    return fail(BLSGPU_E_ARG, "fmt must be one of the four BLSGPU_FMT_* point formats");
  if (!item_offsets) return fail(BLSGPU_E_ARG, "null item_offsets");
  CTX_ACQUIRE(c);
  std::vector<uint64_t> ioffs, woffs;
  int rc = read_offsets(item_offsets, n_groups, "item_offsets", ioffs);
  if (rc) return rc;
  const size_t n = (size_t)ioffs[n_groups];
  if (n == 0) return 0;
  if (!w_offsets) return fail(BLSGPU_E_ARG, "null w_offsets");
  if ((rc = read_offsets(w_offsets, n, "w_offsets", woffs))) return rc;
  const size_t total = (size_t)woffs[n];
  for (size_t i = 0; i < n; i++)
    if ((woffs[i + 1] - woffs[i]) >> 29) return fail(BLSGPU_E_ARG, "a w of 512 MiB or more");
  if (!sigs || !sig_schemes || !us || !vs || !ct_schemes || !pt_range || !status || (total && (!ws || !frames))) return fail(BLSGPU_E_ARG, "null argument");
  const bool wire = fmt == BLSGPU_FMT_COMPRESSED || fmt == BLSGPU_FMT_LEGACY;
  const int pkg = key_group(sig_group);
  const size_t ub = pk_size(sig_group, fmt) * n, sb = sig_size(sig_group, fmt) * n_groups;
  const size_t u_raw = pk_size(sig_group, BLSGPU_FMT_RAW_PROJ) * n, s_raw = sig_size(sig_group, BLSGPU_FMT_RAW_PROJ) * n_groups;
  size_t need = pad256(ub) + pad256(sb) + pad256(n_groups) + pad256(8 * (n_groups + 1)) + pad256(32 * n) + 2 * pad256(total) + pad256(8 * (n + 1)) + pad256(n) +
                pad256(16 * n) + 2 * pad256(4 * n) + pad256((size_t)WS_PAIR1_WORDS * 4 * n) + pad256((size_t)GT_BYTES * n) + 8192;
  if (wire) need += pad256(u_raw) + pad256(s_raw) + pad256(4 * n) + pad256(4 * n_groups);
  const bool split = value_split_wanted(n);
  if (split) need += pad256((size_t)WS_F_WORDS * 4 * n);
  if ((rc = arena_reserve(c, need))) return rc;
  c->arena_off = 0;
  const void *d_sigs, *d_ss, *d_us, *d_vs, *d_ws, *d_cs;
  const uint64_t *d_ioffs, *d_woffs;
  if ((rc = stage_in(c, sigs, sb, &d_sigs))) return rc;
  if ((rc = stage_in(c, sig_schemes, n_groups, &d_ss))) return rc;
  if ((rc = stage_in(c, us, ub, &d_us))) return rc;
  if ((rc = stage_in(c, vs, 32 * n, &d_vs))) return rc;
  if ((rc = stage_in(c, ws, total, &d_ws))) return rc;
  if ((rc = stage_in(c, ct_schemes, n, &d_cs))) return rc;
  if ((rc = upload_offsets(c, ioffs, &d_ioffs))) return rc;
  if ((rc = upload_offsets(c, woffs, &d_woffs))) return rc;
  Carver mem{c};
  uint8_t* d_frames = total ? mem.stage_out<uint8_t>(frames, total) : c->arena;
  uint64_t* d_range = mem.stage_out<uint64_t>(pt_range, 16 * n);
  int32_t* d_status = mem.take<int32_t>(4 * n);
  int32_t* d_flag = mem.take<int32_t>(4 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIR1_WORDS * 4 * n);
  uint8_t* d_gt = mem.take<uint8_t>((size_t)GT_BYTES * n);
  uint8_t* d_u_raw = wire ? mem.take<uint8_t>(u_raw) : nullptr;
  uint8_t* d_s_raw = wire ? mem.take<uint8_t>(s_raw) : nullptr;
  int32_t* d_dec_u = wire ? mem.take<int32_t>(4 * n) : nullptr;
  int32_t* d_dec_s = wire ? mem.take<int32_t>(4 * n_groups) : nullptr;
  uint32_t* d_f = split ? mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n) : nullptr;
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if (total && d_frames != frames) HIPCK(hipMemsetAsync(d_frames, 0, total, c->stream));   // an item that is not opened hands back zeros, not arena bytes
  int kfmt = fmt;
  if (wire) {
    const int legacy = fmt == BLSGPU_FMT_LEGACY;
    with_group(pkg, [&](auto G) { KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_us, legacy, d_u_raw, d_dec_u, 0); });
    with_group(sig_group, [&](auto G) {
      KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(n_groups)), dim3(BLS_BLOCK), n_groups, (const uint8_t*)d_sigs, legacy, d_s_raw, d_dec_s, 0);
    });
    d_us = d_u_raw;
    d_sigs = d_s_raw;
    kfmt = BLSGPU_FMT_RAW_PROJ;
  }
  with_group(sig_group, [&](auto G) {
    KL(KID_TIMECRYPT_PREP, k_timecrypt_prepare<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, n_groups, d_ioffs, (const uint8_t*)d_us, (const uint8_t*)d_sigs, kfmt,
       (const uint8_t*)d_ss, (const uint8_t*)d_cs, (const int32_t*)d_dec_u, (const int32_t*)d_dec_s, d_pairs, d_flag, d_status);
  });
  run_pairing_values(c, n, d_pairs, d_flag, d_gt, d_f, nullptr, nullptr, 0);
  with_group(sig_group, [&](auto G) {
    KL(KID_TIMECRYPT_OPEN, k_timecrypt_open<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_gt, (const uint8_t*)d_us, kfmt, (const uint8_t*)d_vs,
       (const uint8_t*)d_ws, d_woffs, d_frames, d_range, d_status);
  });
  HIPCK(hipGetLastError());
  if (total && (rc = stage_back(c, frames, d_frames, total))) return rc;
  if ((rc = stage_back(c, pt_range, d_range, 16 * n))) return rc;
  return status_out_and_sync(c, status, d_status, n);
}
API_CATCH

/* product of k Fp12 records (the partials of blsgpu_aggregate_partial) -> final exponentiation -> *is_one */
int blsgpu_fp12_product_is_one(const void* f12s, size_t k, int32_t* is_one) try {
  if (!initialised()) return NOT_INIT();
  if (!is_one || (k && !f12s)) return fail(BLSGPU_E_ARG, "null argument");
  int32_t verdict = BLSGPU_OK;
  if (k > 0) {
    CTX_ACQUIRE(c);
    int rc = arena_reserve(c, pad256(576 * k) + pad256((size_t)WS_F_WORDS * 4 * k) + 4096);
    if (rc) return rc;
    c->arena_off = 0;
    const void* d_in;
    if ((rc = stage_in(c, f12s, 576 * k, &d_in))) return rc;
    uint32_t* d_f = (uint32_t*)arena_take(c, (size_t)WS_F_WORDS * 4 * k);
    int32_t* d_v = (int32_t*)arena_take(c, 4);
    if (!d_f || !d_v) return fail(BLSGPU_E_HIP, "internal: arena too small");
    KL(KID_F12_IO, k_f12_import, dim3(blocks_for(k)), dim3(BLS_BLOCK), k, (const uint8_t*)d_in, d_f, k);
    if ((rc = run_f12_product_verdict(c, d_f, k, k, d_v))) return rc;
    HIPCK(hipMemcpyAsync(&verdict, d_v, 4, hipMemcpyDeviceToHost, c->stream));
    SYNC_FLUSH(c);
  }
  int32_t one = verdict == BLSGPU_OK ? 1 : 0;
  return put_i32(is_one, one);
}
API_CATCH


// ---- threshold recovery (shares.cuh): n_sets Lagrange interpolations at zero in one call
// The plan of one call, made on the host from the set sizes: sets of at least BLSGPU_SHARES_MSM_MIN shares run as one bucket MSM
// each (k_msm2_*), all others as per-share ladders and a segmented tree sum; the coefficients of a large set are split over S
// workgroups per tile range (k_share_lagrange).  ws_bytes: what run_combine_shares takes from the arena.
struct combine_plan {
  std::vector<uint32_t> hflags;
  uint64_t tmax = 0, tmax_ladder = 0, tmax_msm = 0;
  size_t S = 1, ws_bytes = 0;
};
static combine_plan combine_make_plan(const std::vector<uint64_t>& offs, size_t n_sets, int group) {
  combine_plan pl;
  const size_t n = (size_t)offs[n_sets], osz = point_bytes(group, BLSGPU_FMT_RAW_PROJ);
  const uint64_t msm_min = (uint64_t)knobs().shares_msm_min;
  pl.hflags.assign(n_sets, 0);
  for (size_t s = 0; s < n_sets; s++) {
    const uint64_t t = offs[s + 1] - offs[s];
    pl.tmax = std::max(pl.tmax, t);
    if (t >= msm_min) {
      pl.hflags[s] = SHARE_F_MSM;
      pl.tmax_msm = std::max(pl.tmax_msm, t);
    } else {
      pl.tmax_ladder = std::max(pl.tmax_ladder, t);
    }
  }
  size_t S = std::max<size_t>(1, std::min<size_t>(64, (size_t)(pl.tmax / 256)));
  pl.S = std::max<size_t>(1, std::min(S, ((size_t)1 << 22) / std::max<size_t>(n, 1)));
  const size_t msm_bytes = pl.tmax_msm ? msm_ws_bytes(pl.tmax_msm) + pad256(osz * accumulate_lanes(pl.tmax_msm)) + pad256(osz * POINT_TREE_START) : 0;
  pl.ws_bytes = pad256(32 * n) + pad256(4 * n) + pad256(64 * pl.S * n) + pad256(osz * n) + pad256(4 * n_sets) + msm_bytes + 2048;
  return pl;
}
// The device part: coefficients, ladders or MSMs, the per-set sums (Z = 1, all-zero for the identity or a failed set) into d_out and
// the per-set statuses into d_st.  Stream-ordered on the context's stream; its workspaces come from the arena.
static int run_combine_shares(Ctx* c, int group, const combine_plan& pl, const std::vector<uint64_t>& offs, size_t n_sets, const uint8_t* d_ids, const uint8_t* d_pts,
                       const uint8_t* d_sch, const uint64_t* o, int fmt, uint8_t* d_out, int32_t* d_st) {
  const size_t n = (size_t)offs[n_sets], S = pl.S;
  const size_t psz = point_bytes(group, fmt), osz = point_bytes(group, BLSGPU_FMT_RAW_PROJ);
  const uint64_t tmax_ladder = pl.tmax_ladder, tmax_msm = pl.tmax_msm;
  const std::vector<uint32_t>& hflags = pl.hflags;
  int rc = 0;
  Carver mem{c};
  uint8_t* d_lam = mem.take<uint8_t>(32 * n);
  uint32_t* d_sid = mem.take<uint32_t>(4 * n);
  uint32_t* d_nd = mem.take<uint32_t>(64 * S * n);
  uint8_t* d_part = mem.take<uint8_t>(osz * n);
  uint32_t* d_flags = mem.take<uint32_t>(4 * n_sets);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if (tmax_msm) HIPCK(hipMemcpyAsync(d_flags, hflags.data(), 4 * n_sets, hipMemcpyHostToDevice, c->stream));
  else HIPCK(hipMemsetAsync(d_flags, 0, 4 * n_sets, c->stream));
  if (n) {
    KL(KID_SHARE_LAGRANGE, k_share_lagrange, dim3(blocks_for(n), (unsigned)S), dim3(BLS_BLOCK), n, o, n_sets, d_ids, d_flags, d_nd, d_sid);
    KL(KID_SHARE_LAGRANGE, k_share_lagrange_fin, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (int)S, o, d_ids, d_sch,
       (const uint32_t*)d_nd, (const uint32_t*)d_sid, d_flags, d_lam);
    if (tmax_ladder >= 2) {
      with_group(group, [&](auto G) {
        KL(KID_SHARE_LADDER, k_share_ladder<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_pts, fmt, (const uint8_t*)d_lam,
           (const uint32_t*)d_sid, (const uint32_t*)d_flags, d_part);
      });
      for (uint64_t step = 1; step < tmax_ladder; step <<= 1) {
        with_group(group, [&](auto G) { KL(KID_SHARE_FOLD, k_share_fold<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, step, o, (const uint32_t*)d_sid, d_part); });
      }
    }
    // the large sets: one MSM each over the set's points and coefficients, its (Z = 1) result into the set's first record.  A failed
    // set computes a value nobody reads (k_share_out gives it the identity).  The MSM's workspace is reused from set to set.
    const size_t mark = c->arena_off;
    for (size_t s = 0; s < n_sets; s++) {
      if (!(hflags[s] & SHARE_F_MSM)) continue;
      const size_t lo = (size_t)offs[s], t = (size_t)(offs[s + 1] - offs[s]), T = accumulate_lanes(t);
      c->arena_off = mark;
      uint8_t* d_msm = (uint8_t*)arena_take(c, osz * T);
      if (!d_msm) return fail(BLSGPU_E_HIP, "internal: arena too small");
      const uint8_t* sp = d_pts + psz * lo;
      rc = with_group(group, [&](auto G) { return run_point_sum<G()>(c, sp, fmt, d_lam + 32 * lo, nullptr, t, d_msm, T); });
      if (rc) return rc;
      HIPCK(hipMemcpyAsync(d_part + osz * lo, d_msm, osz, hipMemcpyDeviceToDevice, c->stream));
    }
  }
  with_group(group, [&](auto G) {
    KL(KID_SHARE_OUT, k_share_out<G()>, dim3(blocks_for(n_sets)), dim3(BLS_BLOCK), n_sets, o, (const uint32_t*)d_flags, (const uint8_t*)d_part, d_out, d_st);
  });
  HIPCK(hipGetLastError());
  return 0;
}

int blsgpu_combine_shares(int group, const uint8_t* ids, const void* pts, const uint8_t* schemes, const uint64_t* set_offsets,
                          size_t n_sets, int fmt, void* out, int32_t* status) try {
  if (!initialised()) return NOT_INIT();
  if (group != 1 && group != 2) return fail(BLSGPU_E_ARG, "group must be 1 (G1) or 2 (G2)");
  if (fmt != BLSGPU_FMT_RAW_PROJ && fmt != BLSGPU_FMT_RAW_AFFINE) return fail(BLSGPU_E_ARG, "fmt must be RAW_PROJ or RAW_AFFINE");
  if (!set_offsets) return fail(BLSGPU_E_ARG, "null set_offsets");
  if (n_sets && (!out || !status)) return fail(BLSGPU_E_ARG, "null argument");
  CTX_ACQUIRE(c);
  std::vector<uint64_t> offs;
  int rc = read_offsets(set_offsets, n_sets, "set_offsets", offs);
  if (rc) return rc;
  const size_t n = (size_t)offs[n_sets];
  if (n >= ((size_t)1 << 32)) return fail(BLSGPU_E_ARG, "too many shares in one call");
  if (n && (!ids || !pts)) return fail(BLSGPU_E_ARG, "null argument");
  if (n_sets == 0) return 0;
  const combine_plan pl = combine_make_plan(offs, n_sets, group);
  const size_t psz = point_bytes(group, fmt), osz = point_bytes(group, BLSGPU_FMT_RAW_PROJ);
  rc = arena_reserve(c, pad256(psz * n) + pad256(32 * n) + pad256(n) + pad256(8 * (n_sets + 1)) + pad256(osz * n_sets) + pad256(4 * n_sets) + pl.ws_bytes + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_pts, *d_ids, *d_sch = nullptr;
  const uint64_t* d_offs;
  if ((rc = stage_in(c, pts, psz * n, &d_pts))) return rc;
  if ((rc = stage_in(c, ids, 32 * n, &d_ids))) return rc;
  if (schemes && n && (rc = stage_in(c, schemes, n, &d_sch))) return rc;
  if ((rc = upload_offsets(c, offs, &d_offs))) return rc;
  uint8_t* d_out = stage_out<uint8_t>(c, out, osz * n_sets);
  int32_t* d_st = (int32_t*)arena_take(c, 4 * n_sets);
  if (!d_out || !d_st) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if ((rc = run_combine_shares(c, group, pl, offs, n_sets, (const uint8_t*)d_ids, (const uint8_t*)d_pts, (const uint8_t*)d_sch, d_offs, fmt, d_out, d_st)))
    return rc;
  if ((rc = stage_back(c, out, d_out, osz * n_sets))) return rc;
  return status_out_and_sync(c, status, d_st, n_sets);
}
API_CATCH

// ---- threshold signcryption (signcrypt.cuh): decryption-share checks and opening with shares, many ciphertexts per call
// (blsgpu_signcrypt_share_verify_batch: below, next to its indexed twin -- signcrypt_share_verify_run)
/* BlsSignCrypt::unseal_with_shares / SignCryptCiphertext::decrypt_with_shares (reference src/traits/sign_crypt.rs:106-136,
 * src/sign_crypt_ciphertext.rs:60-72) for n_ct ciphertexts, or SignCryptDecryptionKey::decrypt (:157-163) when ids and
 * share_offsets are NULL and `shares` holds one key G per ciphertext.  Launch sequence: the validity check of
 * blsgpu_signcrypt_valid_batch (its hash of U || V runs once, inside its prepare stage), the share sum of blsgpu_combine_shares,
 * k_compress of the sums, then k_signcrypt_keystream: SHAKE128, xor, prefix parse and the status merge. */
int blsgpu_signcrypt_open_batch(int sig_group, int scheme, const void* us, const void* ws, const uint8_t* vs, const uint64_t* v_offsets, size_t n_ct,
                                const uint8_t* ids, const void* shares, const uint64_t* share_offsets, int fmt, uint8_t* frames, uint64_t* pt_range,
                                int32_t* status) try {
  int rc = check_common(sig_group, scheme, fmt);
  if (rc) return rc;
  if (!v_offsets) return fail(BLSGPU_E_ARG, "null v_offsets");
  if ((ids == nullptr) != (share_offsets == nullptr)) return fail(BLSGPU_E_ARG, "ids and share_offsets are given together (shares) or both NULL (keys)");
  const bool keys = share_offsets == nullptr;
  CTX_ACQUIRE(c);
  std::vector<uint64_t> voffs, soffs;
  if ((rc = read_offsets(v_offsets, n_ct, "v_offsets", voffs))) return rc;
  if (keys) {
    soffs.resize(n_ct + 1);
    for (size_t s = 0; s <= n_ct; s++) soffs[s] = s;
  } else if ((rc = read_offsets(share_offsets, n_ct, "share_offsets", soffs))) {
    return rc;
  }
  const size_t n = (size_t)soffs[n_ct], total = (size_t)voffs[n_ct];
  if (n >= ((size_t)1 << 32)) return fail(BLSGPU_E_ARG, "too many shares in one call");
  if (n_ct == 0) return 0;
  if (!us || !ws || !pt_range || !status || (total && (!vs || !frames)) || (n && !shares)) return fail(BLSGPU_E_ARG, "null argument");
  const int pkg = key_group(sig_group);
  const size_t K = point_bytes(pkg, BLSGPU_FMT_COMPRESSED), ub = pk_size(sig_group, fmt) * n_ct, wb = sig_size(sig_group, fmt) * n_ct,
               shb = pk_size(sig_group, fmt) * n, osz = point_bytes(pkg, BLSGPU_FMT_RAW_PROJ);
  combine_plan pl;
  if (!keys) pl = combine_make_plan(soffs, n_ct, pkg);
  if ((rc = arena_reserve(c, pad256(ub) + pad256(wb) + 2 * pad256(total) + pad256(shb) + pad256(32 * n) + 2 * pad256(8 * (n_ct + 1)) + pad256(osz * n_ct) +
                                 pad256(K * n_ct) + pad256(16 * n_ct) + 2 * pad256(4 * n_ct) + 2 * pad256((size_t)WS_PAIRS_WORDS * 4 * n_ct) + pl.ws_bytes + 8192)))
    return rc;
  c->arena_off = 0;
  const void *d_us, *d_ws, *d_vs, *d_sh, *d_ids = nullptr;
  const uint64_t *d_voffs, *d_soffs = nullptr;
  if ((rc = stage_in(c, us, ub, &d_us))) return rc;
  if ((rc = stage_in(c, ws, wb, &d_ws))) return rc;
  if ((rc = stage_in(c, vs, total, &d_vs))) return rc;
  if ((rc = stage_in(c, shares, shb, &d_sh))) return rc;
  if (!keys && (rc = stage_in(c, ids, 32 * n, &d_ids))) return rc;
  if ((rc = upload_offsets(c, voffs, &d_voffs))) return rc;
  if (!keys && (rc = upload_offsets(c, soffs, &d_soffs))) return rc;
  Carver mem{c};
  uint8_t* d_G = nullptr;
  int32_t* d_cst = nullptr;
  if (!keys) {
    d_G = mem.take<uint8_t>(osz * n_ct);
    d_cst = mem.take<int32_t>(4 * n_ct);
  }
  uint8_t* d_gb = mem.take<uint8_t>(K * n_ct);
  uint8_t* d_frames = total ? mem.stage_out<uint8_t>(frames, total) : c->arena;
  uint64_t* d_range = mem.stage_out<uint64_t>(pt_range, 16 * n_ct);
  int32_t* d_status = mem.take<int32_t>(4 * n_ct);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIRS_WORDS * 4 * n_ct);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n_ct);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  // BlsSignCrypt::valid: core_verify(pk := U, sig := W, msg := U.to_bytes() || V), the augmentation path of k_prepare
  if ((rc = run_verify_items(c, sig_group, 1, (const uint8_t*)d_us, (const uint8_t*)d_ws, fmt, (const uint8_t*)d_vs, d_voffs, 0, scheme_dst(sig_group, scheme), n_ct,
                             d_pairs, d_f, d_status)))
    return rc;
  // G = sum lambda_i share_i over all shares passed; a set the recovery rejects leaves the identity (combine().unwrap_or_default())
  const uint8_t* d_key = (const uint8_t*)d_sh;
  int key_fmt = fmt;
  if (!keys) {
    if ((rc = run_combine_shares(c, pkg, pl, soffs, n_ct, (const uint8_t*)d_ids, (const uint8_t*)d_sh, nullptr, d_soffs, fmt, d_G, d_cst))) return rc;
    d_key = d_G;
    key_fmt = BLSGPU_FMT_RAW_PROJ;
  }
  with_group(pkg, [&](auto G) { KL(KID_COMPRESS, k_compress<G()>, dim3(blocks_for(n_ct)), dim3(BLS_BLOCK), n_ct, d_key, key_fmt, 0, d_gb); });
  KL(KID_SIGNCRYPT_KEYSTREAM, k_signcrypt_keystream, dim3(blocks_for(n_ct)), dim3(BLS_BLOCK), n_ct, d_voffs, (const uint8_t*)d_vs, (const uint8_t*)d_gb, (int)K,
     d_soffs, d_frames, d_range, d_status);
  HIPCK(hipGetLastError());
  if (total && (rc = stage_back(c, frames, d_frames, total))) return rc;
  if ((rc = stage_back(c, pt_range, d_range, 16 * n_ct))) return rc;
  return status_out_and_sync(c, status, d_status, n_ct);
}
API_CATCH

// ---- ElGamal over the public-key group (elgamal.cuh): proof verification and opening with shares, many items per call
// What every call of an impl shares, made once per process: the message generator BlsElGamal::message_generator() =
// hash_to_curve(generator.to_bytes(), ENC_DST) in the key group (reference src/traits/elgamal.rs:20-23; ENC_DST src/impls/g1.rs:129,
// g2.rs:127 -- the tag names the other group than the one it hashes into, kept as the reference has it) as a Z = 1 RAW_PROJ record,
// and the transcript's state after its fixed prefix (Transcript::new, "dst", "base point").
static const uint8_t ELGAMAL_G1_GEN[48] = {0x97, 0xf1, 0xd3, 0xa7, 0x31, 0x97, 0xd7, 0x94, 0x26, 0x95, 0x63, 0x8c, 0x4f, 0xa9, 0xac, 0x0f, 0xc3, 0x68, 0x8c, 0x4f, 0x97, 0x74, 0xb9, 0x05,
                                           0xa1, 0x4e, 0x3a, 0x3f, 0x17, 0x1b, 0xac, 0x58, 0x6c, 0x55, 0xe8, 0x3f, 0xf9, 0x7a, 0x1a, 0xef, 0xfb, 0x3a, 0xf0, 0x0a, 0xdb, 0x22, 0xc6, 0xbb};
static const uint8_t ELGAMAL_G2_GEN[96] = {0x93, 0xe0, 0x2b, 0x60, 0x52, 0x71, 0x9f, 0x60, 0x7d, 0xac, 0xd3, 0xa0, 0x88, 0x27, 0x4f, 0x65, 0x59, 0x6b, 0xd0, 0xd0, 0x99, 0x20, 0xb6, 0x1a,
                                           0xb5, 0xda, 0x61, 0xbb, 0xdc, 0x7f, 0x50, 0x49, 0x33, 0x4c, 0xf1, 0x12, 0x13, 0x94, 0x5d, 0x57, 0xe5, 0xac, 0x7d, 0x05, 0x5d, 0x04, 0x2b, 0x7e,
                                           0x02, 0x4a, 0xa2, 0xb2, 0xf0, 0x8f, 0x0a, 0x91, 0x26, 0x08, 0x05, 0x27, 0x2d, 0xc5, 0x10, 0x51, 0xc6, 0xe4, 0x7a, 0xd4, 0xfa, 0x40, 0x3b, 0x02,
                                           0xb4, 0x51, 0x0b, 0x64, 0x7a, 0xe3, 0xd1, 0x77, 0x0b, 0xac, 0x03, 0x26, 0xa8, 0x05, 0xbb, 0xef, 0xd4, 0x80, 0x56, 0xc8, 0xc1, 0x21, 0xbd, 0xb8};
struct ElGamalConsts {
  bool ready = false;
  uint8_t h[288];        // the message generator, RAW_PROJ with Z = 1
  strobe128 prefix;
};
static ElGamalConsts g_elgamal[2];
static std::mutex g_elgamal_mu;
// Takes a context of its own: call it before the entry point leases one.
static int elgamal_consts(int sig_group, const ElGamalConsts** out) {
  std::lock_guard<std::mutex> lk(g_elgamal_mu);
  ElGamalConsts& e = g_elgamal[sig_group - 1];
  if (!e.ready) {
    const int pkg = key_group(sig_group);
    const uint8_t* gen = pkg == 1 ? ELGAMAL_G1_GEN : ELGAMAL_G2_GEN;
    const size_t K = point_bytes(pkg, BLSGPU_FMT_COMPRESSED), osz = point_bytes(pkg, BLSGPU_FMT_RAW_PROJ);
    const char* dst = sig_group == 1 ? "BLS_ELGAMAL_BLS12381G2_XMD:SHA-256_SSWU_RO_NUL_" : "BLS_ELGAMAL_BLS12381G1_XMD:SHA-256_SSWU_RO_NUL_";
    CTX_ACQUIRE(c);
    int rc = arena_reserve(c, pad256(K) + pad256(16) + pad256(osz) + 4096);
    if (rc) return rc;
    c->arena_off = 0;
    Carver mem{c};
    uint8_t* d_msg = mem.take<uint8_t>(K);
    uint64_t* d_offs = mem.take<uint64_t>(16);
    uint8_t* d_h = mem.take<uint8_t>(osz);
    if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
    const uint64_t offs[2] = {0, K};
    if ((rc = h2d_small(c, d_msg, gen, K)) || (rc = h2d_small(c, d_offs, offs, 16))) return rc;
    if ((rc = run_hash_group(c, pkg, 1, d_msg, d_offs, make_dst((const uint8_t*)dst, strlen(dst)), d_h))) return rc;
    with_group(pkg, [&](auto G) { KL(KID_MSM_NORM, k_normalize<G()>, dim3(1), dim3(BLS_BLOCK), d_h); });
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(e.h, d_h, osz, hipMemcpyDeviceToHost, c->stream));
    SYNC_FLUSH(c);
    elgamal_transcript_prefix(e.prefix, gen, K);
    e.ready = true;
  }
  *out = &e;
  return 0;
}

int blsgpu_elgamal_message_generator(int sig_group, int fmt_out, void* out) try {
  if (!initialised()) return NOT_INIT();
  if (sig_group != 1 && sig_group != 2) return fail(BLSGPU_E_ARG, "sig_group must be 1 (Bls12381G1Impl) or 2 (Bls12381G2Impl)");
  if (fmt_out < BLSGPU_FMT_RAW_PROJ || fmt_out > BLSGPU_FMT_LEGACY) return fail(BLSGPU_E_ARG, "unknown point format");
  if (!out) return fail(BLSGPU_E_ARG, "null argument");
  const ElGamalConsts* e;
  int rc = elgamal_consts(sig_group, &e);
  if (rc) return rc;
  const int pkg = key_group(sig_group);
  if (fmt_out == BLSGPU_FMT_COMPRESSED || fmt_out == BLSGPU_FMT_LEGACY) return blsgpu_serialize(pkg, e->h, 1, BLSGPU_FMT_RAW_PROJ, fmt_out, out, nullptr);
  // Z = 1: the affine record is the first two coordinates
  HIPCK(hipMemcpy(out, e->h, point_bytes(pkg, fmt_out), is_device_ptr(out) ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
  return 0;
}
API_CATCH

/* BlsElGamal::verify_proof (reference src/traits/elgamal.rs:177-226; ElGamalProof::verify, src/elgamal_proof.rs:74-84) for n
 * independent proofs.  Launch sequence: k_decompress per point array (wire formats only), k_elgamal_fixed (the small multiples of
 * G and H, once), k_elgamal_prep (checks, four points affine and compressed per proof), k_elgamal_ladder (2 n lanes: r1 and r2,
 * one joint windowed ladder each), k_elgamal_transcript (Merlin from the shared prefix state, the 512-bit reduction, the verdict). */
int blsgpu_elgamal_proof_verify_batch(int sig_group, const void* pks, size_t n_pks, const void* generators, const void* c1s, const void* c2s,
                                      const uint8_t* message_proofs, const uint8_t* blinder_proofs, const uint8_t* challenges, size_t n, int fmt,
                                      int32_t* status) try {
  if (!initialised()) return NOT_INIT();
  if (sig_group != 1 && sig_group != 2) return fail(BLSGPU_E_ARG, "sig_group must be 1 (Bls12381G1Impl) or 2 (Bls12381G2Impl)");
  if (fmt < BLSGPU_FMT_RAW_PROJ || fmt > BLSGPU_FMT_LEGACY) return fail(BLSGPU_E_ARG, "unknown point format");
  if (n == 0) return 0;
  if (n_pks != n && n_pks != 1) return fail(BLSGPU_E_ARG, "n_pks must be n (a key per proof) or 1 (one recipient)");
  if (n >= ((size_t)1 << 31)) return fail(BLSGPU_E_ARG, "too many proofs in one call");
  if (!pks || !c1s || !c2s || !message_proofs || !blinder_proofs || !challenges || !status) return fail(BLSGPU_E_ARG, "null argument");
  const ElGamalConsts* e;
  int rc = elgamal_consts(sig_group, &e);
  if (rc) return rc;
  CTX_ACQUIRE(c);
  const int pkg = key_group(sig_group);
  const bool wire = fmt == BLSGPU_FMT_COMPRESSED || fmt == BLSGPU_FMT_LEGACY;
  const size_t psz = point_bytes(pkg, fmt), osz = point_bytes(pkg, BLSGPU_FMT_RAW_PROJ), K = point_bytes(pkg, BLSGPU_FMT_COMPRESSED);
  const size_t n_gens = generators ? n : 0, fixed_bytes = 2 * ELGAMAL_TAB * 2 * 48 * (size_t)pkg;
  if ((rc = arena_reserve(c, pad256(psz * n_pks) + pad256(psz * n_gens) + 2 * pad256(psz * n) + 3 * pad256(32 * n) + pad256(osz) + pad256(fixed_bytes) +
                                 pad256(4 * osz * n) + pad256(4 * K * n) + pad256(2 * osz * n) + 2 * pad256(4 * n) + 256 +
                                 (wire ? pad256(osz * n_pks) + pad256(osz * n_gens) + 2 * pad256(osz * n) : 0) + 8192)))
    return rc;
  c->arena_off = 0;
  const void *d_pks, *d_gens = nullptr, *d_c1, *d_c2, *d_mp, *d_bp, *d_ch;
  if ((rc = stage_in(c, pks, psz * n_pks, &d_pks))) return rc;
  if (generators && (rc = stage_in(c, generators, psz * n, &d_gens))) return rc;
  if ((rc = stage_in(c, c1s, psz * n, &d_c1))) return rc;
  if ((rc = stage_in(c, c2s, psz * n, &d_c2))) return rc;
  if ((rc = stage_in(c, message_proofs, 32 * n, &d_mp))) return rc;
  if ((rc = stage_in(c, blinder_proofs, 32 * n, &d_bp))) return rc;
  if ((rc = stage_in(c, challenges, 32 * n, &d_ch))) return rc;
  Carver mem{c};
  uint8_t* d_h = mem.take<uint8_t>(osz);
  uint32_t* d_fixed = mem.take<uint32_t>(fixed_bytes);
  uint8_t* d_aff = mem.take<uint8_t>(4 * osz * n);
  uint8_t* d_comp = mem.take<uint8_t>(4 * K * n);
  uint8_t* d_rj = mem.take<uint8_t>(2 * osz * n);
  int32_t* d_status = mem.take<int32_t>(4 * n);
  int32_t *d_dec = nullptr, *d_dec_pk = nullptr;
  int pfmt = fmt;
  if (wire) {      // wire bytes -> RAW_PROJ with the checks of from_compressed; the first failure of a proof's points is its verdict
    d_dec = mem.take<int32_t>(4 * n);
    if (n_pks == 1) d_dec_pk = mem.take<int32_t>(4);
    uint8_t* p_pk = mem.take<uint8_t>(osz * n_pks);
    uint8_t* p_gen = generators ? mem.take<uint8_t>(osz * n) : nullptr;
    uint8_t* p_c1 = mem.take<uint8_t>(osz * n);
    uint8_t* p_c2 = mem.take<uint8_t>(osz * n);
    if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
    const int legacy = fmt == BLSGPU_FMT_LEGACY;
    HIPCK(hipMemsetAsync(d_dec, 0, 4 * n, c->stream));
    if (d_dec_pk) HIPCK(hipMemsetAsync(d_dec_pk, 0, 4, c->stream));
    with_group(pkg, [&](auto G) {
      KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(n_pks)), dim3(BLS_BLOCK), n_pks, (const uint8_t*)d_pks, legacy, p_pk, d_dec_pk ? d_dec_pk : d_dec, 1);
      if (p_gen) KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_gens, legacy, p_gen, d_dec, 1);
      KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_c1, legacy, p_c1, d_dec, 1);
      KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_c2, legacy, p_c2, d_dec, 1);
    });
    d_pks = p_pk;
    d_gens = p_gen;
    d_c1 = p_c1;
    d_c2 = p_c2;
    pfmt = BLSGPU_FMT_RAW_PROJ;
  }
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if ((rc = h2d_small(c, d_h, e->h, osz))) return rc;
  const strobe128 prefix = e->prefix;
  with_group(pkg, [&](auto G) {
    KL(KID_ELGAMAL_PREP, k_elgamal_fixed<G()>, dim3(1), dim3(BLS_BLOCK), (const uint8_t*)d_h, d_fixed);
    KL(KID_ELGAMAL_PREP, k_elgamal_prep<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_pks, n_pks, (const uint8_t*)d_gens, (const uint8_t*)d_h,
       (const uint8_t*)d_c1, (const uint8_t*)d_c2, pfmt, (const uint8_t*)d_mp, (const uint8_t*)d_bp, (const uint8_t*)d_ch, (const int32_t*)d_dec,
       (const int32_t*)d_dec_pk, d_aff, d_comp, d_status);
    KL(KID_ELGAMAL_LADDER, k_elgamal_ladder<G()>, dim3(blocks_for(2 * n)), dim3(BLS_BLOCK), n, generators ? 1 : 0, (const uint8_t*)d_aff, (const uint32_t*)d_fixed,
       (const uint8_t*)d_mp, (const uint8_t*)d_bp, (const uint8_t*)d_ch, (const int32_t*)d_status, d_rj);
    KL(KID_ELGAMAL_TRANSCRIPT, k_elgamal_transcript<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, prefix, (const uint8_t*)d_comp, (const uint8_t*)d_rj,
       (const uint8_t*)d_ch, d_status);
  });
  HIPCK(hipGetLastError());
  return status_out_and_sync(c, status, d_status, n);
}
API_CATCH

/* ElGamalDecryptionKey::from_shares + decrypt (reference src/elgamal_decryption_share.rs:76-90) for n_ct ciphertexts: the key of
 * set s by the stages of blsgpu_combine_shares in the key group, then out[s] = c2[s] - key; or the plain decrypt when ids and
 * share_offsets are NULL and `shares` holds one ready key per ciphertext. */
int blsgpu_elgamal_open_batch(int sig_group, const void* c2s, const uint8_t* ids, const void* shares, const uint64_t* share_offsets, size_t n_ct, int fmt,
                              void* out, int32_t* status) try {
  int rc = check_common(sig_group, 0, fmt);
  if (rc) return rc;
  if ((ids == nullptr) != (share_offsets == nullptr)) return fail(BLSGPU_E_ARG, "ids and share_offsets are given together (shares) or both NULL (keys)");
  const bool keys = share_offsets == nullptr;
  CTX_ACQUIRE(c);
  std::vector<uint64_t> soffs;
  if (keys) {
    soffs.resize(n_ct + 1);
    for (size_t s = 0; s <= n_ct; s++) soffs[s] = s;
  } else if ((rc = read_offsets(share_offsets, n_ct, "share_offsets", soffs))) {
    return rc;
  }
  const size_t n = (size_t)soffs[n_ct];
  if (n >= ((size_t)1 << 32)) return fail(BLSGPU_E_ARG, "too many shares in one call");
  if (n_ct == 0) return 0;
  if (!c2s || !out || !status || (n && !shares)) return fail(BLSGPU_E_ARG, "null argument");
  const int pkg = key_group(sig_group);
  const size_t psz = point_bytes(pkg, fmt), osz = point_bytes(pkg, BLSGPU_FMT_RAW_PROJ);
  combine_plan pl;
  if (!keys) pl = combine_make_plan(soffs, n_ct, pkg);
  if ((rc = arena_reserve(c, pad256(psz * n_ct) + pad256(psz * n) + pad256(32 * n) + pad256(8 * (n_ct + 1)) + 2 * pad256(osz * n_ct) + 2 * pad256(4 * n_ct) +
                                 pl.ws_bytes + 8192)))
    return rc;
  c->arena_off = 0;
  const void *d_c2, *d_sh, *d_ids = nullptr;
  const uint64_t* d_soffs = nullptr;
  if ((rc = stage_in(c, c2s, psz * n_ct, &d_c2))) return rc;
  if ((rc = stage_in(c, shares, psz * n, &d_sh))) return rc;
  if (!keys && (rc = stage_in(c, ids, 32 * n, &d_ids))) return rc;
  if (!keys && (rc = upload_offsets(c, soffs, &d_soffs))) return rc;
  Carver mem{c};
  uint8_t* d_out = mem.stage_out<uint8_t>(out, osz * n_ct);
  int32_t* d_status = mem.take<int32_t>(4 * n_ct);
  uint8_t* d_key = nullptr;
  int32_t* d_cst = nullptr;
  if (!keys) {
    d_key = mem.take<uint8_t>(osz * n_ct);
    d_cst = mem.take<int32_t>(4 * n_ct);
  }
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if (!keys && (rc = run_combine_shares(c, pkg, pl, soffs, n_ct, (const uint8_t*)d_ids, (const uint8_t*)d_sh, nullptr, d_soffs, fmt, d_key, d_cst))) return rc;
  with_group(pkg, [&](auto G) {
    KL(KID_ELGAMAL_SUB, k_elgamal_sub<G()>, dim3(blocks_for(n_ct)), dim3(BLS_BLOCK), n_ct, (const uint8_t*)d_c2, fmt, keys ? (const uint8_t*)d_sh : (const uint8_t*)d_key,
       keys ? fmt : BLSGPU_FMT_RAW_PROJ, (const int32_t*)d_cst, d_out, d_status);
  });
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out, d_out, osz * n_ct))) return rc;
  return status_out_and_sync(c, status, d_status, n_ct);
}
API_CATCH

// ---- summed key -> verification tail, the last stage of the batched verify_secure and multi verify.  Its buffers are carved where the
// entry point lists its own (before any workspace that is reused from set to set); run_set_tail writes every set's signature as RAW_PROJ,
// its key part[part_offs[s]] and its status so far (k_set_out, under the caller's kernel id), then runs ONE core_verify tail over all sets.
struct set_tail {
  int32_t* st;
  uint8_t *sigp, *apk;
  uint32_t *pairs, *f;
  set_tail(Carver& mem, size_t n_sets)
      : st(mem.take<int32_t>(4 * n_sets)), sigp(mem.take<uint8_t>(288 * n_sets)), apk(mem.take<uint8_t>(288 * n_sets)),
        pairs(mem.take<uint32_t>((size_t)WS_PAIRS_WORDS * 4 * n_sets)), f(mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n_sets)) {}
};
static int run_set_tail(Ctx* c, const set_tail& t, int sig_group, int scheme, int aug, int kid, size_t n_sets, const uint64_t* d_key_offs,
                        const uint64_t* d_part_offs, uint32_t* d_flags, const uint8_t* d_part, const void* d_sigs, int fmt, const void* d_msgs, const void* d_moffs) {
  with_group(sig_group, [&](auto G) {
    KL(kid, k_set_out<G()>, dim3(blocks_for(n_sets)), dim3(BLS_BLOCK), n_sets, d_key_offs, d_part_offs, d_flags, d_part, (const uint8_t*)d_sigs, fmt, t.sigp,
       t.apk, t.st);
  });
  return run_verify_items(c, sig_group, aug, t.apk, t.sigp, BLSGPU_FMT_RAW_PROJ, (const uint8_t*)d_msgs, (const uint64_t*)d_moffs, 0,
                          scheme_dst(sig_group, scheme), n_sets, t.pairs, t.f, t.st, 1);
}

// ---- the ragged arguments of the batched secure / multi verify and of the batched sums, checked and read.  `keys` stands for the
// keys in the null check: the caller's array, or its positions in a key set (indexed_begin)
struct set_args {
  std::vector<uint64_t> offs, moffs;
  size_t n = 0;
};
static int set_args_read(set_args& a, const void* keys, const uint64_t* key_offsets, size_t n_sets, const void* sigs, const uint8_t* msgs,
                         const uint64_t* msg_offsets, const int32_t* status) {
  int rc;
  if (!key_offsets) return fail(BLSGPU_E_ARG, "null key_offsets");
  if (n_sets && (!sigs || !msg_offsets || !status)) return fail(BLSGPU_E_ARG, "null argument");
  if ((rc = read_offsets(key_offsets, n_sets, "key_offsets", a.offs))) return rc;
  a.n = (size_t)a.offs[n_sets];
  if (a.n >= ((size_t)1 << 32)) return fail(BLSGPU_E_ARG, "2^32 or more keys in one call");
  if (a.n && !keys) return fail(BLSGPU_E_ARG, "null argument");
  if (n_sets == 0) return 0;
  if ((rc = read_offsets(msg_offsets, n_sets, "msg_offsets", a.moffs, false))) return rc;      // set s's message is msgs + moffs[s]
  if (a.moffs[n_sets] && !msgs) return fail(BLSGPU_E_ARG, "null argument");
  return 0;
}
static int sum_args_read(std::vector<uint64_t>& offs, const void* pts, const uint64_t* offsets, size_t n_sets, const void* out) {
  if (!offsets) return fail(BLSGPU_E_ARG, "null offsets");
  if (n_sets && !out) return fail(BLSGPU_E_ARG, "null argument");
  int rc = read_offsets(offsets, n_sets, "offsets", offs);
  if (rc) return rc;
  if (offs[n_sets] >= ((uint64_t)1 << 32)) return fail(BLSGPU_E_ARG, "2^32 or more points in one call");
  return offs[n_sets] && !pts ? fail(BLSGPU_E_ARG, "null argument") : 0;
}

// ---- the secure batch calls (secure.cuh).  Their plan: a set of at least BLSGPU_SECURE_BATCH_MAX keys (SECURE_F_LARGE in its flags)
// runs one at a time through the machinery of the single call, all others together through the segmented kernels; S is the second
// grid dimension of the rank kernels.
struct secure_plan {
  std::vector<uint32_t> hflags;
  uint64_t tmax_small = 0, tmax_large = 0;
  size_t S;
  secure_plan(const std::vector<uint64_t>& offs, size_t n_sets, uint64_t max_small) : hflags(n_sets, 0) {
    for (size_t s = 0; s < n_sets; s++) {
      const uint64_t t = offs[s + 1] - offs[s];
      if (t >= max_small) {
        hflags[s] = SECURE_F_LARGE;
        tmax_large = std::max(tmax_large, t);
      } else {
        tmax_small = std::max(tmax_small, t);
      }
    }
    S = std::max<size_t>(1, std::min<size_t>(64, (size_t)(tmax_small / 256)));
  }
};
// The buffers of the coefficient pipeline, carved as set_tail is: per key its serialised bytes, their sorted copy, coefficient, rank,
// set id and product (osz bytes: a key or a signature as RAW_PROJ); per set its digest and flags.
struct secure_bufs {
  uint8_t *bytes, *sorted, *scal;
  uint32_t *rank, *sid;
  uint8_t *part, *H;
  uint32_t* flags;
  secure_bufs(Carver& mem, size_t n, size_t n_sets, size_t width, size_t osz)
      : bytes(mem.take<uint8_t>(width * n)), sorted(mem.take<uint8_t>(width * n)), scal(mem.take<uint8_t>(32 * n)), rank(mem.take<uint32_t>(4 * n)),
        sid(mem.take<uint32_t>(4 * n)), part(mem.take<uint8_t>(osz * n)), H(mem.take<uint8_t>(32 * n_sets)), flags(mem.take<uint32_t>(4 * n_sets)) {}
};
// the small sets' coefficients from b.bytes: every key's rank within its set, the sorted stream, its digest per set, the scalars
static int run_secure_coefficients(Ctx* c, const secure_plan& p, const secure_bufs& b, size_t n, const uint64_t* o, size_t n_sets, size_t width) {
  HIPCK(hipMemsetAsync(b.rank, 0, 4 * n, c->stream));
  const dim3 grid(blocks_for(n), (unsigned)p.S);
  const uint32_t *flags = b.flags, *rank = b.rank, *sid = b.sid;
  if (width == 96) KL(KID_SECURE_RANK, k_secure_rank<24>, grid, dim3(BLS_BLOCK), n, o, n_sets, (const uint8_t*)b.bytes, flags, b.rank, b.sid);
  else KL(KID_SECURE_RANK, k_secure_rank<12>, grid, dim3(BLS_BLOCK), n, o, n_sets, (const uint8_t*)b.bytes, flags, b.rank, b.sid);
  KL(KID_SECURE_GATHER, k_secure_gather, dim3(blocks_for(n * (width / 4))), dim3(BLS_BLOCK), n, width, o, (const uint8_t*)b.bytes, rank, sid, flags, b.sorted);
  KL(KID_SECURE_DIGEST, k_secure_digest, dim3((unsigned)n_sets), dim3(BLS_BLOCK), n_sets, width, o, (const uint8_t*)b.sorted, flags, b.H);
  KL(KID_SECURE_COEFF, k_secure_coeff, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, rank, sid, (const uint8_t*)b.H, b.flags, b.scal);
  return 0;
}

// ---- The batched secure verify, multi verify and plain sums after their argument checks: each body serves the entry point with keys
// by value and its twin with keys named in a registered key set.  The keys (for the sums: points) come from `keys`, which is
// keys_by_value or keys_indexed:
//   keys.arena_bytes(n_sets, large)      what stage() takes from the arena; large: some secure set runs one at a time
//   keys.stage(c, o, n_sets, large)      after the arena is reserved and the key offsets are uploaded (o): the caller's keys on the
//                                        device, or its positions and k_keyset_check of them into d_cidx and d_pre
//   keys.key_bytes(c, n, d_bytes)        secure: PublicKey::to_bytes / to_bytes_with_mode of every key (reference
//                                        src/secure_aggregation.rs:42,47,272-275)
//   keys.mul_small(c, n, scal, sid, flags, part)    secure: part[i] = scal[i] * key i for the keys of the small sets
//   keys.large_keys(c, n, &kfmt)         secure: the n keys as a DEVICE buffer in kfmt, for run_point_sum over a large set
//   keys.accumulate(c, Q, o, so, sid, part)         multi, sums: the strip sums
//   keys.fin(c, n_sets, d_status)        after the last kernel, before the statuses leave the device
//   keys.done()                          sums (no status vector): after the call's synchronisation, its return code
extern "C++" {
// batched verify_secure: n_sets independent Signature::verify_secure checks in one call.  a: the checked key and message offsets;
// every other pointer as the caller gave it (host or device).
template <class Keys>
static int verify_secure_batch_run(Ctx* c, int sig_group, int scheme, const Keys& keys, const set_args& a, size_t n_sets, const void* sigs, const uint8_t* msgs,
                                   const uint64_t* msg_offsets, int fmt, int32_t* status) {
  int rc;
  const int pk_group = key_group(sig_group);
  const size_t n = a.n, ssz = sig_size(sig_group, fmt), width = pk_size(sig_group, BLSGPU_FMT_COMPRESSED), osz = pk_size(sig_group, BLSGPU_FMT_RAW_PROJ);
  const secure_plan plan(a.offs, n_sets, (uint64_t)knobs().secure_batch_max);
  const uint64_t tmax_large = plan.tmax_large;
  const size_t mtotal = (size_t)a.moffs[n_sets];
  const size_t large_bytes = tmax_large ? keysort_ws_bytes(tmax_large, width) + msm_ws_bytes(tmax_large) + pad256(osz * accumulate_lanes(tmax_large)) +
                                              pad256(osz * POINT_TREE_START) + 4096
                                        : 0;
  rc = arena_reserve(c, keys.arena_bytes(n_sets, tmax_large != 0) + 2 * pad256(width * n) + pad256(32 * n) + 2 * pad256(4 * n) + pad256(osz * n) +
                            pad256(ssz * n_sets) + pad256(mtotal) + 2 * pad256(8 * (n_sets + 1)) + pad256(32 * n_sets) + 2 * pad256(4 * n_sets) +
                            2 * pad256(288 * n_sets) + pad256((size_t)WS_PAIRS_WORDS * 4 * n_sets) + pad256((size_t)WS_F_WORDS * 4 * n_sets) + large_bytes + 16384);
  if (rc) return rc;
  c->arena_off = 0;
  const uint64_t* o;
  if ((rc = upload_offsets(c, a.offs, &o)) || (rc = keys.stage(c, o, n_sets, tmax_large != 0))) return rc;
  const void *d_sigs, *d_msgs, *d_moffs;
  if ((rc = stage_in(c, sigs, ssz * n_sets, &d_sigs))) return rc;
  if ((rc = stage_in(c, msgs, mtotal, &d_msgs))) return rc;
  if ((rc = stage_in(c, msg_offsets, 8 * (n_sets + 1), &d_moffs))) return rc;
  Carver mem{c};
  const secure_bufs b(mem, n, n_sets, width, osz);
  const set_tail tail(mem, n_sets);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  HIPCK(hipMemcpyAsync(b.flags, plan.hflags.data(), 4 * n_sets, hipMemcpyHostToDevice, c->stream));
  if (n) {
    keys.key_bytes(c, n, b.bytes);
    if (plan.tmax_small) {
      if ((rc = run_secure_coefficients(c, plan, b, n, o, n_sets, width))) return rc;
      // aggregated_pk = sum t_i pk_i per set (reference :201-204): one multiplication per key, then a segmented tree sum
      keys.mul_small(c, n, b.scal, b.sid, b.flags, b.part);
      for (uint64_t step = 1; step < plan.tmax_small; step <<= 1) {
        with_group(pk_group, [&](auto G) { KL(KID_SHARE_FOLD, k_share_fold<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, step, o, (const uint32_t*)b.sid, b.part); });
      }
    }
    // the large sets, one at a time as blsgpu_verify_secure runs them: device sort, host SHA-256 of the sorted stream, the
    // coefficients, one MSM; its result goes to the set's first record (after the fold, which left the identity there).  The
    // workspace is reused from set to set.
    int kfmt = fmt;
    const uint8_t* kp = tmax_large ? keys.large_keys(c, n, &kfmt) : nullptr;
    const size_t ksz = pk_size(sig_group, kfmt), mark = c->arena_off;
    for (size_t s = 0; s < n_sets; s++) {
      if (!(plan.hflags[s] & SECURE_F_LARGE)) continue;
      const size_t lo = (size_t)a.offs[s], t = (size_t)(a.offs[s + 1] - a.offs[s]), T = accumulate_lanes(t);
      c->arena_off = mark;
      keysort_ws w;
      if ((rc = keysort_ws_take(c, t, width, w))) return rc;
      uint8_t* d_msm = (uint8_t*)arena_take(c, osz * T);
      if (!d_msm) return fail(BLSGPU_E_HIP, "internal: arena too small");
      if ((rc = run_key_sort_to_host(c, b.bytes + width * lo, t, width, w, nullptr, nullptr))) return rc;
      uint8_t H[32];
      keys_digest_host(c->hpin, width * t, H);
      HIPCK(hipMemcpy(b.H + 32 * s, H, 32, hipMemcpyHostToDevice));       // the stream is idle here (the sort synchronised)
      if ((rc = run_coefficients(c, b.H + 32 * s, w.perm_a, t, 0, t, 0, b.scal + 32 * lo, (int32_t*)(b.flags + s)))) return rc;
      rc = with_group(pk_group, [&](auto G) { return run_point_sum<G()>(c, kp + ksz * lo, kfmt, b.scal + 32 * lo, nullptr, t, d_msm, T); });
      if (rc) return rc;
      HIPCK(hipMemcpyAsync(b.part + osz * lo, d_msm, osz, hipMemcpyDeviceToDevice, c->stream));
    }
    c->arena_off = mark;
  }
  // the tail: core_verify with the scheme's DST and no key prefix (reference :236-246); a set's key sum lies at its first key's record
  if ((rc = run_set_tail(c, tail, sig_group, scheme, 0, KID_SECURE_OUT, n_sets, o, o, b.flags, b.part, d_sigs, fmt, d_msgs, d_moffs))) return rc;
  KL(KID_SECURE_FIN, k_secure_fin, dim3(blocks_for(n_sets)), dim3(BLS_BLOCK), n_sets, o, (const uint32_t*)b.flags, tail.st);
  keys.fin(c, n_sets, tail.st);
  HIPCK(hipGetLastError());
  return status_out_and_sync(c, status, tail.st, n_sets);
}

// The segmented strip sum (multi_batch.cuh) of the batched multi verify and plain sums: every set's points in strips, one strip sum
// per lane (lane pair in G2) -- the serial `g += key` of reference src/traits/pk_multi.rs:7-13, src/multi_signature.rs:87-100 and
// src/aggregate_signature.rs:130-141 -- then a segmented pairwise tree over every set's strips under the caller's fold id.  Set s's
// sum lies at its first strip's record, d_part[so[s]].  The constructor plans; begin() uploads both offset arrays and carves.
struct strip_sum {
  std::vector<uint64_t> soffs;
  std::vector<uint32_t> ssid;
  uint64_t qmax;
  size_t Q;
  const uint64_t *o = nullptr, *so = nullptr;
  uint32_t* d_ssid = nullptr;
  uint8_t* d_part = nullptr;
  strip_sum(const std::vector<uint64_t>& offs, size_t n_sets) {
    const uint64_t n = offs[n_sets];
    qmax = multi_strip_plan(offs.data(), n_sets, multi_strip_len(n, accumulate_lanes(n), (uint64_t)knobs().multi_strip), soffs, ssid);
    Q = ssid.size();
  }
  int begin(Ctx* c, const std::vector<uint64_t>& offs, size_t osz) {
    int rc;
    if ((rc = upload_offsets(c, offs, &o)) || (rc = upload_offsets(c, soffs, &so))) return rc;
    Carver mem{c};
    d_ssid = mem.take<uint32_t>(4 * Q);
    d_part = mem.take<uint8_t>(osz * Q);
    return mem.ok ? 0 : fail(BLSGPU_E_HIP, "internal: arena too small");
  }
  template <class Keys>
  int run(Ctx* c, int group, const Keys& keys, int fold_kid) const {
    if (!Q) return 0;
    HIPCK(hipMemcpyAsync(d_ssid, ssid.data(), 4 * Q, hipMemcpyHostToDevice, c->stream));
    const uint32_t* sid = d_ssid;
    keys.accumulate(c, Q, o, so, sid, d_part);
    for (uint64_t step = 1; step < qmax; step <<= 1)
      with_group(group, [&](auto G) { KL(fold_kid, k_share_fold<G()>, dim3(blocks_for(Q)), dim3(BLS_BLOCK), Q, step, so, sid, d_part); });
    return 0;
  }
};

// batched multi verify (multi_batch.cuh): n_sets independent MultiSignature::verify checks in one call
template <class Keys>
static int multi_verify_batch_run(Ctx* c, int sig_group, int scheme, const Keys& keys, const set_args& a, size_t n_sets, const void* sigs, const uint8_t* msgs,
                                  const uint64_t* msg_offsets, int fmt, int32_t* status) {
  int rc;
  strip_sum strips(a.offs, n_sets);
  const size_t ssz = sig_size(sig_group, fmt), osz = pk_size(sig_group, BLSGPU_FMT_RAW_PROJ), mtotal = (size_t)a.moffs[n_sets], Q = strips.Q;
  rc = arena_reserve(c, keys.arena_bytes(n_sets, false) + pad256(ssz * n_sets) + pad256(mtotal) + 3 * pad256(8 * (n_sets + 1)) + pad256(4 * Q) + pad256(osz * Q) +
                            2 * pad256(288 * n_sets) + pad256(4 * n_sets) + pad256((size_t)WS_PAIRS_WORDS * 4 * n_sets) +
                            pad256((size_t)WS_F_WORDS * 4 * n_sets) + 16384);
  if (rc) return rc;
  c->arena_off = 0;
  if ((rc = strips.begin(c, a.offs, osz)) || (rc = keys.stage(c, strips.o, n_sets, false))) return rc;
  const void *d_sigs, *d_msgs, *d_moffs;
  if ((rc = stage_in(c, sigs, ssz * n_sets, &d_sigs))) return rc;
  if ((rc = stage_in(c, msgs, mtotal, &d_msgs))) return rc;
  if ((rc = stage_in(c, msg_offsets, 8 * (n_sets + 1), &d_moffs))) return rc;
  Carver mem{c};
  const set_tail tail(mem, n_sets);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if ((rc = strips.run(c, key_group(sig_group), keys, KID_SHARE_FOLD))) return rc;
  // the tail: core_verify with the scheme's DST, under MessageAugmentation with the summed key's bytes in front of the message
  // (reference src/traits/sig_aug.rs:20-24); no set is decided before the tail
  rc = run_set_tail(c, tail, sig_group, scheme, scheme == BLSGPU_SCHEME_AUG, KID_MULTI_OUT, n_sets, strips.o, strips.so, nullptr, strips.d_part, d_sigs, fmt,
                    d_msgs, d_moffs);
  if (rc) return rc;
  keys.fin(c, n_sets, tail.st);
  HIPCK(hipGetLastError());
  return status_out_and_sync(c, status, tail.st, n_sets);
}

// batched plain sums (multi_batch.cuh): the sum of every one of n_sets ragged sets of points in one call; one set is a plan with one set
template <class Keys>
static int sum_batch_run(Ctx* c, int group, const Keys& keys, const std::vector<uint64_t>& offs, size_t n_sets, void* out) {
  int rc;
  strip_sum strips(offs, n_sets);
  const size_t osz = point_bytes(group, BLSGPU_FMT_RAW_PROJ), Q = strips.Q;
  rc = arena_reserve(c, keys.arena_bytes(n_sets, false) + 2 * pad256(8 * (n_sets + 1)) + pad256(4 * Q) + pad256(osz * Q) + pad256(osz * n_sets) + 16384);
  if (rc) return rc;
  c->arena_off = 0;
  if ((rc = strips.begin(c, offs, osz)) || (rc = keys.stage(c, strips.o, n_sets, false))) return rc;
  uint8_t* d_out = stage_out<uint8_t>(c, out, osz * n_sets);
  if (!d_out) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if ((rc = strips.run(c, group, keys, KID_SUM_FOLD))) return rc;
  with_group(group, [&](auto G) {
    KL(KID_SUM_OUT, k_set_sum_out<G()>, dim3(blocks_for(n_sets)), dim3(BLS_BLOCK), n_sets, strips.o, strips.so, (const uint32_t*)nullptr,
       (const uint8_t*)strips.d_part, d_out, (int32_t*)nullptr);
  });
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out, d_out, osz * n_sets))) return rc;
  SYNC_FLUSH(c);
  return keys.done();
}
}  // extern "C++"

// The keys of a by-value call: the caller's array of points of `group` in `fmt`, staged.  For the secure verify one joint NAF ladder
// per key of a small set; kid: the caller's profile id of the strip sums.
struct keys_by_value {
  const void* pts;
  int group, fmt, ser_format, kid;
  size_t bytes;
  mutable const void* d_pts = nullptr;
  size_t arena_bytes(size_t, bool) const { return pad256(bytes); }
  int stage(Ctx* c, const uint64_t*, size_t, bool) const { return stage_in(c, pts, bytes, &d_pts); }
  void key_bytes(Ctx* c, size_t n, uint8_t* d_bytes) const {
    with_group(group, [&](auto G) { KL(KID_COMPRESS, k_compress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_pts, fmt, ser_format, d_bytes); });
  }
  void mul_small(Ctx* c, size_t n, const uint8_t* d_scal, const uint32_t* d_sid, const uint32_t* d_flags, uint8_t* d_part) const {
    with_group(group, [&](auto G) {
      KL(KID_SHARE_LADDER, k_share_ladder<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_pts, fmt, d_scal, d_sid, d_flags, d_part);
    });
  }
  const uint8_t* large_keys(Ctx*, size_t, int* kfmt) const {
    *kfmt = fmt;
    return (const uint8_t*)d_pts;
  }
  void accumulate(Ctx* c, size_t Q, const uint64_t* o, const uint64_t* so, const uint32_t* sid, uint8_t* d_part) const {
    with_group(group, [&](auto G) {
      KL(kid, k_multi_accumulate_seg<G()>, dim3(blocks_for(G() * Q)), dim3(BLS_BLOCK), Q, (const uint8_t*)d_pts, fmt, o, so, sid, d_part);
    });
  }
  void fin(Ctx*, size_t, int32_t*) const {}
  int done() const { return 0; }
};
int blsgpu_verify_secure_batch(int sig_group, int scheme, const void* pks, const uint64_t* key_offsets, size_t n_sets, const void* sigs,
                               const uint8_t* msgs, const uint64_t* msg_offsets, int ser_format, int fmt, int32_t* status) try {
  int rc = check_common(sig_group, scheme, fmt);
  if (rc || (rc = check_ser_format(sig_group, ser_format))) return rc;
  set_args a;
  rc = set_args_read(a, pks, key_offsets, n_sets, sigs, msgs, msg_offsets, status);
  if (rc || n_sets == 0) return rc;
  // One large set alone IS blsgpu_verify_secure (on one device: no sharding).
  if (n_sets == 1 && a.n >= (uint64_t)knobs().secure_batch_max) {
    NestedScope ns;
    return blsgpu_verify_secure(sig_group, scheme, pks, a.n, sigs, msgs + a.moffs[0], (size_t)(a.moffs[1] - a.moffs[0]), ser_format, fmt, status);
  }
  CTX_ACQUIRE(c);
  const keys_by_value keys = {pks, key_group(sig_group), fmt, ser_format, 0, pk_size(sig_group, fmt) * a.n};
  return verify_secure_batch_run(c, sig_group, scheme, keys, a, n_sets, sigs, msgs, msg_offsets, fmt, status);
}
API_CATCH

// ---- batched aggregate verify (agg_batch.cuh): n_sets independent AggregateSignature::verify checks in one call
// The call after its argument checks, shared by blsgpu_aggregate_verify_batch (keys by value) and
// blsgpu_aggregate_verify_indexed_batch (keys named in a registered key set).  offs: the checked set_offsets, T pairs, `total`
// message bytes; every other pointer as the caller gave it (host or device).  The keys come from `keys`:
//   keys.arena_bytes                          what stage() takes from the arena
//   keys.stage(c, &kp, &key_table, &cidx)     after the arena is reserved: the T keys as a DEVICE buffer in the signatures' format
//                                             (kp), and optionally the rows of a key set with line tables plus the sanitised index
//                                             of every caller position -- then the batched sets' pair items take their line values
//                                             from the rows (k_linesp_keyed) and no item walks a point
//   keys.fin(c, d_status, d_aux)              after the last kernel, before the results leave the device
extern "C++" {
template <class Keys>
static int aggregate_batch_run(Ctx* c, int sig_group, int scheme, const Keys& keys, const uint8_t* msgs, const uint64_t* msg_offsets, uint64_t total,
                               const std::vector<uint64_t>& offs, size_t n_sets, const void* sigs, int fmt, int32_t* status, uint64_t* aux) {
  int rc;
  const size_t T = (size_t)offs[n_sets];
  // plan: a set of at least BLSGPU_AGG_BATCH_MAX pairs runs one at a time through the kernels of blsgpu_aggregate_verify
  // (aggregate_enqueue: its per-entry product form is what wins at tens of thousands of pairs), all others together through the
  // segmented kernels of agg_batch.cuh.
  const uint64_t max_small = (uint64_t)knobs().agg_batch_max;
  const bool basic = scheme == BLSGPU_SCHEME_BASIC;
  // the batched sets as one flat list: boffs (their item ranges), bsrc (where a set's pairs start in the caller's arrays), bset (its index)
  std::vector<uint64_t> boffs, bsrc;
  std::vector<uint32_t> bset;
  std::vector<size_t> large;
  uint64_t tmax_large = 0;
  const uint64_t tmax_b = agg_batch_plan(offs.data(), n_sets, max_small, boffs, bsrc, bset, large, &tmax_large);
  const size_t n_b = bset.size(), T_b = (size_t)boffs.back(), M = n_b ? T_b + n_b : 0;
  const size_t psz = pk_size(sig_group, fmt), ssz = sig_size(sig_group, fmt);
  size_t dup_cap = 64;
  while (dup_cap < 2 * T_b) dup_cap <<= 1;
  const bool dup_b = basic && T_b > 0;
  // Miller values in rounds of at most one machine round of lane pairs (65,536 items), all of the same size; the final
  // exponentiation in chunks of the same bound; both pass through the context's line workspace
  const size_t round = 65536, per_round = agg_round_size(M, round);
  const size_t fx_chunk = std::min(n_b, miller_chunk_items() ? miller_chunk_items() : round);
  const size_t m_large = (size_t)tmax_large + 1;
  const size_t large_bytes = large.empty() ? 0
                                           : pad256(256 * large.size()) + pad256(4 * m_large) + 2 * pad256((size_t)WS_PAIRS_WORDS * 4 * m_large) + 8192 +
                                                 (basic ? dup_ws_bytes((size_t)tmax_large) : 0);
  const size_t batch_bytes = n_b ? pad256(8 * (n_b + 1)) + pad256(8 * n_b) + pad256(4 * n_b) + pad256(4 * M) + 2 * pad256(4 * (T_b ? T_b : 1)) +
                                       pad256((size_t)WS_PAIR1_WORDS * 4 * M) + pad256((size_t)WS_F_WORDS * 4 * M) + pad256((size_t)WS_F_WORDS * 4 * n_b) +
                                       4 * pad256(4 * n_b) + (dup_b ? 2 * pad256(4 * dup_cap) + pad256(4 * T_b) : 0) + keys.flat_bytes(T_b)
                                 : 0;
  rc = arena_reserve(c, keys.arena_bytes + pad256(ssz * n_sets) + pad256(total) + pad256(8 * (T + 1)) + pad256(4 * n_sets) + pad256(16 * n_sets) + batch_bytes +
                            large_bytes + 16384);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_sigs, *d_msgs, *d_moffs;
  const uint8_t* kp = nullptr;
  const uint32_t *key_table = nullptr, *d_cidx = nullptr;
  if ((rc = keys.stage(c, &kp, &key_table, &d_cidx))) return rc;
  if ((rc = stage_in(c, sigs, ssz * n_sets, &d_sigs))) return rc;
  if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
  if ((rc = stage_in(c, msg_offsets, 8 * (T + 1), &d_moffs))) return rc;
  int32_t* d_status = stage_out<int32_t>(c, status, 4 * n_sets);
  uint64_t* d_aux = aux ? stage_out<uint64_t>(c, aux, 16 * n_sets) : nullptr;
  if (!d_status || (aux && !d_aux)) return fail(BLSGPU_E_HIP, "internal: arena too small");
  const uint8_t* sp = (const uint8_t*)d_sigs;
  const uint8_t* mp = (const uint8_t*)d_msgs;
  const uint64_t* mo = (const uint64_t*)d_moffs;
  if (n_b) {
    const uint64_t* bo;
    if ((rc = upload_offsets(c, boffs, &bo))) return rc;
    Carver mem{c};
    uint64_t* d_bsrc = mem.take<uint64_t>(8 * n_b);
    uint32_t* d_bset = mem.take<uint32_t>(4 * n_b);
    int32_t* d_bad = mem.take<int32_t>(4 * M);
    uint32_t* d_sid = mem.take<uint32_t>(4 * (T_b ? T_b : 1));
    uint32_t* d_src = mem.take<uint32_t>(4 * (T_b ? T_b : 1));
    uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIR1_WORDS * 4 * M);
    uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * M);
    uint32_t* d_rec = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n_b);
    uint32_t* d_first = mem.take<uint32_t>(4 * n_b);
    uint32_t* d_sigid = mem.take<uint32_t>(4 * n_b);
    uint32_t* d_best = mem.take<uint32_t>(4 * n_b);
    int32_t* d_stb = mem.take<int32_t>(4 * n_b);
    uint32_t *d_tab = nullptr, *d_minidx = nullptr, *d_slot = nullptr;
    if (dup_b) {
      d_tab = mem.take<uint32_t>(4 * dup_cap);
      d_minidx = mem.take<uint32_t>(4 * dup_cap);
      d_slot = mem.take<uint32_t>(4 * T_b);
    }
    uint32_t* d_key_of = key_table && T_b ? mem.take<uint32_t>(4 * T_b) : nullptr;
    if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
    const size_t lanes_round = row_stride(lanes_for(per_round)), lanes_fx = row_stride(lanes_for(fx_chunk));
    if (lines_reserve(c, std::max((size_t)MILLER_ENTRIES * LINE3_WORDS_H * 4 * lanes_round, (size_t)FX_STORE_WORDS * 4 * lanes_fx)))
      return fail(BLSGPU_E_HIP, "no room for the line workspace");
    HIPCK(hipMemcpyAsync(d_bsrc, bsrc.data(), 8 * n_b, hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemcpyAsync(d_bset, bset.data(), 4 * n_b, hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemsetAsync(d_bad, 0, 4 * M, c->stream));
    HIPCK(hipMemsetAsync(d_first, 0xff, 4 * n_b, c->stream));
    HIPCK(hipMemsetAsync(d_best, 0xff, 4 * n_b, c->stream));
    // 1. every item's hash, identity flag and affine pair (two lanes per item while that fits one machine round, as aggregate_enqueue)
    const dst_arg dst = scheme_dst(sig_group, scheme);
    const int aug = scheme == BLSGPU_SCHEME_AUG;
    const int agg_lanes_env = (int)knobs().agg_lanes;
    const int one_lane = agg_lanes_env == 1 || (agg_lanes_env != 2 && M > 65536 + 1024);
    const int agg_flags = sig_group == 1 ? (one_lane ? 2 : 3) : 1;
    with_group(sig_group, [&](auto G) {
      KL(KID_PREPARE_AGG, k_prepare_agg_seg<G()>, dim3(blocks_for((agg_flags & 1) ? 2 * M : M)), dim3(BLS_BLOCK), M, T_b, n_b, bo, (const uint64_t*)d_bsrc,
         (const uint32_t*)d_bset, kp, sp, fmt, aug, mp, mo, dst, d_pairs, d_bad, d_sid, d_src, agg_flags);
    });
    // 2. one Miller value per item (a flagged item's is 1): no partial product spans two sets because none is formed.  k_miller1s
    // multiplies items a fixed stride apart, which ragged sets cannot align with, so the remainder of a round takes the line kernels too.
    // (over a key set with line tables: every item's rows come from a table -- a pair item's from its key's, found through src)
    if (d_key_of) KL(KID_AGG_SEG_INDEX, k_agg_flat_keys, dim3(blocks_for(T_b)), dim3(BLS_BLOCK), T_b, (const uint32_t*)d_src, d_cidx, d_key_of);
    for (size_t first = 0; first < M; first += per_round) {
      const size_t cnt = std::min(per_round, M - first), nlanes = lanes_for(cnt), lanes = row_stride(nlanes);
      const dim3 grid((unsigned)(nlanes / BLS_BLOCK));
      if (key_table)
        KL(KID_LINESP_KEYED, k_linesp_keyed, grid, dim3(BLS_BLOCK), T_b, first, cnt, M, (const uint32_t*)d_pairs, (const int32_t*)d_bad, c->lines_ws, lanes, key_table,
           (const uint32_t*)d_key_of);
      else
        KL(KID_LINESP, k_linesp, grid, dim3(BLS_BLOCK), cnt, cnt, M, (const uint32_t*)(d_pairs + first), (const int32_t*)(d_bad + first), c->lines_ws, c->lines_ws,
           lanes, (size_t)0, cnt, 1);
      KL(KID_MILLERFP, k_millerfp3, grid, dim3(BLS_BLOCK), cnt, cnt, 1, (const int32_t*)(d_bad + first), (const uint32_t*)c->lines_ws, lanes, d_f + first, M, (size_t)0);
    }
    // 3. every set's product: ceil(log2(largest batched set)) halving rounds over all pair items, then times the signature's value
    for (int r = 0, nr = agg_fold_rounds(tmax_b); r < nr; r++)
      KL(KID_AGG_SEG_FOLD, k_f12_fold_seg, dim3(blocks_for(T_b)), dim3(BLS_BLOCK), T_b, r, (const uint32_t*)d_sid, bo, d_f, M);
    KL(KID_AGG_SEG_FOLD, k_f12_fold_seg_out, dim3(blocks_for(n_b)), dim3(BLS_BLOCK), n_b, T_b, bo, (const uint32_t*)d_f, M, d_rec);
    // 4., 5. the identity rules and Basic's duplicate rule, per set
    KL(KID_AGG_SEG_INDEX, k_first_bad_seg, dim3(blocks_for(M)), dim3(BLS_BLOCK), M, T_b, (const uint32_t*)d_sid, bo, (const int32_t*)d_bad, d_first, d_sigid);
    if (dup_b) {
      HIPCK(hipMemsetAsync(d_tab, 0xff, 4 * dup_cap, c->stream));
      HIPCK(hipMemsetAsync(d_minidx, 0xff, 4 * dup_cap, c->stream));
      KL(KID_AGG_SEG_INDEX, k_dup_insert_seg, dim3(blocks_for(T_b)), dim3(BLS_BLOCK), T_b, mp, mo, (const uint32_t*)d_sid, (const uint32_t*)d_src,
         (uint32_t)(dup_cap - 1), d_tab, d_minidx, d_slot);
      KL(KID_AGG_SEG_INDEX, k_dup_find_seg, dim3(blocks_for(T_b)), dim3(BLS_BLOCK), T_b, (const uint32_t*)d_sid, bo, (const uint32_t*)d_slot,
         (const uint32_t*)d_minidx, d_best);
    }
    const uint32_t* best = dup_b ? d_best : nullptr;
    // 6. one final exponentiation per set the rules left open (k_finalexp2s, the batch form, whatever the number of sets)
    KL(KID_AGG_SEG_FIN, k_agg_batch_mark, dim3(blocks_for(n_b)), dim3(BLS_BLOCK), n_b, bo, best, (const uint32_t*)d_slot, (const uint32_t*)d_minidx,
       (const uint32_t*)d_first, (const uint32_t*)d_sigid, d_stb);
    for (size_t first = 0; first < n_b; first += fx_chunk)
      launch_finalexp_chunk(c, n_b, first, std::min(fx_chunk, n_b - first), d_rec, d_stb, knobs().finalexp_seg != 0);
    // 7. the reference's precedence
    KL(KID_AGG_SEG_FIN, k_agg_batch_fin, dim3(blocks_for(n_b)), dim3(BLS_BLOCK), n_b, bo, (const uint32_t*)d_bset, best, (const uint32_t*)d_slot,
       (const uint32_t*)d_minidx, (const uint32_t*)d_first, (const uint32_t*)d_sigid, (const int32_t*)d_stb, d_status, d_aux);
    HIPCK(hipGetLastError());
  }
  if (!large.empty()) {
    // the large sets, one at a time as blsgpu_aggregate_verify runs them (the duplicate rule on the device: the messages are staged);
    // the workspace is reused from set to set, the results of each stay in a record of their own
    uint8_t* d_res = (uint8_t*)arena_take(c, 256 * large.size());
    if (!d_res) return fail(BLSGPU_E_HIP, "internal: arena too small");
    const size_t mark = c->arena_off;
    for (size_t k = 0; k < large.size(); k++) {
      const size_t s = large[k], lo = (size_t)offs[s], t = (size_t)(offs[s + 1] - offs[s]);
      c->arena_off = mark;
      int64_t* d_first1 = (int64_t*)(d_res + 256 * k);
      int32_t* d_verdict = (int32_t*)(d_res + 256 * k + 64);
      uint64_t* d_dup = (uint64_t*)(d_res + 256 * k + 128);
      if ((rc = aggregate_enqueue(c, sig_group, scheme, kp + psz * lo, sp + ssz * s, fmt, mp, mo + lo, t, d_first1, d_verdict, nullptr))) return rc;
      if (basic && (rc = run_first_duplicate(c, mp, mo + lo, t, d_dup))) return rc;
      KL(KID_AGG_SEG_FIN, k_agg_large_fin, dim3(1), dim3(BLS_BLOCK), t, (const int64_t*)d_first1, (const int32_t*)d_verdict,
         basic ? (const uint64_t*)d_dup : nullptr, d_status + s, d_aux ? d_aux + 2 * s : nullptr);
      HIPCK(hipGetLastError());
    }
  }
  if ((rc = keys.fin(c, d_status, d_aux))) return rc;
  if (aux && (rc = stage_back(c, aux, d_aux, 16 * n_sets))) return rc;
  return status_out_and_sync(c, status, d_status, n_sets);
}
}  // extern "C++"

// the keys of the by-value call: the caller's array, staged
struct agg_keys_by_value {
  const void* pks;
  size_t bytes, arena_bytes;
  size_t flat_bytes(size_t) const { return 0; }
  int stage(Ctx* c, const uint8_t** kp, const uint32_t**, const uint32_t**) const {
    const void* d_pks = nullptr;
    int rc;
    if (bytes && (rc = stage_in(c, pks, bytes, &d_pks))) return rc;
    *kp = (const uint8_t*)d_pks;
    return 0;
  }
  int fin(Ctx*, int32_t*, uint64_t*) const { return 0; }
};
int blsgpu_aggregate_verify_batch(int sig_group, int scheme, const void* pks, const uint8_t* msgs, const uint64_t* msg_offsets,
                                  const uint64_t* set_offsets, size_t n_sets, const void* sigs, int fmt, int32_t* status, uint64_t* aux) try {
  int rc = check_common(sig_group, scheme, fmt);
  if (rc) return rc;
  if (!set_offsets) return fail(BLSGPU_E_ARG, "null set_offsets");
  if (n_sets && (!sigs || !msg_offsets || !status)) return fail(BLSGPU_E_ARG, "null argument");
  std::vector<uint64_t> offs;
  if ((rc = read_offsets(set_offsets, n_sets, "set_offsets", offs))) return rc;
  const size_t T = (size_t)offs[n_sets];
  if (T >= ((size_t)1 << 32)) return fail(BLSGPU_E_ARG, "2^32 or more pairs in one call");
  if (T && !pks) return fail(BLSGPU_E_ARG, "null argument");
  if (n_sets == 0) return 0;
  // One large set alone IS blsgpu_aggregate_verify (on one device: no sharding).
  if (n_sets == 1 && T >= (uint64_t)knobs().agg_batch_max) {
    NestedScope ns;
    return blsgpu_aggregate_verify(sig_group, scheme, pks, msgs, msg_offsets, T, sigs, fmt, status, aux);
  }
  CTX_ACQUIRE(c);
  uint64_t total = 0;
  if (is_device_ptr(msg_offsets)) HIPCK(hipMemcpy(&total, msg_offsets + T, 8, hipMemcpyDeviceToHost));
  else total = msg_offsets[T];
  if (total && !msgs) return fail(BLSGPU_E_ARG, "null argument");
  const size_t psz = pk_size(sig_group, fmt);
  const agg_keys_by_value keys = {pks, psz * T, pad256(psz * T)};
  return aggregate_batch_run(c, sig_group, scheme, keys, msgs, msg_offsets, total, offs, n_sets, sigs, fmt, status, aux);
}
API_CATCH

int blsgpu_multi_verify_batch(int sig_group, int scheme, const void* pks, const uint64_t* key_offsets, size_t n_sets, const void* sigs,
                              const uint8_t* msgs, const uint64_t* msg_offsets, int fmt, int32_t* status) try {
  int rc = check_common(sig_group, scheme, fmt);
  if (rc) return rc;
  set_args a;
  rc = set_args_read(a, pks, key_offsets, n_sets, sigs, msgs, msg_offsets, status);
  if (rc || n_sets == 0) return rc;
  // one set alone IS blsgpu_multi_verify: its split over the bound devices and its cut tail serve one huge set
  if (n_sets == 1) return blsgpu_multi_verify(sig_group, scheme, pks, a.n, sigs, msgs + a.moffs[0], (size_t)(a.moffs[1] - a.moffs[0]), fmt, status);
  CTX_ACQUIRE(c);
  const keys_by_value keys = {pks, key_group(sig_group), fmt, 0, KID_MULTI_SEG_ACCUM, pk_size(sig_group, fmt) * a.n};
  return multi_verify_batch_run(c, sig_group, scheme, keys, a, n_sets, sigs, msgs, msg_offsets, fmt, status);
}
API_CATCH
// ---- batched secure aggregation (secure.cuh): n_sets independent aggregate_secure[_with_mode] sums in one call
int blsgpu_aggregate_secure_batch(int sig_group, const void* pks, const void* sigs, const uint64_t* key_offsets, size_t n_sets, int ser_format, int fmt,
                                  void* out_sigs, int32_t* status) try {
  int rc = check_common(sig_group, 0, fmt);
  if (rc) return rc;
  if ((rc = check_ser_format(sig_group, ser_format))) return rc;
  if (!key_offsets) return fail(BLSGPU_E_ARG, "null key_offsets");
  if (n_sets && (!out_sigs || !status)) return fail(BLSGPU_E_ARG, "null argument");
  std::vector<uint64_t> offs;
  if ((rc = read_offsets(key_offsets, n_sets, "key_offsets", offs))) return rc;
  const size_t n = (size_t)offs[n_sets];
  if (n >= ((size_t)1 << 32)) return fail(BLSGPU_E_ARG, "2^32 or more keys in one call");
  if (n && (!pks || !sigs)) return fail(BLSGPU_E_ARG, "null argument");
  if (n_sets == 0) return 0;
  const size_t osz = sig_size(sig_group, BLSGPU_FMT_RAW_PROJ);
  // plan (secure_plan): a large set runs through the steps of blsgpu_aggregate_secure (run_aggregate_secure_set); all others through
  // the segmented kernels of secure.cuh, one ladder per key in the signature group and a segmented tree sum.  One large set alone IS
  // blsgpu_aggregate_secure.
  const uint64_t max_small = (uint64_t)knobs().secure_batch_max;
  if (n_sets == 1 && n >= max_small) {
    if (is_device_ptr(out_sigs)) HIPCK(hipMemset(out_sigs, 0, osz));      // the single call leaves a failed set's record alone
    else memset(out_sigs, 0, osz);
    return blsgpu_aggregate_secure(sig_group, pks, sigs, n, ser_format, fmt, out_sigs, status);
  }
  CTX_ACQUIRE(c);
  const int pk_group = key_group(sig_group);
  const size_t psz = pk_size(sig_group, fmt), ssz = sig_size(sig_group, fmt), width = pk_size(sig_group, BLSGPU_FMT_COMPRESSED);
  const secure_plan plan(offs, n_sets, max_small);
  const uint64_t tmax_large = plan.tmax_large;
  const size_t large_bytes = tmax_large ? aggregate_secure_set_bytes(tmax_large, width) + pad256(osz * accumulate_lanes(tmax_large)) +
                                              pad256(osz * POINT_TREE_START) + 4096
                                        : 0;
  rc = arena_reserve(c, pad256(psz * n) + pad256(ssz * n) + pad256(8 * (n_sets + 1)) + 2 * pad256(width * n) + pad256(32 * n) + 3 * pad256(4 * n) +
                            pad256(osz * n) + pad256(32 * n_sets) + 2 * pad256(4 * n_sets) + pad256(osz * n_sets) + large_bytes + 16384);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_pks = nullptr, *d_sigs = nullptr;
  if (n && (rc = stage_in(c, pks, psz * n, &d_pks))) return rc;
  if (n && (rc = stage_in(c, sigs, ssz * n, &d_sigs))) return rc;
  const uint64_t* o;
  if ((rc = upload_offsets(c, offs, &o))) return rc;
  Carver mem{c};
  const secure_bufs b(mem, n, n_sets, width, osz);
  uint32_t* d_first = mem.take<uint32_t>(4 * n);
  int32_t* d_st = mem.take<int32_t>(4 * n_sets);
  uint8_t* d_out = mem.stage_out<uint8_t>(out_sigs, osz * n_sets);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  HIPCK(hipMemcpyAsync(b.flags, plan.hflags.data(), 4 * n_sets, hipMemcpyHostToDevice, c->stream));
  const uint8_t *kp = (const uint8_t*)d_pks, *sp = (const uint8_t*)d_sigs;
  if (n) {
    // PublicKey::to_bytes / to_bytes_with_mode of every key (reference src/secure_aggregation.rs:141,144,166,349)
    with_group(pk_group, [&](auto G) { KL(KID_COMPRESS, k_compress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, kp, fmt, ser_format, b.bytes); });
    if (plan.tmax_small) {
      if ((rc = run_secure_coefficients(c, plan, b, n, o, n_sets, width))) return rc;
      // the signature that goes with the key of a sorted position is that of the FIRST input position holding the same bytes
      // (reference :138-147): duplicates of a key all take the first copy's signature
      HIPCK(hipMemsetAsync(d_first, 0xff, 4 * n, c->stream));
      const dim3 grid(blocks_for(n), (unsigned)plan.S);
      if (width == 96)
        KL(KID_SECURE_FIRST, k_secure_first<24>, grid, dim3(BLS_BLOCK), n, o, (const uint8_t*)b.bytes, (const uint32_t*)b.sid, (const uint32_t*)b.flags, d_first);
      else
        KL(KID_SECURE_FIRST, k_secure_first<12>, grid, dim3(BLS_BLOCK), n, o, (const uint8_t*)b.bytes, (const uint32_t*)b.sid, (const uint32_t*)b.flags, d_first);
      // sum t_i sig[first_i] per set (reference :149-153): one joint NAF ladder per key, then a segmented tree sum
      with_group(sig_group, [&](auto G) {
        KL(KID_SECURE_LADDER, k_secure_ladder<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, sp, fmt, (const uint8_t*)b.scal, (const uint32_t*)d_first,
           (const uint32_t*)b.sid, (const uint32_t*)b.flags, b.part);
      });
      for (uint64_t step = 1; step < plan.tmax_small; step <<= 1) {
        with_group(sig_group, [&](auto G) {
          KL(KID_SECURE_AGG_FOLD, k_share_fold<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, step, o, (const uint32_t*)b.sid, b.part);
        });
      }
      HIPCK(hipGetLastError());
    }
    // the large sets, one at a time as blsgpu_aggregate_secure runs them; the sum goes to the set's first record (where the fold left
    // the identity), a zero coefficient into the set's flags (1 = SECURE_F_ZERO).  The workspace is reused from set to set; so is
    // the pinned record of the digest, which the next set writes only after its sort has synchronised the stream.
    const size_t mark = c->arena_off, hmark = c->hsmall_off;
    for (size_t s = 0; s < n_sets; s++) {
      if (!(plan.hflags[s] & SECURE_F_LARGE)) continue;
      const size_t lo = (size_t)offs[s], t = (size_t)(offs[s + 1] - offs[s]), T = accumulate_lanes(t);
      c->arena_off = mark;
      c->hsmall_off = hmark;
      uint8_t* d_msm = (uint8_t*)arena_take(c, osz * T);
      if (!d_msm) return fail(BLSGPU_E_HIP, "internal: arena too small");
      if ((rc = run_aggregate_secure_set(c, sig_group, b.bytes + width * lo, sp + ssz * lo, t, width, fmt, (int32_t*)(b.flags + s), d_msm, T))) return rc;
      HIPCK(hipMemcpyAsync(b.part + osz * lo, d_msm, osz, hipMemcpyDeviceToDevice, c->stream));
    }
    c->arena_off = mark;
  }
  with_group(sig_group, [&](auto G) {
    KL(KID_SECURE_AGG_OUT, k_set_sum_out<G()>, dim3(blocks_for(n_sets)), dim3(BLS_BLOCK), n_sets, o, o, (const uint32_t*)b.flags, (const uint8_t*)b.part, d_out,
       d_st);
  });
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out_sigs, d_out, osz * n_sets))) return rc;
  return status_out_and_sync(c, status, d_st, n_sets);
}
API_CATCH

int blsgpu_sum_batch(int group, const void* pts, const uint64_t* offsets, size_t n_sets, int fmt, void* out) try {
  if (!initialised()) return NOT_INIT();
  if (group != 1 && group != 2) return fail(BLSGPU_E_ARG, "group must be 1 (G1) or 2 (G2)");
  if (fmt != BLSGPU_FMT_RAW_PROJ && fmt != BLSGPU_FMT_RAW_AFFINE) return fail(BLSGPU_E_ARG, "fmt must be RAW_PROJ or RAW_AFFINE");
  std::vector<uint64_t> offs;
  int rc = sum_args_read(offs, pts, offsets, n_sets, out);
  if (rc || n_sets == 0) return rc;
  CTX_ACQUIRE(c);
  const keys_by_value keys = {pts, group, fmt, 0, KID_SUM_SEG_ACCUM, point_bytes(group, fmt) * (size_t)offs[n_sets]};
  return sum_batch_run(c, group, keys, offs, n_sets, out);
}
API_CATCH
// =========================================================================================================
// Registered key sets (keyset.cuh): a table of public keys that stays on the device, sets named by positions in it
static int keyset_fmt_check(int sig_group, int fmt) {
  if (sig_group != 1 && sig_group != 2) return fail(BLSGPU_E_ARG, "sig_group must be 1 (Bls12381G1Impl) or 2 (Bls12381G2Impl)");
  if (fmt < BLSGPU_FMT_RAW_PROJ || fmt > BLSGPU_FMT_LEGACY) return fail(BLSGPU_E_ARG, "fmt must be one of BLSGPU_FMT_*");
  if (fmt == BLSGPU_FMT_LEGACY && sig_group != 2)
    return fail(BLSGPU_E_ARG, "Legacy serialization exists only for Bls12381G2Impl (48-byte keys), reference src/signature.rs:201-204");
  return 0;
}
// scal[i] * key[cidx[i]] for every position: from the fixed-base tables when the set has them, else the joint NAF ladder
static int keyset_launch_mul(Ctx* c, const KeySet& k, size_t n, const uint32_t* d_cidx, const uint8_t* d_scal, const uint32_t* d_sid, const uint32_t* d_flags,
                             uint8_t* d_part) {
  with_group(k.group, [&](auto G) {
    if (k.table)
      KL(KID_KEYSET_MUL, (k_keyset_mul<G(), 1>), dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)k.aff, (const uint8_t*)k.table, d_cidx, d_scal, d_sid,
         d_flags, d_part);
    else
      KL(KID_KEYSET_MUL, (k_keyset_mul<G(), 0>), dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)k.aff, (const uint8_t*)nullptr, d_cidx, d_scal, d_sid,
         d_flags, d_part);
  });
  return 0;
}
// the fixed-base tables of a new set, chunk by chunk through a workspace that lives for this call only; leaves k.table null (and
// the set without tables) when the knob or the device's memory says no
static int keyset_build_tables(Ctx* c, KeySet& k) {
  const size_t tb = keyset_table_bytes(k.group, k.n);
  if (k.n == 0 || tb > ((size_t)knobs().keyset_table_mb << 20)) return 0;
  const size_t chunk = std::min<size_t>(k.n, 4096);
  const size_t rec = keyset_table_bytes(k.group, 1);                   // one key's table: POINTS (x, y) records
  uint8_t *table = nullptr, *jac_ws = nullptr, *prod_ws = nullptr;
  if (hipMalloc((void**)&table, tb) != hipSuccess || hipMalloc((void**)&jac_ws, chunk * (rec / 2 * 3)) != hipSuccess ||
      hipMalloc((void**)&prod_ws, chunk * (rec / 2)) != hipSuccess) {
    (void)hipGetLastError();
    for (void* p : {(void*)table, (void*)jac_ws, (void*)prod_ws})
      if (p) (void)hipFree(p);
    return 0;
  }
  for (size_t k0 = 0; k0 < k.n; k0 += chunk) {
    const size_t cnt = std::min(chunk, k.n - k0);
    with_group(k.group, [&](auto G) {
      KL(KID_KEYSET_BUILD, k_keyset_build<G()>, dim3(blocks_for(cnt)), dim3(BLS_BLOCK), k0, cnt, (const uint8_t*)k.aff, jac_ws, prod_ws, table);
    });
  }
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
  (void)hipFree(jac_ws);
  (void)hipFree(prod_ws);
  if (e1 != hipSuccess || e2 != hipSuccess) {
    (void)hipFree(table);
    return fail(BLSGPU_E_HIP, std::string("k_keyset_build: ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2));
  }
  k.table = table;
  k.bytes += tb;
  return 0;
}
// ---- what the three kinds of registered set share: rows, growth, the tail of an append, the positions of an update
extern "C++" {
// a device buffer that lives for one call
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};
// k_keyset_lines[_at] work in chunks of 4,096 entries so that the scratch rows they need (as much again as the rows they write)
// stay at 62 MB
static size_t set_lines_scratch_bytes(size_t count) { return std::min<size_t>(count, 4096) * (size_t)KEYSET_LINES_KEY_BYTES; }
// the rows of `count` entries of a set that has rows, through a scratch of set_lines_scratch_bytes(count): the entries d_pos[0 .. count)
// (k_keyset_lines_at) or -- d_pos == nullptr -- the entries [first, first + count) (k_keyset_lines)
static void set_launch_lines(Ctx* c, const DevSet& s, const uint32_t* d_pos, size_t first, size_t count, void* scratch) {
  const size_t chunk = std::min<size_t>(count, 4096);
  for (size_t l0 = 0; l0 < count; l0 += chunk) {
    const size_t cnt = std::min(chunk, count - l0);
    if (d_pos)
      KL(KID_KEYSET_LINES_AT, k_keyset_lines_at, dim3(blocks_for(2 * cnt)), dim3(BLS_BLOCK), cnt, d_pos + l0, (const uint8_t*)s.aff, s.lines, (uint32_t*)scratch,
         s.nolines);
    else
      KL(KID_KEYSET_LINES, k_keyset_lines, dim3(blocks_for(2 * cnt)), dim3(BLS_BLOCK), first + l0, cnt, (const uint8_t*)s.aff, s.lines, (uint32_t*)scratch, s.nolines);
  }
}
// One array of a growing set: `bytes_new` bytes with the first `bytes_old` copied from *p; *p is replaced and the old array left in
// *old for the caller to free once no record names it.  false: the device has no room (or the copy failed) and *p is untouched.
static bool set_grow(Ctx* c, void** p, size_t bytes_old, size_t bytes_new, void** old) {
  void* q = nullptr;
  if (hipMalloc(&q, std::max<size_t>(bytes_new, 1)) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (bytes_old && (hipMemcpyAsync(q, *p, bytes_old, hipMemcpyDeviceToDevice, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)) {
    (void)hipGetLastError();
    (void)hipFree(q);
    return false;
  }
  *old = *p;
  *p = q;
  return true;
}
// what a kind builds besides rows once the tail of an append is published: a key set the tables its creator asked for and it lacks.
// They share the rows' cap, so rows that no longer fit beside them are dropped.
static int set_build_others(Ctx*, uint64_t, DevSet&) { return 0; }
static int set_build_others(Ctx* c, uint64_t handle, KeySet& k) {
  if (!(k.flags & BLSGPU_KEYSET_TABLES) || k.table) return 0;
  int rc = keyset_build_tables(c, k);
  if (rc) return rc;
  if (k.table && k.lines && !keyset_lines_fit(k.n, keyset_table_bytes(k.group, k.n), (uint64_t)knobs().keyset_table_mb)) {
    void *old = k.lines, *old_no = k.nolines;
    k.lines = nullptr;
    k.nolines = nullptr;
    k.bytes = set_bytes(k);
    set_publish(handle, k);
    (void)hipFree(old);
    (void)hipFree(old_no);
  } else if (k.table) {
    set_publish(handle, k);
  }
  return 0;
}
// the rows of a whole set whose entries are in G2, in chunks of 4,096 entries; leaves s.lines null (and the set without rows) when
// the size rule (keyset_lines_fit: the 32-bit offset of the kernels that read them, and the cap of BLSGPU_KEYSET_TABLE_MB together
// with a key set's fixed-base tables) or the device's memory says no
template <class T>
static int set_build_lines(Ctx* c, T& s) {
  if (set_rows_group(s) != 2 || !keyset_lines_fit(s.n, set_other_bytes(s, s.n), (uint64_t)knobs().keyset_table_mb)) return 0;
  uint32_t *lines = nullptr, *scratch = nullptr;
  int32_t* nolines = nullptr;
  if (hipMalloc((void**)&lines, s.n * (size_t)KEYSET_LINES_KEY_BYTES) != hipSuccess || hipMalloc((void**)&scratch, set_lines_scratch_bytes(s.n)) != hipSuccess ||
      hipMalloc((void**)&nolines, 4 * s.n) != hipSuccess) {
    (void)hipGetLastError();
    for (void* p : {(void*)lines, (void*)scratch, (void*)nolines})
      if (p) (void)hipFree(p);
    return 0;
  }
  s.lines = lines;
  s.nolines = nolines;
  set_launch_lines(c, s, nullptr, 0, s.n, scratch);
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
  (void)hipFree(scratch);
  if (e1 != hipSuccess || e2 != hipSuccess) {
    (void)hipFree(lines);
    (void)hipFree(nolines);
    s.lines = nullptr;
    s.nolines = nullptr;
    return fail(BLSGPU_E_HIP, std::string("k_keyset_lines: ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2));
  }
  s.bytes = set_bytes(s);
  return 0;
}
// An append, step 1: room for n1 entries in the arrays that hold a record per entry -- all of the new arrays before any of the old
// ones goes, so that a refusal leaves the set as it was; the published record keeps n0 until the tail is written.
template <class T>
static int set_grow_base(Ctx* c, uint64_t handle, T& s, size_t n0, size_t n1) {
  T g = s;
  const std::vector<SetArray> arrays = set_arrays(g);
  std::vector<void*> old(arrays.size(), nullptr);
  for (size_t i = 0; i < arrays.size(); i++)
    if (!set_grow(c, arrays[i].p, arrays[i].entry_bytes * n0, arrays[i].entry_bytes * n1, &old[i])) {
      for (size_t j = 0; j < i; j++) (void)hipFree(*arrays[j].p);
      return fail(BLSGPU_E_HIP, std::string("no device memory for the grown ") + set_name(s));
    }
  s = g;
  set_publish(handle, s);
  for (void* p : old) (void)hipFree(p);
  return 0;
}
// step 2: rows by the creation rule on the final size: grown, or dropped (the set works without them)
template <class T>
static void set_grow_or_drop_lines(Ctx* c, uint64_t handle, T& s, size_t n0, size_t n1) {
  if (!s.lines) return;
  void *old = nullptr, *old_no = nullptr, *unused = nullptr;
  bool keep = keyset_lines_fit(n1, set_other_bytes(s, n1), (uint64_t)knobs().keyset_table_mb) &&
              set_grow(c, (void**)&s.lines, n0 * (size_t)KEYSET_LINES_KEY_BYTES, n1 * (size_t)KEYSET_LINES_KEY_BYTES, &old);
  if (keep && !set_grow(c, (void**)&s.nolines, 4 * n0, 4 * n1, &old_no)) {
    unused = s.lines;                         // the grown rows go with the old ones
    s.lines = (uint32_t*)old;
    keep = false;
  }
  if (!keep) {
    old = s.lines;
    old_no = s.nolines;
    s.lines = nullptr;
    s.nolines = nullptr;
  }
  s.bytes = set_bytes(s);
  set_publish(handle, s);
  for (void* p : {old, old_no, unused}) (void)hipFree(p);
}
// step 4, once the kind's apply has written the tail (the published record still said n0, so nothing named the new entries before
// they were whole): the record says n1; then what the creator asked for and the set does not have (an empty set has nothing) is
// built whole where creation would build it -- a key set's tables first, then the rows in what the cap leaves.  Every record
// published on the way is a whole set.
template <class T>
static int set_finish_append(Ctx* c, uint64_t handle, T& s, size_t n1) {
  s.n = n1;
  s.bytes = set_bytes(s);
  set_publish(handle, s);
  int rc = set_build_others(c, handle, s);
  if (rc) return rc;
  if ((s.flags & set_rows_flag(s)) && !s.lines) {
    if ((rc = set_build_lines(c, s))) return rc;
    if (s.lines) set_publish(handle, s);
  }
  SYNC_FLUSH(c);
  return 0;
}
// the position list of an update, on the host (copied down first when it lives on the device) and checked: in range, no two equal
template <class T>
static int set_read_checked_positions(const T& s, const uint32_t* pos, size_t count, std::vector<uint32_t>& h) {
  h.resize(count);
  if (is_device_ptr(pos)) HIPCK(hipMemcpy(h.data(), pos, 4 * count, hipMemcpyDeviceToHost));
  else memcpy(h.data(), pos, 4 * count);
  switch (keyset_positions_check(h.data(), count, s.n)) {
    case KEYSET_POS_RANGE: return fail(BLSGPU_E_ARG, std::string("a position is outside the ") + set_name(s));
    case KEYSET_POS_DUP: return fail(BLSGPU_E_ARG, "the same position twice in one update");
  }
  return 0;
}
}  // extern "C++"
int blsgpu_keyset_create(int sig_group, const void* keys, size_t n, int fmt, int flags, int32_t* status, uint64_t* out_handle) try {
  if (!initialised()) return NOT_INIT();
  int rc = keyset_fmt_check(sig_group, fmt);
  if (rc) return rc;
  if (!out_handle || (n && !keys)) return fail(BLSGPU_E_ARG, "null argument");
  if (flags & ~(BLSGPU_KEYSET_TABLES | BLSGPU_KEYSET_LINES)) return fail(BLSGPU_E_ARG, "unknown flag");
  if (n >= 0xffffffffull) return fail(BLSGPU_E_ARG, "more than 2^32 - 2 keys");
  *out_handle = 0;
  CTX_ACQUIRE(c);
  KeySet k;
  k.sig_group = sig_group;
  k.group = key_group(sig_group);
  k.flags = flags;
  k.n = n;
  k.devidx = t_devidx;
  k.dev = c->dev;
  const bool wire = fmt == BLSGPU_FMT_COMPRESSED || fmt == BLSGPU_FMT_LEGACY;
  const size_t isz = point_bytes(k.group, fmt), osz = point_bytes(k.group, BLSGPU_FMT_RAW_PROJ), asz = point_bytes(k.group, BLSGPU_FMT_RAW_AFFINE),
               csz = point_bytes(k.group, BLSGPU_FMT_COMPRESSED), m = std::max<size_t>(n, 1);
  struct Guard {
    KeySet* k;
    ~Guard() {
      if (k) set_free(*k);
    }
  } guard{&k};
  HIPCK(hipMalloc((void**)&k.aff, asz * m));
  HIPCK(hipMalloc((void**)&k.comp, csz * m));
  HIPCK(hipMalloc((void**)&k.status, 4 * m));
  k.bytes = set_bytes(k);
  if (n) {
    if ((rc = arena_reserve(c, pad256(isz * n) + pad256(osz * n) + 4096))) return rc;
    c->arena_off = 0;
    const void* d_in;
    if ((rc = stage_in(c, keys, isz * n, &d_in))) return rc;
    const uint8_t* d_pts = (const uint8_t*)d_in;
    int kfmt = fmt;
    if (wire) {
      // PublicKey::from_bytes[_with_mode]: the checked decompression of blsgpu_deserialize; its status is the entry's
      uint8_t* d_raw = (uint8_t*)arena_take(c, osz * n);
      if (!d_raw) return fail(BLSGPU_E_HIP, "internal: arena too small");
      with_group(k.group, [&](auto G) {
        KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_pts, (int)(fmt == BLSGPU_FMT_LEGACY), d_raw, k.status, 0);
      });
      d_pts = d_raw;
      kfmt = BLSGPU_FMT_RAW_PROJ;
    } else {
      HIPCK(hipMemsetAsync(k.status, 0, 4 * n, c->stream));
    }
    with_group(k.group, [&](auto G) {
      KL(KID_KEYSET_SEAL, k_keyset_seal<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_pts, kfmt, (const int32_t*)k.status, k.aff, k.comp);
    });
    HIPCK(hipGetLastError());
    if (status && (rc = copy_out(c, status, k.status, 4 * n))) return rc;
    if ((flags & BLSGPU_KEYSET_TABLES) && (rc = keyset_build_tables(c, k))) return rc;
    if ((flags & BLSGPU_KEYSET_LINES) && (rc = set_build_lines(c, k))) return rc;
    SYNC_FLUSH(c);
  }
  *out_handle = set_issue(k);
  guard.k = nullptr;
  return 0;
}
API_CATCH

int blsgpu_keyset_destroy(uint64_t handle) try { return set_destroy<KeySet>(handle); }
API_CATCH

// ---- blsgpu_keyset_update / blsgpu_keyset_append: `count` keys in `fmt` become the entries h_pos[0 .. count) of k (positions the
// caller has checked with keyset_positions_check: in range, no two equal).  The steps of creation on those entries alone:
// the checked decompression of a wire format, k_keyset_seal_at (record, Modern bytes, status), and -- for a set that has them --
// k_keyset_build_at and k_keyset_lines_at in chunks of 4,096 keys through workspaces that live for this call only.  The
// workspaces are allocated before anything is written, so a device without room for them leaves the set as it was.
static int keyset_apply(Ctx* c, const KeySet& k, const uint32_t* h_pos, const void* keys, size_t count, int fmt, int32_t* status) {
  const bool wire = fmt == BLSGPU_FMT_COMPRESSED || fmt == BLSGPU_FMT_LEGACY;
  const size_t isz = point_bytes(k.group, fmt), osz = point_bytes(k.group, BLSGPU_FMT_RAW_PROJ), chunk = std::min<size_t>(count, 4096);
  const size_t rec = keyset_table_bytes(k.group, 1);
  int rc = arena_reserve(c, pad256(isz * count) + pad256(osz * count) + 2 * pad256(4 * count) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  DevBuf jac, prod, scratch;
  if (k.table) {
    HIPCK(hipMalloc(&jac.p, chunk * (rec / 2 * 3)));
    HIPCK(hipMalloc(&prod.p, chunk * (rec / 2)));
  }
  if (k.lines) HIPCK(hipMalloc(&scratch.p, set_lines_scratch_bytes(count)));
  Carver mem{c};
  uint32_t* d_pos = mem.take<uint32_t>(4 * count);
  int32_t* d_st = mem.take<int32_t>(4 * count);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  HIPCK(hipMemcpyAsync(d_pos, h_pos, 4 * count, hipMemcpyHostToDevice, c->stream));
  const void* d_in;
  if ((rc = stage_in(c, keys, isz * count, &d_in))) return rc;
  const uint8_t* d_pts = (const uint8_t*)d_in;
  int kfmt = fmt;
  if (wire) {
    uint8_t* d_raw = (uint8_t*)arena_take(c, osz * count);
    if (!d_raw) return fail(BLSGPU_E_HIP, "internal: arena too small");
    with_group(k.group, [&](auto G) {
      KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(count)), dim3(BLS_BLOCK), count, d_pts, (int)(fmt == BLSGPU_FMT_LEGACY), d_raw, d_st, 0);
    });
    d_pts = d_raw;
    kfmt = BLSGPU_FMT_RAW_PROJ;
  } else {
    HIPCK(hipMemsetAsync(d_st, 0, 4 * count, c->stream));
  }
  with_group(k.group, [&](auto G) {
    KL(KID_KEYSET_SEAL_AT, k_keyset_seal_at<G()>, dim3(blocks_for(count)), dim3(BLS_BLOCK), count, d_pts, kfmt, (const int32_t*)d_st, (const uint32_t*)d_pos,
       k.aff, k.comp, k.status);
  });
  for (size_t l0 = 0; l0 < count; l0 += chunk) {
    const size_t cnt = std::min(chunk, count - l0);
    if (k.table)
      with_group(k.group, [&](auto G) {
        KL(KID_KEYSET_BUILD_AT, k_keyset_build_at<G()>, dim3(blocks_for(cnt)), dim3(BLS_BLOCK), cnt, (const uint32_t*)d_pos + l0, (const uint8_t*)k.aff,
           (uint8_t*)jac.p, (uint8_t*)prod.p, k.table);
      });
    if (k.lines) set_launch_lines(c, k, d_pos + l0, 0, cnt, scratch.p);       // this chunk's rows, after its tables
  }
  HIPCK(hipGetLastError());
  if (status && (rc = copy_out(c, status, d_st, 4 * count))) return rc;
  SYNC_FLUSH(c);                      // before the workspaces go
  return 0;
}

int blsgpu_keyset_update(uint64_t handle, const uint32_t* pos, const void* keys, size_t count, int fmt, int32_t* status) try {
  KeySet k;
  int rc = set_find(handle, k);
  if (rc) return rc;
  if ((rc = keyset_fmt_check(k.sig_group, fmt))) return rc;
  if (count == 0) return 0;
  if (!pos || !keys) return fail(BLSGPU_E_ARG, "null argument");
  if (count > k.n) return fail(BLSGPU_E_ARG, "more positions than the key set has entries");
  CTX_ACQUIRE_ON(c, k.devidx);
  std::vector<uint32_t> h_pos;
  if ((rc = set_read_checked_positions(k, pos, count, h_pos))) return rc;
  return keyset_apply(c, k, h_pos.data(), keys, count, fmt, status);
}
API_CATCH

int blsgpu_keyset_append(uint64_t handle, const void* keys, size_t count, int fmt, int32_t* status, uint64_t* out_first) try {
  KeySet k;
  int rc = set_find(handle, k);
  if (rc) return rc;
  if ((rc = keyset_fmt_check(k.sig_group, fmt))) return rc;
  if (count && !keys) return fail(BLSGPU_E_ARG, "null argument");
  if (keyset_positions_check(nullptr, count, k.n) != KEYSET_POS_OK) return fail(BLSGPU_E_ARG, "more than 2^32 - 2 keys");
  if (out_first) *out_first = k.n;
  if (count == 0) return 0;
  CTX_ACQUIRE_ON(c, k.devidx);
  const size_t n0 = k.n, n1 = k.n + count;
  if ((rc = set_grow_base(c, handle, k, n0, n1))) return rc;
  if (k.table) {  // the tables by the creation rule on the final size: grown, or dropped (the set works without them)
    void* old = nullptr;
    const size_t tb = keyset_table_bytes(k.group, n1);
    if (tb > (size_t)knobs().keyset_table_mb << 20 || !set_grow(c, (void**)&k.table, keyset_table_bytes(k.group, n0), tb, &old)) {
      old = k.table;
      k.table = nullptr;
    }
    k.bytes = set_bytes(k);
    set_publish(handle, k);
    (void)hipFree(old);
  }
  set_grow_or_drop_lines(c, handle, k, n0, n1);
  // the tail through the update path
  std::vector<uint32_t> h_pos(count);
  for (size_t i = 0; i < count; i++) h_pos[i] = (uint32_t)(n0 + i);
  if ((rc = keyset_apply(c, k, h_pos.data(), keys, count, fmt, status))) return rc;
  return set_finish_append(c, handle, k, n1);
}
API_CATCH

int blsgpu_keyset_info(uint64_t handle, int* sig_group, uint64_t* n, int* has_tables, uint64_t* device_bytes) try {
  KeySet k;
  int rc = set_find(handle, k);
  if (rc) return rc;
  if (sig_group) *sig_group = k.sig_group;
  if (n) *n = k.n;
  if (has_tables) *has_tables = (k.table ? BLSGPU_KEYSET_TABLES : 0) | (k.lines ? BLSGPU_KEYSET_LINES : 0);
  if (device_bytes) *device_bytes = k.bytes;
  return 0;
}
API_CATCH

// the indices of a call against the table: d_cidx gets idx[i] or KEYSET_SKIP, d_pre (n_sets slots, or one when d_offs is null and
// `whole` is set: the whole call is one set) each set's precedence
// d_walk (a set with line tables, a call that may take a kernel that reads the rows): one word, raised when a position names a finite
// entry without usable rows
static int keyset_check(Ctx* c, const KeySet& k, const uint32_t* d_idx, size_t n, const uint64_t* d_offs, size_t n_sets, uint32_t* d_cidx,
                        unsigned long long* d_pre, uint32_t* d_walk = nullptr) {
  HIPCK(hipMemsetAsync(d_pre, 0xff, 8 * n_sets, c->stream));
  if (d_walk) HIPCK(hipMemsetAsync(d_walk, 0, 4, c->stream));
  if (n)
    KL(KID_KEYSET_CHECK, k_keyset_check, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_offs, n_sets, d_idx, (uint64_t)k.n, (const int32_t*)k.status, d_cidx,
       d_pre, d_walk ? (const int32_t*)k.nolines : (const int32_t*)nullptr, d_walk);
  return 0;
}
// May a one-key-per-item call of n items over set k read the keys' rows?  Decided from the call's shape: a set with line tables
// (so: signatures in G1) above the row-wide engine's range -- on the one-wave path (k_pairing_coop_keyed), or on the lane-split
// path with its two-kernel Miller loop (k_lines2s_keyed).  At and below BLSGPU_WIDE_MAX items a call gains no read-back.
static bool keyset_lines_wanted(const KeySet& k, size_t n) {
  return k.lines && k.sig_group == 1 && pair_path_reads_rows(n);
}
// ... and, after k_keyset_check with d_walk: the one word read back (as run_verify_shared_items reads k_group_lines' word) says
// whether every named entry has rows; *table = the set's rows, or null: the call walks the keys
static int keyset_lines_decide(Ctx* c, const KeySet& k, const uint32_t* d_walk, const uint32_t** table) {
  uint32_t walk = 0;
  const int rc = word_back(c, d_walk, &walk);
  *table = !rc && walk == 0 ? k.lines : nullptr;
  return rc;
}
// for the calls without a status vector: one set over all positions; after the call's last synchronisation *h_pre == 0 says that
// some index was outside the table
static int keyset_check_whole(Ctx* c, const KeySet& k, const void* idx, size_t n, uint32_t** d_cidx, unsigned long long** h_pre) {
  const void* d_idx;
  int rc = stage_in(c, idx, 4 * n, &d_idx);
  if (rc) return rc;
  Carver mem{c};
  uint64_t* d_one = mem.take<uint64_t>(16);
  unsigned long long* d_pre = mem.take<unsigned long long>(8);
  *d_cidx = mem.take<uint32_t>(4 * n);
  *h_pre = (unsigned long long*)hsmall_take(c, 8);
  if (!mem.ok || !*h_pre) return fail(BLSGPU_E_HIP, "internal: arena too small");
  const uint64_t one[2] = {0, (uint64_t)n};
  if ((rc = h2d_small(c, d_one, one, 16))) return rc;
  if ((rc = keyset_check(c, k, (const uint32_t*)d_idx, n, d_one, 1, *d_cidx, d_pre))) return rc;
  HIPCK(hipMemcpyAsync(*h_pre, d_pre, 8, hipMemcpyDeviceToHost, c->stream));
  return 0;
}
// cnt records of `words` words each, record i from entry d_cidx[i] of the set's array src
#define KEYSET_GATHER(cnt, words, src, legacy, dst) \
  KL(KID_KEYSET_GATHER, k_keyset_gather, dim3(blocks_for((size_t)(cnt) * (words))), dim3(BLS_BLOCK), (size_t)(cnt), (size_t)(words), (const uint32_t*)d_cidx, \
     (const uint32_t*)(src), legacy, (uint32_t*)(dst))
// the keys a call names, in its own order and in its signatures' format: the affine records into d_aff, and for RAW_PROJ
// (d_keys != d_aff) k_keyset_to_proj of those into d_keys
static void keyset_gather_keys(Ctx* c, const KeySet& k, const uint32_t* d_cidx, size_t cnt, uint8_t* d_aff, uint8_t* d_keys) {
  KEYSET_GATHER(cnt, point_bytes(k.group, BLSGPU_FMT_RAW_AFFINE) / 4, k.aff, 0, d_aff);
  if (d_keys != d_aff)
    with_group(k.group, [&](auto G) { KL(KID_KEYSET_GATHER, k_keyset_to_proj<G()>, dim3(blocks_for(cnt)), dim3(BLS_BLOCK), cnt, (const uint8_t*)d_aff, d_keys); });
}

int blsgpu_keyset_get(uint64_t handle, const uint32_t* idx, size_t count, int fmt_out, void* out, int32_t* status) try {
  KeySet k;
  int rc = set_find(handle, k);
  if (rc) return rc;
  if ((rc = keyset_fmt_check(k.sig_group, fmt_out))) return rc;
  if (count == 0) return 0;
  if (!idx || !out) return fail(BLSGPU_E_ARG, "null argument");
  if (count >= ((size_t)1 << 32)) return fail(BLSGPU_E_ARG, "2^32 or more positions in one call");
  CTX_ACQUIRE_ON(c, k.devidx);
  const size_t asz = point_bytes(k.group, BLSGPU_FMT_RAW_AFFINE), csz = point_bytes(k.group, BLSGPU_FMT_COMPRESSED), osz = point_bytes(k.group, fmt_out);
  if ((rc = arena_reserve(c, 2 * pad256(4 * count) + pad256(asz * count) + pad256(osz * count) + pad256(4 * count) + 4096))) return rc;
  c->arena_off = 0;
  uint32_t* d_cidx;
  unsigned long long* h_pre;
  if ((rc = keyset_check_whole(c, k, idx, count, &d_cidx, &h_pre))) return rc;
  Carver mem{c};
  uint8_t* d_out = mem.stage_out<uint8_t>(out, osz * count);
  int32_t* d_st = status ? mem.stage_out<int32_t>(status, 4 * count) : nullptr;
  uint8_t* d_aff = fmt_out == BLSGPU_FMT_RAW_PROJ ? mem.take<uint8_t>(asz * count) : nullptr;
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if (fmt_out == BLSGPU_FMT_RAW_AFFINE || fmt_out == BLSGPU_FMT_RAW_PROJ)
    keyset_gather_keys(c, k, d_cidx, count, d_aff ? d_aff : d_out, d_out);
  else
    KEYSET_GATHER(count, csz / 4, k.comp, (int)(fmt_out == BLSGPU_FMT_LEGACY), d_out);       // the Legacy header is a transcode of byte 0
  if (d_st) KEYSET_GATHER(count, 1, k.status, 0, d_st);
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out, d_out, osz * count))) return rc;
  if (d_st && (rc = stage_back(c, status, d_st, 4 * count))) return rc;
  SYNC_FLUSH(c);
  if (*h_pre == 0) return fail(BLSGPU_E_ARG, "an index is outside the key set");
  return 0;
}
API_CATCH

int blsgpu_keyset_mul(uint64_t handle, const uint32_t* idx, const uint8_t* scalars, size_t count, void* out) try {
  KeySet k;
  int rc = set_find(handle, k);
  if (rc) return rc;
  if (count == 0) return 0;
  if (!idx || !scalars || !out) return fail(BLSGPU_E_ARG, "null argument");
  if (count >= ((size_t)1 << 32)) return fail(BLSGPU_E_ARG, "2^32 or more positions in one call");
  CTX_ACQUIRE_ON(c, k.devidx);
  const size_t osz = point_bytes(k.group, BLSGPU_FMT_RAW_PROJ);
  if ((rc = arena_reserve(c, 2 * pad256(4 * count) + pad256(32 * count) + pad256(osz * count) + 4096))) return rc;
  c->arena_off = 0;
  uint32_t* d_cidx;
  unsigned long long* h_pre;
  if ((rc = keyset_check_whole(c, k, idx, count, &d_cidx, &h_pre))) return rc;
  const void* d_scal;
  if ((rc = stage_in(c, scalars, 32 * count, &d_scal))) return rc;
  uint8_t* d_out = stage_out<uint8_t>(c, out, osz * count);
  if (!d_out) return fail(BLSGPU_E_HIP, "internal: arena too small");
  rc = keyset_launch_mul(c, k, count, d_cidx, (const uint8_t*)d_scal, nullptr, nullptr, d_out);
  if (rc) return rc;
  HIPCK(hipGetLastError());
  if ((rc = stage_back(c, out, d_out, osz * count))) return rc;
  SYNC_FLUSH(c);
  if (*h_pre == 0) return fail(BLSGPU_E_ARG, "an index is outside the key set");
  return 0;
}
API_CATCH

// ---- the batched entry points over a key set: (handle, idx) in place of the keys; fmt describes the signatures only
// the arguments of the secure and multi verify, checked and read as their by-value twins': the key set gives the signature group,
// idx stands for the keys
struct indexed_args : set_args {
  KeySet k;
};
static int indexed_begin(indexed_args& a, int scheme, uint64_t keyset, const uint32_t* idx, const uint64_t* key_offsets, size_t n_sets, const void* sigs,
                         const uint8_t* msgs, const uint64_t* msg_offsets, int fmt, int32_t* status) {
  int rc = set_find(keyset, a.k);
  if (rc) return rc;
  if ((rc = check_common(a.k.sig_group, scheme, fmt))) return rc;
  return set_args_read(a, idx, key_offsets, n_sets, sigs, msgs, msg_offsets, status);
}

// The keys of an indexed call: n positions in key set k (the hooks: above verify_secure_batch_run).  stage: the indices, and
// k_keyset_check of them into d_cidx (idx[i] or KEYSET_SKIP) and d_pre (each set's precedence); fin: k_keyset_fin, the precedence
// over the statuses.  The strip sums read the set's affine records through d_cidx.  For the secure verify: the stored compressed
// bytes (no compression and no inversion), one multiplication per key of a small set -- from the fixed-base tables when the set
// has them -- and for the large sets one gather of the affine records into the arena.
struct keys_indexed {
  const KeySet& k;
  const void* idx;
  size_t n;
  int ser_format;
  mutable uint32_t* d_cidx = nullptr;
  mutable unsigned long long* d_pre = nullptr;
  mutable uint8_t* d_keys = nullptr;
  size_t asz() const { return point_bytes(k.group, BLSGPU_FMT_RAW_AFFINE); }
  size_t arena_bytes(size_t n_sets, bool large) const { return 2 * pad256(4 * n) + pad256(8 * n_sets) + (large ? pad256(asz() * n) : 0); }
  int stage(Ctx* c, const uint64_t* o, size_t n_sets, bool large) const {
    const void* d_idx = nullptr;
    int rc;
    if (n && (rc = stage_in(c, idx, 4 * n, &d_idx))) return rc;
    Carver mem{c};
    d_cidx = mem.take<uint32_t>(4 * n);
    d_pre = mem.take<unsigned long long>(8 * n_sets);
    if (large) d_keys = mem.take<uint8_t>(asz() * n);
    if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
    return keyset_check(c, k, (const uint32_t*)d_idx, n, o, n_sets, d_cidx, d_pre);
  }
  void key_bytes(Ctx* c, size_t cnt, uint8_t* d_bytes) const { KEYSET_GATHER(cnt, point_bytes(k.group, BLSGPU_FMT_COMPRESSED) / 4, k.comp, ser_format, d_bytes); }
  void mul_small(Ctx* c, size_t cnt, const uint8_t* d_scal, const uint32_t* d_sid, const uint32_t* d_flags, uint8_t* d_part) const {
    (void)keyset_launch_mul(c, k, cnt, d_cidx, d_scal, d_sid, d_flags, d_part);
  }
  const uint8_t* large_keys(Ctx* c, size_t cnt, int* kfmt) const {
    KEYSET_GATHER(cnt, asz() / 4, k.aff, 0, d_keys);
    *kfmt = BLSGPU_FMT_RAW_AFFINE;
    return d_keys;
  }
  void accumulate(Ctx* c, size_t Q, const uint64_t* o, const uint64_t* so, const uint32_t* sid, uint8_t* d_part) const {
    const uint32_t* ci = d_cidx;
    with_group(k.group, [&](auto G) {
      KL(KID_KEYSET_ACCUM, k_keyset_accumulate_seg<G()>, dim3(blocks_for(G() * Q)), dim3(BLS_BLOCK), Q, (const uint8_t*)k.aff, ci, o, so, sid, d_part);
    });
  }
  void fin(Ctx* c, size_t n_sets, int32_t* d_status) const {
    KL(KID_KEYSET_FIN, k_keyset_fin, dim3(blocks_for(n_sets)), dim3(BLS_BLOCK), n_sets, (const unsigned long long*)d_pre, d_status);
  }
};
// ... of the indexed sum, a call without a status vector: keyset_check_whole in place of the per-set check, and after the call's
// synchronisation the one word that says whether some index was outside the table
struct keys_indexed_whole : keys_indexed {
  mutable unsigned long long* h_pre = nullptr;
  size_t arena_bytes(size_t, bool) const { return 2 * pad256(4 * n); }
  int stage(Ctx* c, const uint64_t*, size_t, bool) const { return keyset_check_whole(c, k, idx, n, &d_cidx, &h_pre); }
  int done() const { return *h_pre == 0 ? fail(BLSGPU_E_ARG, "an index is outside the key set") : 0; }
};

int blsgpu_multi_verify_indexed_batch(int scheme, uint64_t keyset, const uint32_t* idx, const uint64_t* key_offsets, size_t n_sets, const void* sigs,
                                      const uint8_t* msgs, const uint64_t* msg_offsets, int fmt, int32_t* status) try {
  indexed_args a;
  int rc = indexed_begin(a, scheme, keyset, idx, key_offsets, n_sets, sigs, msgs, msg_offsets, fmt, status);
  if (rc || n_sets == 0) return rc;
  CTX_ACQUIRE_ON(c, a.k.devidx);
  const keys_indexed keys = {a.k, idx, a.n, 0};
  return multi_verify_batch_run(c, a.k.sig_group, scheme, keys, a, n_sets, sigs, msgs, msg_offsets, fmt, status);
}
API_CATCH

int blsgpu_sum_indexed_batch(uint64_t keyset, const uint32_t* idx, const uint64_t* offsets, size_t n_sets, void* out) try {
  KeySet k;
  int rc = set_find(keyset, k);
  if (rc) return rc;
  std::vector<uint64_t> offs;
  rc = sum_args_read(offs, idx, offsets, n_sets, out);
  if (rc || n_sets == 0) return rc;
  CTX_ACQUIRE_ON(c, k.devidx);
  const keys_indexed_whole keys = {{k, idx, (size_t)offs[n_sets], 0}};
  return sum_batch_run(c, k.group, keys, offs, n_sets, out);
}
API_CATCH

int blsgpu_verify_secure_indexed_batch(int scheme, uint64_t keyset, const uint32_t* idx, const uint64_t* key_offsets, size_t n_sets, const void* sigs,
                                       const uint8_t* msgs, const uint64_t* msg_offsets, int ser_format, int fmt, int32_t* status) try {
  indexed_args a;
  int rc = indexed_begin(a, scheme, keyset, idx, key_offsets, n_sets, sigs, msgs, msg_offsets, fmt, status);
  if (rc || (rc = check_ser_format(a.k.sig_group, ser_format)) || n_sets == 0) return rc;
  CTX_ACQUIRE_ON(c, a.k.devidx);
  const keys_indexed keys = {a.k, idx, a.n, ser_format};
  return verify_secure_batch_run(c, a.k.sig_group, scheme, keys, a, n_sets, sigs, msgs, msg_offsets, fmt, status);
}
API_CATCH

// ---- The keys of a one-key-per-item door -- verify_shared_run, signcrypt_share_verify_run, msgset_verify; blsgpu_verify_indexed_batch
// keeps its own body on the indexed provider's stages -- n keys, item i's the i-th, by value or as positions in a key set.  The hooks:
//   indexed           constexpr: are the keys entries of a registered set?  (The plans that read BOTH G2 members from tables exist
//                     behind the indexed doors only.)
//   sig_group()       the orientation of the call: the caller's argument, or the key set's
//   devidx()          the device the call runs on: the calling thread's, or the key set's (CTX_ACQUIRE_ON)
//   null()            is the argument that stands for the keys missing?  (part of the door's "null argument" check)
//   arena_bytes(n)    what stage takes from the arena
//   stage(c, n, &d_keys, &key)  the keys on the device in the signatures' format fmt.  By index: the positions staged, k_keyset_check
//                     (every item its own set) into d_cidx and d_pre, over a set with line tables where the call's path may read rows
//                     the one word back that says whether every named entry has them (keyset_lines_decide: the provider's only
//                     synchronisation), k_keyset_gather of the affine records and k_keyset_to_proj for RAW_PROJ.  key: where a pairing
//                     kernel may take item i's G2 member from instead of walking it -- key.of = d_cidx, key.rows = the set's rows, or
//                     null: every key is walked (always so by value, where key stays empty).  run_pairing2 reads key only with
//                     fixed_g2 = 2 and rows (launch_pairing_coop, launch_lines2s), so Bls12381G2Impl may hand it on as it is.
//   fin(c, n, d_status)  after the door's own statuses: k_keyset_fin, the precedence of a position outside the set and of an invalid
//                     entry over them.  Returns whether anything was launched (by value: nothing).  Valid only after a
//                     successful stage: by index it reads the d_pre that stage carved.
struct item_keys_by_value {
  static constexpr bool indexed = false;
  const void* pks;
  int sg, fmt;
  int sig_group() const { return sg; }
  size_t devidx() const { return t_devidx; }
  bool null() const { return !pks; }
  size_t arena_bytes(size_t n) const { return pad256(pk_size(sg, fmt) * n); }
  int stage(Ctx* c, size_t n, const uint8_t** d_keys, TabledG2*) const { return stage_in(c, pks, pk_size(sg, fmt) * n, (const void**)d_keys); }
  bool fin(Ctx*, size_t, int32_t*) const { return false; }
};
struct item_keys_indexed {
  static constexpr bool indexed = true;
  const KeySet& k;
  const void* idx;
  int fmt;
  mutable unsigned long long* d_pre = nullptr;
  int sig_group() const { return k.sig_group; }
  size_t devidx() const { return k.devidx; }
  bool null() const { return !idx; }
  size_t asz() const { return point_bytes(k.group, BLSGPU_FMT_RAW_AFFINE); }
  size_t arena_bytes(size_t n) const {
    return 2 * pad256(4 * n) + pad256(8 * n) + pad256(asz() * n) + (fmt == BLSGPU_FMT_RAW_AFFINE ? 0 : pad256(point_bytes(k.group, fmt) * n)) + 256;
  }
  int stage(Ctx* c, size_t n, const uint8_t** keys_out, TabledG2* key) const {
    const void* d_idx;
    int rc = stage_in(c, idx, 4 * n, &d_idx);
    if (rc) return rc;
    Carver mem{c};
    uint32_t* d_cidx = mem.take<uint32_t>(4 * n);
    d_pre = mem.take<unsigned long long>(8 * n);
    // one key per item: the gather is a few hundred bytes against a pairing, so the keys go to the arena, in the signatures' format
    uint8_t* d_aff = mem.take<uint8_t>(asz() * n);
    uint8_t* d_keys = fmt == BLSGPU_FMT_RAW_AFFINE ? d_aff : mem.take<uint8_t>(point_bytes(k.group, fmt) * n);
    uint32_t* d_walk = keyset_lines_wanted(k, n) ? mem.take<uint32_t>(4) : nullptr;
    if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
    if ((rc = keyset_check(c, k, (const uint32_t*)d_idx, n, nullptr, n, d_cidx, d_pre, d_walk))) return rc;
    key->of = d_cidx;
    key->rows = nullptr;       // ... unless the word says otherwise: a named finite entry without rows makes every item walk
    if (d_walk && (rc = keyset_lines_decide(c, k, d_walk, &key->rows))) return rc;
    keyset_gather_keys(c, k, d_cidx, n, d_aff, d_keys);
    *keys_out = d_keys;
    return 0;
  }
  bool fin(Ctx* c, size_t n, int32_t* d_status) const {
    KL(KID_KEYSET_FIN, k_keyset_fin, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const unsigned long long*)d_pre, d_status);
    return true;
  }
};

// Launch sequence: the provider's stage (k_keyset_check, [one word back], k_keyset_gather), run_verify_items with the keys' rows
// where the set has them, k_keyset_fin.
int blsgpu_verify_indexed_batch(int scheme, uint64_t keyset, const uint32_t* idx, const void* sigs, const uint8_t* msgs, const uint64_t* msg_offsets,
                                size_t n, int fmt, int32_t* status) try {
  KeySet k;
  int rc = set_find(keyset, k);
  if (rc) return rc;
  const int sig_group = k.sig_group;
  if ((rc = check_common(sig_group, scheme, fmt))) return rc;
  if (n == 0) return 0;
  if (!idx || !sigs || !msg_offsets || !status) return fail(BLSGPU_E_ARG, "null argument");
  if (n >= ((size_t)1 << 32)) return fail(BLSGPU_E_ARG, "2^32 or more items in one call");
  CTX_ACQUIRE_ON(c, k.devidx);
  uint64_t total = 0;
  if (is_device_ptr(msg_offsets)) HIPCK(hipMemcpy(&total, msg_offsets + n, 8, hipMemcpyDeviceToHost));
  else total = msg_offsets[n];
  const item_keys_indexed keys = {k, idx, fmt};
  const size_t sgb = sig_size(sig_group, fmt) * n;
  rc = arena_reserve(c, keys.arena_bytes(n) + pad256(sgb) + pad256(total) + pad256(8 * (n + 1)) + pad256(4 * n) + 2 * pad256((size_t)WS_PAIRS_WORDS * 4 * n) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_sigs, *d_msgs, *d_offs;
  if ((rc = stage_in(c, sigs, sgb, &d_sigs))) return rc;
  if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
  if ((rc = stage_in(c, msg_offsets, 8 * (n + 1), &d_offs))) return rc;
  Carver mem{c};
  int32_t* d_status = mem.take<int32_t>(4 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIRS_WORDS * 4 * n);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n);
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  const uint8_t* d_keys;
  TabledG2 key;
  if ((rc = keys.stage(c, n, &d_keys, &key))) return rc;       // (run_verify_items reads keys and signatures with one format)
  rc = run_verify_items(c, sig_group, scheme == BLSGPU_SCHEME_AUG, d_keys, (const uint8_t*)d_sigs, fmt, (const uint8_t*)d_msgs, (const uint64_t*)d_offs, 0,
                        scheme_dst(sig_group, scheme), n, d_pairs, d_f, d_status, 0, key);
  if (rc) return rc;
  keys.fin(c, n, d_status);
  HIPCK(hipGetLastError());
  return status_out_and_sync(c, status, d_status, n);
}
API_CATCH

// The batched aggregate verify over a key set: pair i's key is the entry at position idx[i].  k_keyset_check with the call's
// set_offsets (per-set precedence, and with line tables the one word that says whether every named entry has rows),
// k_keyset_gather of the affine records in the caller's pair order (k_keyset_to_proj for RAW_PROJ signatures), then the body of
// blsgpu_aggregate_verify_batch on the gathered keys -- with line tables and signatures in G1 its line kernel is k_linesp_keyed,
// which reads a pair item's rows at cidx[src[i]] -- and k_keyset_fin_aux: the precedence over status AND aux.
struct agg_keys_indexed {
  const KeySet& k;
  const void* idx;
  const std::vector<uint64_t>& offs;
  size_t n_sets;
  int fmt;
  bool want_lines;           // a set with line tables, signatures in G1: the call may take the keyed line kernel
  size_t arena_bytes;
  mutable unsigned long long* d_pre = nullptr;
  static size_t bytes_for(const KeySet& k, size_t T, size_t n_sets, int fmt) {
    return 2 * pad256(4 * (T ? T : 1)) + pad256(8 * (n_sets + 1)) + pad256(8 * n_sets) + pad256(pk_size(k.sig_group, BLSGPU_FMT_RAW_AFFINE) * (T ? T : 1)) +
           pad256(pk_size(k.sig_group, fmt) * (T ? T : 1)) + 256;
  }
  size_t flat_bytes(size_t T_b) const { return want_lines ? pad256(4 * (T_b ? T_b : 1)) : 0; }
  int stage(Ctx* c, const uint8_t** kp, const uint32_t** key_table, const uint32_t** cidx) const {
    const size_t T = (size_t)offs[n_sets], asz = pk_size(k.sig_group, BLSGPU_FMT_RAW_AFFINE), ksz = pk_size(k.sig_group, fmt);
    int rc;
    const void* d_idx = nullptr;
    if (T && (rc = stage_in(c, idx, 4 * T, &d_idx))) return rc;
    const uint64_t* o;
    if ((rc = upload_offsets(c, offs, &o))) return rc;
    Carver mem{c};
    uint32_t* d_cidx = mem.take<uint32_t>(4 * (T ? T : 1));
    d_pre = mem.take<unsigned long long>(8 * n_sets);
    uint8_t* d_aff = mem.take<uint8_t>(asz * (T ? T : 1));
    uint8_t* d_keys = fmt == BLSGPU_FMT_RAW_AFFINE ? d_aff : mem.take<uint8_t>(ksz * (T ? T : 1));
    uint32_t* d_walk = want_lines && T ? mem.take<uint32_t>(4) : nullptr;
    if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
    if ((rc = keyset_check(c, k, (const uint32_t*)d_idx, T, o, n_sets, d_cidx, d_pre, d_walk))) return rc;
    if (d_walk && (rc = keyset_lines_decide(c, k, d_walk, key_table))) return rc;      // a named finite entry without rows: every item walks
    if (T) {
      keyset_gather_keys(c, k, d_cidx, T, d_aff, d_keys);
      HIPCK(hipGetLastError());
    }
    *kp = d_keys;
    *cidx = d_cidx;
    return 0;
  }
  int fin(Ctx* c, int32_t* d_status, uint64_t* d_aux) const {
    KL(KID_KEYSET_FIN, k_keyset_fin_aux, dim3(blocks_for(n_sets)), dim3(BLS_BLOCK), n_sets, (const unsigned long long*)d_pre, d_status, d_aux);
    HIPCK(hipGetLastError());
    return 0;
  }
};
int blsgpu_aggregate_verify_indexed_batch(int scheme, uint64_t keyset, const uint32_t* idx, const uint8_t* msgs, const uint64_t* msg_offsets,
                                          const uint64_t* set_offsets, size_t n_sets, const void* sigs, int fmt, int32_t* status, uint64_t* aux) try {
  KeySet k;
  int rc = set_find(keyset, k);
  if (rc) return rc;
  const int sig_group = k.sig_group;
  if ((rc = check_common(sig_group, scheme, fmt))) return rc;
  if (!set_offsets) return fail(BLSGPU_E_ARG, "null set_offsets");
  if (n_sets && (!sigs || !msg_offsets || !status)) return fail(BLSGPU_E_ARG, "null argument");
  std::vector<uint64_t> offs;
  if ((rc = read_offsets(set_offsets, n_sets, "set_offsets", offs))) return rc;
  const size_t T = (size_t)offs[n_sets];
  if (T >= ((size_t)1 << 32)) return fail(BLSGPU_E_ARG, "2^32 or more pairs in one call");
  if (T && !idx) return fail(BLSGPU_E_ARG, "null argument");
  if (n_sets == 0) return 0;
  CTX_ACQUIRE_ON(c, k.devidx);                 // on the key set's device, without sharding (one large set alone too: its keys are gathered here)
  uint64_t total = 0;
  if (is_device_ptr(msg_offsets)) HIPCK(hipMemcpy(&total, msg_offsets + T, 8, hipMemcpyDeviceToHost));
  else total = msg_offsets[T];
  if (total && !msgs) return fail(BLSGPU_E_ARG, "null argument");
  const agg_keys_indexed keys = {k, idx, offs, n_sets, fmt, k.lines != nullptr && sig_group == 1, agg_keys_indexed::bytes_for(k, T, n_sets, fmt)};
  return aggregate_batch_run(c, sig_group, scheme, keys, msgs, msg_offsets, total, offs, n_sets, sigs, fmt, status, aux);
}
API_CATCH

// The row builder (k_group_lines): the Miller-loop rows of m affine G2 points into d_table (SHARED_TABLE_WORDS per point; d_scratch as
// large, d_flags m + 1 words), and one word back to the host (word_back): *usable = every point has rows -- the identity and a point
// whose walk meets h = 0 have none.  One launch, one synchronisation.
static int build_rows(Ctx* c, size_t m, const uint8_t* d_aff, uint32_t* d_table, uint32_t* d_scratch, int32_t* d_flags, bool* usable) {
  HIPCK(hipMemsetAsync(d_flags + m, 0, 4, c->stream));
  KL(KID_GROUP_LINES, k_group_lines, dim3(blocks_for(2 * m)), dim3(BLS_BLOCK), m, d_aff, d_table, d_scratch, d_flags);
  uint32_t any = 1;
  const int rc = word_back(c, d_flags + m, &any);
  *usable = !rc && any == 0;
  return rc;
}

// ---- shared-message verify (verify_shared.cuh): Signature::verify for items that come in groups under one message each
// What a call needs beyond its inputs, statuses and pair / Fp12 workspaces, decided from its shape alone (never from a result).
struct shared_plan {
  bool aug = false;        // MessageAugmentation: nothing to share, the messages are copied out per item for run_verify_items
  bool table = false;      // Bls12381G2Impl on the lane-split path: one line table per group (k_group_lines, k_lines2s_shared)
  size_t table_bytes = 0, x_total = 0, ws_bytes = 0;
  std::vector<uint64_t> x_offs;   // aug: item j's message at [x_offs[j], x_offs[j + 1]) of the per-item buffer
};
static void shared_make_plan(shared_plan& p, int sg, int scheme, size_t n, size_t n_groups, const std::vector<uint64_t>& ioffs,
                             const std::vector<uint64_t>& moffs) {
  p.aug = scheme == BLSGPU_SCHEME_AUG;
  if (p.aug) {
    p.x_offs.resize(n + 1);
    uint64_t t = 0;
    for (size_t g = 0; g < n_groups; g++)
      for (uint64_t j = ioffs[g]; j < ioffs[g + 1]; j++) {
        p.x_offs[j] = t;
        t += moffs[g + 1] - moffs[g];
      }
    p.x_offs[n] = t;
    p.x_total = (size_t)t;
    p.ws_bytes = pad256(8 * (n + 1)) + pad256(p.x_total);
    return;
  }
  const size_t hb = point_bytes(sg, BLSGPU_FMT_RAW_PROJ) * n_groups, ab = point_bytes(sg, BLSGPU_FMT_RAW_AFFINE) * n_groups;
  p.ws_bytes = pad256(hb) + pad256(ab) + pad256(768 * n_groups);
  // The table form: the lane-split path with its two-kernel Miller loop, tables that a 32-bit byte offset reaches, and groups
  // large enough on average that a group's walk of H(m) is shared by enough items (BLSGPU_SHARED_LINES_MIN; 0: never; unset: the
  // measured rule above the knob table).
  p.table_bytes = n_groups * (size_t)SHARED_TABLE_WORDS * 4;
  const long knob = knobs().shared_lines_min;
  const bool wanted = knob < 0 ? n >= SHARED_LINES_AUTO_ITEMS && n / n_groups >= SHARED_LINES_AUTO_MIN : knob > 0 && n / n_groups >= (size_t)knob;
  p.table = sg == 2 && wanted && pair_path(n) == PATH_LANE_SPLIT && lane_split_chunked() && p.table_bytes <= 0xffffffffull;
  if (p.table) p.ws_bytes += 2 * pad256(p.table_bytes) + pad256(4 * (n_groups + 1)) + pad256(4 * n);
}
// statuses of the n items into d_status (device).  Launch sequence, Basic and ProofOfPossession: the groups' hashes
// (run_hash_group; Bls12381G1Impl: uncleared), k_group_affine, [k_group_lines and one word back to the host], k_prepare_shared,
// run_pairing2 (fixed_g2 = 2 for Bls12381G1Impl; two general pairs, or the groups' tables, for Bls12381G2Impl).
static int run_verify_shared_items(Ctx* c, int sg, int scheme, const shared_plan& p, size_t n, size_t n_groups, const uint8_t* d_pks, const uint8_t* d_sigs,
                                   int fmt, const uint64_t* d_ioffs, const uint8_t* d_msgs, const uint64_t* d_moffs, uint32_t* d_pairs, uint32_t* d_f,
                                   int32_t* d_status, const TabledG2& key = {}) {
  // key (Bls12381G1Impl over a registered set with line tables): passed on to run_pairing2 as PairTables::key, all three schemes
  int rc;
  const dst_arg dst = scheme_dst(sg, scheme);
  if (p.aug) {
    const uint64_t* d_xoffs;
    if ((rc = upload_offsets(c, p.x_offs, &d_xoffs))) return rc;
    uint8_t* d_xmsgs = (uint8_t*)arena_take(c, p.x_total ? p.x_total : 1);
    if (!d_xmsgs) return fail(BLSGPU_E_HIP, "internal: arena too small");
    if (p.x_total)
      KL(KID_PREPARE_SHARED, k_shared_expand, dim3(blocks_for(p.x_total)), dim3(BLS_BLOCK), p.x_total, d_xoffs, n, d_ioffs, n_groups, d_moffs, d_msgs, d_xmsgs);
    rc = run_verify_items(c, sg, 1, d_pks, d_sigs, fmt, d_xmsgs, d_xoffs, 0, dst, n, d_pairs, d_f, d_status, 0, key);
    if (rc) (void)hipStreamSynchronize(c->stream);      // the upload above reads p.x_offs
    return rc;
  }
  Carver mem{c};
  uint8_t* d_hash = mem.take<uint8_t>(point_bytes(sg, BLSGPU_FMT_RAW_PROJ) * n_groups);
  uint8_t* d_aff = mem.take<uint8_t>(point_bytes(sg, BLSGPU_FMT_RAW_AFFINE) * n_groups);
  uint32_t *d_table = nullptr, *d_scratch = nullptr, *d_group = nullptr;
  int32_t* d_flags = nullptr;
  if (p.table) {
    d_table = mem.take<uint32_t>(p.table_bytes);
    d_scratch = mem.take<uint32_t>(p.table_bytes);
    d_flags = mem.take<int32_t>(4 * (n_groups + 1));
    d_group = mem.take<uint32_t>(4 * n);
  }
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  if ((rc = run_hash_group(c, sg, n_groups, d_msgs, d_moffs, dst, d_hash, sg == 1))) return rc;
  with_group(sg, [&](auto G) {
    KL(KID_PREPARE_SHARED, k_group_affine<G()>, dim3(blocks_for(n_groups)), dim3(BLS_BLOCK), n_groups, (const uint8_t*)d_hash, d_aff);
  });
  bool table = p.table;
  if (table) {
    // a group whose point is the identity or whose walk meets h = 0 has no usable rows (never seen for a hash output): the
    // call then takes the general form for every item -- one word read back decides it before the records are written
    if ((rc = build_rows(c, n_groups, d_aff, d_table, d_scratch, d_flags, &table))) return rc;
  }
  with_group(sg, [&](auto G) {
    KL(KID_PREPARE_SHARED, k_prepare_shared<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, n_groups, d_ioffs, d_pks, d_sigs, fmt, (const uint8_t*)d_aff, d_pairs,
       d_status, table ? 1 : 0, table ? d_group : (uint32_t*)nullptr);
  });
  HIPCK(hipGetLastError());
  PairTables t = pairs_walked(sg == 1 ? 2 : 0);
  if (sg == 1) t.key = key;
  if (table) {               // (only on the lane-split path: shared_make_plan) the records carry the signature's pair first
    t.shared.rows = d_table;
    t.shared.of = d_group;
  }
  return run_pairing2(c, n, d_pairs, d_f, d_status, t);
}
// the offsets of a shared-message call, read and checked; n = the item count
static int shared_read_offsets(const uint64_t* item_offsets, const uint64_t* msg_offsets, size_t n_groups, std::vector<uint64_t>& ioffs,
                               std::vector<uint64_t>& moffs, size_t* n) {
  int rc;
  if ((rc = read_offsets(item_offsets, n_groups, "item_offsets", ioffs))) return rc;
  if ((rc = read_offsets(msg_offsets, n_groups, "msg_offsets", moffs))) return rc;
  if (ioffs[n_groups] >= ((uint64_t)1 << 32)) return fail(BLSGPU_E_ARG, "2^32 or more items in one call");
  *n = (size_t)ioffs[n_groups];
  return 0;
}

/* Signature::verify (reference src/signature.rs:130-138) for the items of n_groups groups, every item of a group under the
 * group's message: status[i] is what blsgpu_verify_batch gives for item i with that message.  Keys: item_keys_by_value, or over a
 * registered key set item_keys_indexed -- item i's key is the entry at position idx[i]: the provider's stage (k_keyset_check, every
 * item its own set, k_keyset_gather), the shared path above, k_keyset_fin -- the sequence and the status precedence of
 * blsgpu_verify_indexed_batch. */
extern "C++" {
template <class Keys>
static int verify_shared_run(const Keys& keys, int scheme, const void* sigs, const uint64_t* item_offsets, size_t n_groups, const uint8_t* msgs,
                             const uint64_t* msg_offsets, int fmt, int32_t* status) {
  const int sig_group = keys.sig_group();
  int rc = check_common(sig_group, scheme, fmt);
  if (rc) return rc;
  if (n_groups == 0) return 0;
  if (!item_offsets || !msg_offsets) return fail(BLSGPU_E_ARG, "null offsets");
  CTX_ACQUIRE_ON(c, keys.devidx());
  std::vector<uint64_t> ioffs, moffs;
  size_t n = 0;
  if ((rc = shared_read_offsets(item_offsets, msg_offsets, n_groups, ioffs, moffs, &n))) return rc;
  if (n == 0) return 0;
  const size_t total = (size_t)moffs[n_groups];
  if (keys.null() || !sigs || !status || (total && !msgs)) return fail(BLSGPU_E_ARG, "null argument");
  shared_plan plan;
  shared_make_plan(plan, sig_group, scheme, n, n_groups, ioffs, moffs);
  const size_t sgb = sig_size(sig_group, fmt) * n;
  if ((rc = arena_reserve(c, keys.arena_bytes(n) + pad256(sgb) + pad256(total) + 2 * pad256(8 * (n_groups + 1)) + pad256(4 * n) +
                                 2 * pad256((size_t)WS_PAIRS_WORDS * 4 * n) + plan.ws_bytes + 8192)))
    return rc;
  c->arena_off = 0;
  const void *d_sigs, *d_msgs;
  const uint64_t *d_ioffs, *d_moffs;
  if ((rc = stage_in(c, sigs, sgb, &d_sigs))) return rc;
  if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
  if ((rc = upload_offsets(c, ioffs, &d_ioffs)) || (rc = upload_offsets(c, moffs, &d_moffs))) return drain(c, rc);
  // from here on every way out drains: the uploads read ioffs / moffs
  Carver mem{c};
  int32_t* d_status = mem.take<int32_t>(4 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIRS_WORDS * 4 * n);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n);
  if (!mem.ok) return drain(c, fail(BLSGPU_E_HIP, "internal: arena too small"));
  const uint8_t* d_keys;
  TabledG2 key;
  if ((rc = keys.stage(c, n, &d_keys, &key))) return drain(c, rc);
  rc = run_verify_shared_items(c, sig_group, scheme, plan, n, n_groups, d_keys, (const uint8_t*)d_sigs, fmt, d_ioffs, (const uint8_t*)d_msgs, d_moffs, d_pairs, d_f,
                               d_status, key);
  if (rc) return drain(c, rc);
  if (keys.fin(c, n, d_status) && hipGetLastError() != hipSuccess) return drain(c, fail(BLSGPU_E_HIP, "k_keyset_fin launch failed"));
  return status_out_and_sync(c, status, d_status, n);
}
}  // extern "C++"
int blsgpu_verify_shared_batch(int sig_group, int scheme, const void* pks, const void* sigs, const uint64_t* item_offsets, size_t n_groups,
                               const uint8_t* msgs, const uint64_t* msg_offsets, int fmt, int32_t* status) try {
  const item_keys_by_value keys = {pks, sig_group, fmt};
  return verify_shared_run(keys, scheme, sigs, item_offsets, n_groups, msgs, msg_offsets, fmt, status);
}
API_CATCH
int blsgpu_verify_shared_indexed_batch(int scheme, uint64_t keyset, const uint32_t* idx, const void* sigs, const uint64_t* item_offsets, size_t n_groups,
                                       const uint8_t* msgs, const uint64_t* msg_offsets, int fmt, int32_t* status) try {
  KeySet k;
  int rc = set_find(keyset, k);
  if (rc) return rc;
  const item_keys_indexed keys = {k, idx, fmt};
  return verify_shared_run(keys, scheme, sigs, item_offsets, n_groups, msgs, msg_offsets, fmt, status);
}
API_CATCH

// ---- threshold signcryption (signcrypt.cuh): the decryption-share check, many ciphertexts per call
/* BlsSignCrypt::verify_share (reference src/traits/sign_crypt.rs:192-207; SignDecryptionShare::verify,
 * src/sign_decryption_share.rs:45-62) for every share of n_ct ciphertexts: W' = H(u.to_bytes() || v) once per CIPHERTEXT, then
 * one two-pair check (-W', share) (w, pk) per share on the stages of blsgpu_pairing2_check_batch.  Keys: item_keys_by_value (on the
 * calling thread's device), or item_keys_indexed: share i's public-key share at position idx[i] of a registered key set, every share
 * its own set (the status precedence of blsgpu_verify_indexed_batch), on the key set's device, without sharding.
 * Launch sequence: [indexed: k_keyset_check, k_keyset_gather], the message and hash stages (k_signcrypt_hash_prefix,
 * k_signcrypt_hash_copy, run_hash_group), [plan T2: k_signcrypt_ct_affine, k_group_lines over 2 n_ct points and one word back,
 * k_signcrypt_tab_of], k_signcrypt_share_pairs, [plan ROWS on the one-wave path: k_signcrypt_swap_pairs], run_pairing2,
 * k_signcrypt_share_status, [indexed: k_keyset_fin].  The plan comes from the call's shape and the set's flags alone:
 *   ROWS  Bls12381G1Impl over a set whose named entries have line rows, above BLSGPU_WIDE_MAX shares (the provider hands back rows): the
 *         pair (w, pk) reads the key's rows and only the share is walked -- k_pairing_coop_rows / k_lines2s_shared with the set's rows in
 *         the place of a message set's / the groups' table;
 *   T2    behind the indexed door only (Keys::indexed), Bls12381G2Impl above BLSGPU_WIDE_MAX shares with at least
 *         BLSGPU_SIGNCRYPT_LINES_MIN shares per ciphertext on average: the rows of -W' and w are built once per ciphertext and a share
 *         walks nothing (k_pairing_coop_tables2 / k_lines2s_tables2);
 *   else  two general pairs: all a by-value call ever launches. */
extern "C++" {
template <class Keys>
static int signcrypt_share_verify_run(const Keys& keys, int scheme, const void* us, const void* ws, const uint8_t* vs, const uint64_t* v_offsets, size_t n_ct,
                                      const void* shares, const uint64_t* share_offsets, int fmt, int32_t* status) {
  const int sig_group = keys.sig_group();
  int rc = check_common(sig_group, scheme, fmt);
  if (rc) return rc;
  if (!v_offsets || !share_offsets) return fail(BLSGPU_E_ARG, "null offsets");
  CTX_ACQUIRE_ON(c, keys.devidx());
  std::vector<uint64_t> voffs, soffs;
  if ((rc = read_offsets(v_offsets, n_ct, "v_offsets", voffs))) return rc;
  if ((rc = read_offsets(share_offsets, n_ct, "share_offsets", soffs))) return rc;
  const size_t n = (size_t)soffs[n_ct], total = (size_t)voffs[n_ct];
  if (n >= ((size_t)1 << 32)) return fail(BLSGPU_E_ARG, "too many shares in one call");
  if (n == 0) return 0;
  if (keys.null() || !us || !ws || !shares || !status || (total && !vs)) return fail(BLSGPU_E_ARG, "null argument");
  const size_t K = point_bytes(key_group(sig_group), BLSGPU_FMT_COMPRESSED), ub = pk_size(sig_group, fmt) * n_ct, wb = sig_size(sig_group, fmt) * n_ct,
               shb = pk_size(sig_group, fmt) * n, wtb = sig_size(sig_group, BLSGPU_FMT_RAW_PROJ) * n_ct, mtotal = total + K * n_ct;
  std::vector<uint64_t> moffs(n_ct + 1);
  for (size_t s = 0; s <= n_ct; s++) moffs[s] = voffs[s] + K * s;
  // plan T2, from the shape alone (the knob prices the 2 n_ct walks of the row builder against the two walks a share saves)
  const size_t t2_bytes = 2 * n_ct * (size_t)SHARED_TABLE_WORDS * 4;
  const long knob = knobs().signcrypt_lines_min;
  const bool t2_plan = Keys::indexed && sig_group == 2 && knob > 0 && n / n_ct >= (size_t)knob && pair_path_reads_rows(n) && t2_bytes <= 0xffffffffull;
  const size_t t2_ws = t2_plan ? pad256(2 * 192 * n_ct) + 2 * pad256(t2_bytes) + pad256(4 * (2 * n_ct + 1)) + pad256(8 * n) : 0;
  if ((rc = arena_reserve(c, keys.arena_bytes(n) + pad256(ub) + pad256(wb) + pad256(total) + pad256(shb) + 3 * pad256(8 * (n_ct + 1)) + pad256(mtotal) + pad256(wtb) +
                                 pad256(768 * n_ct) + pad256(4 * n) + 2 * pad256((size_t)WS_PAIRS_WORDS * 4 * n) + t2_ws + 8192)))
    return rc;
  c->arena_off = 0;
  const void *d_us, *d_ws, *d_vs, *d_sh;
  const uint64_t *d_voffs, *d_soffs, *d_moffs;
  if ((rc = stage_in(c, us, ub, &d_us))) return rc;
  if ((rc = stage_in(c, ws, wb, &d_ws))) return rc;
  if ((rc = stage_in(c, vs, total, &d_vs))) return rc;
  if ((rc = stage_in(c, shares, shb, &d_sh))) return rc;
  if ((rc = upload_offsets(c, voffs, &d_voffs)) || (rc = upload_offsets(c, soffs, &d_soffs)) || (rc = upload_offsets(c, moffs, &d_moffs))) return drain(c, rc);
  // from here on every way out drains: the uploads read voffs / soffs / moffs
  Carver mem{c};
  uint8_t* d_msgs = mem.take<uint8_t>(mtotal);
  uint8_t* d_wt = mem.take<uint8_t>(wtb);
  int32_t* d_status = mem.take<int32_t>(4 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIRS_WORDS * 4 * n);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n);
  uint8_t* d_caff = nullptr;
  uint32_t *d_table = nullptr, *d_scratch = nullptr, *d_tof = nullptr;
  int32_t* d_flags = nullptr;
  if (t2_plan) {
    d_caff = mem.take<uint8_t>(2 * 192 * n_ct);
    d_table = mem.take<uint32_t>(t2_bytes);
    d_scratch = mem.take<uint32_t>(t2_bytes);
    d_flags = mem.take<int32_t>(4 * (2 * n_ct + 1));
    d_tof = mem.take<uint32_t>(8 * n);
  }
  if (!mem.ok) return drain(c, fail(BLSGPU_E_HIP, "internal: arena too small"));
  const uint8_t* d_keys;
  TabledG2 key;                                    // plan ROWS: key.rows (a named finite entry without rows makes every share walk)
  if ((rc = keys.stage(c, n, &d_keys, &key))) return drain(c, rc);
  // the messages U.to_bytes() || V, one per ciphertext, and their hash: every share of a ciphertext pairs against the same W'
  with_group(sig_group, [&](auto G) {
    KL(KID_SIGNCRYPT_GATHER, k_signcrypt_hash_prefix<G()>, dim3(blocks_for(n_ct)), dim3(BLS_BLOCK), n_ct, (const uint8_t*)d_us, fmt, d_voffs, d_msgs);
  });
  if (total) KL(KID_SIGNCRYPT_GATHER, k_signcrypt_hash_copy, dim3(blocks_for(total)), dim3(BLS_BLOCK), total, n_ct, (const uint8_t*)d_vs, d_voffs, K, d_msgs);
  if ((rc = run_hash_group(c, sig_group, n_ct, d_msgs, d_moffs, scheme_dst(sig_group, scheme), d_wt))) return drain(c, rc);
  bool t2 = t2_plan;
  if (t2) {
    // a FINITE w or W' whose walk meets h = 0 has no usable rows: the call then takes the general form for every share -- one word
    // read back decides it.  (An identity w never raises it: k_signcrypt_ct_affine.)
    KL(KID_SIGNCRYPT_GATHER, k_signcrypt_ct_affine, dim3(blocks_for(n_ct)), dim3(BLS_BLOCK), n_ct, (const uint8_t*)d_ws, fmt, (const uint8_t*)d_wt, d_caff);
    if ((rc = build_rows(c, 2 * n_ct, d_caff, d_table, d_scratch, d_flags, &t2))) return drain(c, rc);
    if (t2) KL(KID_SIGNCRYPT_GATHER, k_signcrypt_tab_of, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, n_ct, d_soffs, d_tof, d_tof + n);
  }
  with_group(sig_group, [&](auto G) {
    KL(KID_SIGNCRYPT_GATHER, k_signcrypt_share_pairs<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, n_ct, d_soffs, (const uint8_t*)d_sh, d_keys,
       (const uint8_t*)d_ws, fmt, (const uint8_t*)d_wt, d_pairs, d_status);
  });
  PairTables t = pairs_walked(0);
  if (key.rows && pair_path(n) == PATH_LANE_SPLIT) {
    t.shared = key;           // the records as written: the share's pair first, the key's rows as the groups' table
  } else if (key.rows) {      // plan ROWS on the one-wave path: the key's pair first, its rows as a message set's
    KL(KID_SIGNCRYPT_GATHER, k_signcrypt_swap_pairs, dim3(blocks_for(n * (size_t)WS_PAIR1_WORDS)), dim3(BLS_BLOCK), n, d_pairs);
    t.msg = key;
  }
  if (t2) {
    t.both.rows = d_table;
    t.both.of = d_tof;
  }
  if ((rc = run_pairing2(c, n, d_pairs, d_f, d_status, t))) return drain(c, rc);
  KL(KID_SIGNCRYPT_GATHER, k_signcrypt_share_status, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, d_status);
  keys.fin(c, n, d_status);
  if (hipGetLastError() != hipSuccess) return drain(c, fail(BLSGPU_E_HIP, "a kernel of the share check failed to launch"));
  return status_out_and_sync(c, status, d_status, n);
}
}  // extern "C++"
int blsgpu_signcrypt_share_verify_batch(int sig_group, int scheme, const void* us, const void* ws, const uint8_t* vs, const uint64_t* v_offsets,
                                        size_t n_ct, const void* shares, const void* pk_shares, const uint64_t* share_offsets, int fmt,
                                        int32_t* status) try {
  const item_keys_by_value keys = {pk_shares, sig_group, fmt};
  return signcrypt_share_verify_run(keys, scheme, us, ws, vs, v_offsets, n_ct, shares, share_offsets, fmt, status);
}
API_CATCH
int blsgpu_signcrypt_share_verify_indexed_batch(int scheme, uint64_t keyset, const uint32_t* idx, const void* us, const void* ws, const uint8_t* vs,
                                                const uint64_t* v_offsets, size_t n_ct, const void* shares, const uint64_t* share_offsets, int fmt,
                                                int32_t* status) try {
  KeySet k;
  int rc = set_find(keyset, k);
  if (rc) return rc;
  const item_keys_indexed keys = {k, idx, fmt};
  return signcrypt_share_verify_run(keys, scheme, us, ws, vs, v_offsets, n_ct, shares, share_offsets, fmt, status);
}
API_CATCH

/* Self-test hook of k_pairing_coop_keyed (include/blsgpu.h): the records of blsgpu_debug_coop_pairing with fixed_g2 = 2, pair 0's G2
 * member being entry idx[i] of a set with line tables.  The kernel goes through run_pairing2's launcher (debug_pairing_coop): mode 1 the
 * verdict, mode 0 the export of the easy-part value. */
int blsgpu_debug_coop_pairing_keyed(int mode, uint64_t keyset, const uint32_t* idx, const int32_t* in, size_t n, int32_t* status, int32_t* out_f12) try {
  KeySet k;
  int rc = set_find(keyset, k);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!in || !idx || !status || mode < 0 || mode > 1 || n > 4096 || (mode == 0 && !out_f12) || is_device_ptr(in) || is_device_ptr(idx) || is_device_ptr(status) ||
      is_device_ptr(out_f12))
    return fail(BLSGPU_E_ARG, "bad argument");
  if (!k.lines || k.sig_group != 1) return fail(BLSGPU_E_ARG, "the key set has no line tables");
  for (size_t i = 0; i < n; i++)
    if ((uint64_t)idx[i] >= (uint64_t)k.n) return fail(BLSGPU_E_ARG, "index outside the key set");
  CTX_ACQUIRE_ON(c, k.devidx);
  if ((rc = arena_reserve(c, pad256((size_t)WS_PAIRS_WORDS * 4 * n) + 2 * pad256(4 * n) + pad256((size_t)WIDE_EASY_WORDS * 4 * n) + 4096))) return rc;
  c->arena_off = 0;
  DebugStaged s;
  if ((rc = debug_stage(c, in, WS_PAIRS_WORDS, n, status, &s, idx, n))) return rc;
  PairTables t = pairs_walked(2);
  t.key.rows = k.lines;
  t.key.of = s.of;
  return debug_pairing_coop(c, mode, t, s, n, status, out_f12);
}
API_CATCH

/* Self-test hook of the kernels that PRODUCE line values (include/blsgpu.h): each shipped line kernel, launched with the grid, row stride,
 * first / count, lines3 offset and pass order of run_pairing2 / the product paths, one chunk after another, on caller-supplied items in
 * the pair-workspace layout (word w = 14 * vector + limb of item i at ws[w * n + i]).  The line workspace is filled with the sentinel
 * byte before every chunk and the chunk's rows are read back whole before the next one: what a kernel did not write reads as the
 * sentinel, and *stray counts the words it wrote on lanes beyond the chunk's items, in pass 1's lines3 rows for a skipped item, or
 * behind the rows it owns. */
int blsgpu_debug_lines(int kernel, int variant, const int32_t* items, size_t n, const int32_t* status, size_t chunk, uint64_t keyset, const uint32_t* idx, size_t t_b,
                       int32_t* out, uint64_t* stray) try {
  if (!initialised()) return NOT_INIT();
  const bool keyed = kernel == BLSGPU_LINES_2S_KEYED || kernel == BLSGPU_LINES_P_KEYED;
  const bool two_pairs = kernel == BLSGPU_LINES_2S || kernel == BLSGPU_LINES_2S_KEYED || kernel == BLSGPU_LINES_MILLER2S;
  const bool fixed_arg = kernel == BLSGPU_LINES_2S || kernel == BLSGPU_LINES_MILLER2S;
  if (kernel < BLSGPU_LINES_2S || kernel > BLSGPU_LINES_MILLER2S || (fixed_arg && (variant < 0 || variant > 2)) || (kernel == BLSGPU_LINES_FIXED && variant != 1 && variant != 2))
    return fail(BLSGPU_E_ARG, "unknown kernel or variant");
  KeySet k;
  if (keyed) {
    int rc = set_find(keyset, k);
    if (rc) return rc;
    if (!k.lines || k.sig_group != 1) return fail(BLSGPU_E_ARG, "the key set has no line tables");
  }
  if (n == 0) return 0;
  if (!items || !status || !out || !stray || n > 4096 || (keyed && !idx) || is_device_ptr(items) || is_device_ptr(status) || is_device_ptr(out) || is_device_ptr(idx) ||
      (kernel == BLSGPU_LINES_P_KEYED && t_b > n))
    return fail(BLSGPU_E_ARG, "bad argument");
  if (keyed)
    for (size_t i = 0; i < n; i++)
      if ((kernel == BLSGPU_LINES_2S_KEYED || i < t_b) && (uint64_t)idx[i] >= (uint64_t)k.n) return fail(BLSGPU_E_ARG, "index outside the key set");
  CTX_ACQUIRE_ON(c, keyed ? k.devidx : t_devidx);
  const size_t rec = two_pairs ? WS_PAIRS_WORDS : WS_PAIRS_WORDS / 2, E = MILLER_ENTRIES;
  int rc = arena_reserve(c, pad256(rec * 4 * n) + 2 * pad256(4 * n) + pad256((size_t)WS_F_WORDS * 4 * n) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  DebugStaged s;
  if ((rc = debug_stage(c, items, rec, n, status, &s, keyed ? idx : nullptr, n))) return rc;
  const uint32_t *d_pairs = s.pairs, *d_idx = s.of;
  const int32_t* d_status = s.status;
  *stray = 0;
  if (kernel == BLSGPU_LINES_MILLER2S) {              // the one-kernel loop run_pairing2 falls back to
    uint32_t* d_f = (uint32_t*)arena_take(c, (size_t)WS_F_WORDS * 4 * n);
    if (!d_f) return fail(BLSGPU_E_HIP, "internal: arena too small");
    HIPCK(hipMemsetAsync(d_f, BLSGPU_DEBUG_COOP_SENTINEL & 0xff, (size_t)WS_F_WORDS * 4 * n, c->stream));
    KL(KID_MILLER2_V1, k_miller2s, dim3(blocks_for(2 * n)), dim3(BLS_BLOCK), n, d_pairs, d_status, d_f, variant);
    HIPCK(hipGetLastError());
    std::vector<uint32_t> f((size_t)WS_F_WORDS * n);
    HIPCK(hipMemcpyAsync(f.data(), d_f, f.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; i++)
      for (size_t w = 0; w < WS_F_WORDS; w++) out[i * WS_F_WORDS + w] = (int32_t)f[w * n + i];
    SYNC_FLUSH(c);
    return 0;
  }
  // the items a chunk covers (virtual items for the two-pass product form, which is one chunk: item v pairs with item v + half)
  const size_t half = (n + 1) / 2;
  const size_t total = kernel == BLSGPU_LINES_P12 ? half : kernel == BLSGPU_LINES_FIXED ? 1 : n;
  const bool one_chunk = kernel == BLSGPU_LINES_P12 || kernel == BLSGPU_LINES_FIXED;
  const bool five = kernel == BLSGPU_LINES_2S || kernel == BLSGPU_LINES_2S_KEYED || kernel == BLSGPU_LINES_P12;
  const bool two_pass = (kernel == BLSGPU_LINES_2S && variant == 0) || kernel == BLSGPU_LINES_P12;
  PairTables t = pairs_walked(kernel == BLSGPU_LINES_2S_KEYED ? 2 : variant);      // BLSGPU_LINES_2S: variant = fixed_g2 (0: two passes)
  if (kernel == BLSGPU_LINES_2S_KEYED) {
    t.key.rows = k.lines;
    t.key.of = d_idx;
  }
  return debug_line_chunks(c, total, one_chunk ? total : chunk, five ? LINE5_WORDS : LINE3_WORDS_H, two_pass, status, out, stray, [&](size_t first, size_t cnt, size_t lanes) {
    const dim3 grid((unsigned)(lanes_for(cnt) / BLS_BLOCK)), block(BLS_BLOCK);
    uint32_t* lines3 = c->lines_ws + E * LINE5_WORDS * lanes;
    switch (kernel) {
      case BLSGPU_LINES_2S:
      case BLSGPU_LINES_2S_KEYED:
        launch_lines2s(c, n, first, cnt, d_pairs, d_status, t, lanes);
        break;
      case BLSGPU_LINES_P1:
        KL(KID_LINESP, k_linesp, grid, block, cnt, cnt, n, d_pairs + first, d_status + first, c->lines_ws, c->lines_ws, lanes, (size_t)0, cnt, 1);
        break;
      case BLSGPU_LINES_P12:
        KL(KID_LINESP, k_linesp, grid, block, n, half, n, d_pairs, d_status, c->lines_ws, lines3, lanes, (size_t)0, cnt, 1);
        KL(KID_LINESP, k_linesp, grid, block, n, half, n, d_pairs, d_status, c->lines_ws, lines3, lanes, (size_t)0, cnt, 2);
        break;
      case BLSGPU_LINES_P4:
        KL(KID_LINESP4, k_linesp4, dim3(blocks_for(4 * cnt)), block, cnt, n, d_pairs + first, d_status + first, c->lines_ws, lanes);
        break;
      case BLSGPU_LINES_FIXED:
        KL(KID_TAIL, k_lines_fixed, dim3(1), block, n, d_pairs, d_status, c->lines_ws, lanes, variant);
        break;
      default:   // BLSGPU_LINES_P_KEYED
        KL(KID_LINESP_KEYED, k_linesp_keyed, grid, block, t_b, first, cnt, n, d_pairs, d_status, c->lines_ws, lanes, (const uint32_t*)k.lines, d_idx);
        break;
    }
  });
}
API_CATCH

/* Self-test hook of the two kernels that read BOTH pairs' rows from one table in global memory (include/blsgpu.h): the m affine G2
 * points become a table through the row builder (k_group_lines), and item i's pairs are (P0, entry t0[i]), (P1, entry t1[i]) -- the
 * records of blsgpu_debug_coop_pairing, whose Q members are not read.  Modes 0 and 1: k_pairing_coop_tables2 through run_pairing2's
 * launcher, with the easy-part export / the verdict, as blsgpu_debug_coop_pairing_keyed.  Mode 2: k_lines2s_tables2 chunk after chunk
 * through launch_lines2s, the line5 entries and *stray as BLSGPU_LINES_2S_KEYED of blsgpu_debug_lines (debug_line_chunks). */
int blsgpu_debug_tables2(int mode, const void* points, size_t m, const uint32_t* t0, const uint32_t* t1, const int32_t* in, size_t n, int32_t* status, size_t chunk,
                         int32_t* out, uint64_t* stray) try {
  if (!initialised()) return NOT_INIT();
  if (n == 0) return 0;
  if (!points || !t0 || !t1 || !in || !status || mode < 0 || mode > 2 || n > 4096 || m == 0 || m > 4096 || (mode != 1 && !out) || (mode == 2 && !stray) ||
      is_device_ptr(points) || is_device_ptr(t0) || is_device_ptr(t1) || is_device_ptr(in) || is_device_ptr(status) || is_device_ptr(out))
    return fail(BLSGPU_E_ARG, "bad argument");
  for (size_t i = 0; i < n; i++)
    if ((uint64_t)t0[i] >= (uint64_t)m || (uint64_t)t1[i] >= (uint64_t)m) return fail(BLSGPU_E_ARG, "index outside the table");
  CTX_ACQUIRE(c);
  const size_t rec = WS_PAIRS_WORDS, tb = m * (size_t)SHARED_TABLE_WORDS * 4;
  int rc = arena_reserve(c, pad256(192 * m) + 2 * pad256(tb) + pad256(4 * (m + 1)) + pad256(rec * 4 * n) + 2 * pad256(8 * n) + pad256((size_t)WIDE_EASY_WORDS * 4 * n) + 8192);
  if (rc) return rc;
  c->arena_off = 0;
  std::vector<uint32_t> tt(2 * n);
  for (size_t i = 0; i < n; i++) {
    tt[i] = t0[i];
    tt[n + i] = t1[i];
  }
  const void* d_pts;
  if ((rc = stage_in(c, points, 192 * m, &d_pts))) return rc;
  Carver mem{c};
  uint32_t* d_table = mem.take<uint32_t>(tb);
  uint32_t* d_scratch = mem.take<uint32_t>(tb);
  int32_t* d_flags = mem.take<int32_t>(4 * (m + 1));
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  bool usable = false;
  if ((rc = build_rows(c, m, (const uint8_t*)d_pts, d_table, d_scratch, d_flags, &usable))) return rc;
  if (!usable) return fail(BLSGPU_E_ARG, "a point has no usable rows");
  DebugStaged s;
  if ((rc = debug_stage(c, in, WS_PAIRS_WORDS, n, status, &s, tt.data(), 2 * n))) return rc;
  PairTables t;
  t.both.rows = d_table;
  t.both.of = s.of;
  if (mode != 2) return debug_pairing_coop(c, mode, t, s, n, status, out);
  // mode 2: the line kernel through the chunk loop and the stray count of blsgpu_debug_lines
  *stray = 0;
  return debug_line_chunks(c, n, chunk, LINE5_WORDS, false, status, out, stray,
                           [&](size_t first, size_t cnt, size_t lanes) { launch_lines2s(c, n, first, cnt, s.pairs, s.status, t, lanes); });
}
API_CATCH
// =========================================================================================================
// Registered message sets (msgset.cuh): a table of HASHED messages that stays on the device, groups named by positions in it
static int msgset_kind_check(int sig_group, int scheme) {
  if (sig_group != 1 && sig_group != 2) return fail(BLSGPU_E_ARG, "sig_group must be 1 (Bls12381G1Impl) or 2 (Bls12381G2Impl)");
  if (scheme != BLSGPU_SCHEME_BASIC && scheme != BLSGPU_SCHEME_POP)
    return fail(BLSGPU_E_ARG, "a message set is Basic or ProofOfPossession: MessageAugmentation hashes pk || m, so there is nothing to register");
  return 0;
}
static size_t msgset_rec_bytes(const MsgSet& m) { return point_bytes(m.sig_group, BLSGPU_FMT_RAW_AFFINE); }
// `count` messages become the entries h_pos[0 .. count) of m (positions the caller has checked), or -- h_pos == nullptr -- the entries
// [first, first + count): the hash under the set's DST (run_hash_group; Bls12381G1Impl: uncleared), k_msgset_seal, and for a set that
// has rows k_keyset_lines[_at] on those entries alone, through a scratch that lives for this call only and is allocated before
// anything is written.
static int msgset_apply(Ctx* c, const MsgSet& m, const uint32_t* h_pos, size_t first, const uint8_t* msgs, const uint64_t* msg_offsets, size_t count) {
  std::vector<uint64_t> moffs;
  int rc = read_offsets(msg_offsets, count, "msg_offsets", moffs);
  if (rc) return rc;
  const size_t total = (size_t)moffs[count], hsz = point_bytes(m.sig_group, BLSGPU_FMT_RAW_PROJ);
  if (total && !msgs) return fail(BLSGPU_E_ARG, "null argument");
  if ((rc = arena_reserve(c, pad256(total) + pad256(8 * (count + 1)) + pad256(hsz * count) + pad256(768 * count) + pad256(4 * count) + 4096))) return rc;
  c->arena_off = 0;
  DevBuf scratch;
  if (m.lines) HIPCK(hipMalloc(&scratch.p, set_lines_scratch_bytes(count)));
  const void* d_msgs;
  const uint64_t* d_moffs;
  if ((rc = stage_in(c, msgs, total, &d_msgs))) return rc;
  if ((rc = upload_offsets(c, moffs, &d_moffs))) return rc;
  Carver mem{c};
  uint8_t* d_hash = mem.take<uint8_t>(hsz * count);
  uint32_t* d_pos = h_pos ? mem.take<uint32_t>(4 * count) : nullptr;
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  // the ways out through drain(c, rc): the uploads read moffs / h_pos
  if (h_pos && hipMemcpyAsync(d_pos, h_pos, 4 * count, hipMemcpyHostToDevice, c->stream) != hipSuccess) return drain(c, fail(BLSGPU_E_HIP, "position upload failed"));
  if ((rc = run_hash_group(c, m.sig_group, count, (const uint8_t*)d_msgs, d_moffs, scheme_dst(m.sig_group, m.scheme), d_hash, m.sig_group == 1))) return drain(c, rc);
  with_group(m.sig_group, [&](auto G) {
    KL(KID_MSGSET_SEAL, k_msgset_seal<G()>, dim3(blocks_for(count)), dim3(BLS_BLOCK), count, (const uint8_t*)d_hash, (const uint32_t*)d_pos, first, m.aff);
  });
  if (m.lines) set_launch_lines(c, m, d_pos, first, count, scratch.p);
  if (hipGetLastError() != hipSuccess) return drain(c, fail(BLSGPU_E_HIP, "a message set kernel failed to launch"));
  SYNC_FLUSH(c);                      // before the scratch goes
  return 0;
}
// a new set around `m` (kind, flags, n set by the caller) in two steps: the records allocated; then, once the caller has filled them,
// the rows built and the handle issued.  A failure in between frees what the set holds (msgset_free).
static int msgset_create_begin(Ctx* c, MsgSet& m) {
  m.devidx = t_devidx;
  m.dev = c->dev;
  HIPCK(hipMalloc((void**)&m.aff, msgset_rec_bytes(m) * std::max<size_t>(m.n, 1)));
  m.bytes = set_bytes(m);
  return 0;
}
static int msgset_create_finish(Ctx* c, MsgSet& m, uint64_t* out_handle) {
  int rc;
  if (m.n && (m.flags & BLSGPU_MSGSET_LINES) && (rc = set_build_lines(c, m))) return rc;
  *out_handle = set_issue(m);
  return 0;
}
int blsgpu_msgset_create(int sig_group, int scheme, const uint8_t* msgs, const uint64_t* msg_offsets, size_t n, int flags, uint64_t* out_handle) try {
  if (!initialised()) return NOT_INIT();
  int rc = msgset_kind_check(sig_group, scheme);
  if (rc) return rc;
  if (!out_handle || (n && !msg_offsets)) return fail(BLSGPU_E_ARG, "null argument");
  if (flags & ~BLSGPU_MSGSET_LINES) return fail(BLSGPU_E_ARG, "unknown flag");
  if (n >= 0xffffffffull) return fail(BLSGPU_E_ARG, "more than 2^32 - 2 messages");
  *out_handle = 0;
  CTX_ACQUIRE(c);
  MsgSet m;
  m.sig_group = sig_group;
  m.scheme = scheme;
  m.flags = flags;
  m.n = n;
  if ((rc = msgset_create_begin(c, m)) || (n && (rc = msgset_apply(c, m, nullptr, 0, msgs, msg_offsets, n))) || (rc = msgset_create_finish(c, m, out_handle)))
    set_free(m);
  return rc;
}
API_CATCH

int blsgpu_msgset_destroy(uint64_t handle) try { return set_destroy<MsgSet>(handle); }
API_CATCH

int blsgpu_msgset_info(uint64_t handle, int* sig_group, int* scheme, uint64_t* n, int* has_lines, uint64_t* device_bytes) try {
  MsgSet m;
  int rc = set_find(handle, m);
  if (rc) return rc;
  if (sig_group) *sig_group = m.sig_group;
  if (scheme) *scheme = m.scheme;
  if (n) *n = m.n;
  if (has_lines) *has_lines = m.lines ? 1 : 0;
  if (device_bytes) *device_bytes = m.bytes;
  return 0;
}
API_CATCH

int blsgpu_msgset_update(uint64_t handle, const uint32_t* pos, const uint8_t* msgs, const uint64_t* msg_offsets, size_t count) try {
  MsgSet m;
  int rc = set_find(handle, m);
  if (rc) return rc;
  if (count == 0) return 0;
  if (!pos || !msg_offsets) return fail(BLSGPU_E_ARG, "null argument");
  if (count > m.n) return fail(BLSGPU_E_ARG, "more positions than the message set has entries");
  CTX_ACQUIRE_ON(c, m.devidx);
  std::vector<uint32_t> h_pos;
  if ((rc = set_read_checked_positions(m, pos, count, h_pos))) return rc;
  return msgset_apply(c, m, h_pos.data(), 0, msgs, msg_offsets, count);
}
API_CATCH

int blsgpu_msgset_append(uint64_t handle, const uint8_t* msgs, const uint64_t* msg_offsets, size_t count, uint64_t* out_first) try {
  MsgSet m;
  int rc = set_find(handle, m);
  if (rc) return rc;
  if (count && !msg_offsets) return fail(BLSGPU_E_ARG, "null argument");
  if (keyset_positions_check(nullptr, count, m.n) != KEYSET_POS_OK) return fail(BLSGPU_E_ARG, "more than 2^32 - 2 messages");
  if (out_first) *out_first = m.n;
  if (count == 0) return 0;
  CTX_ACQUIRE_ON(c, m.devidx);
  {  // the offsets are checked before anything moves
    std::vector<uint64_t> moffs;
    if ((rc = read_offsets(msg_offsets, count, "msg_offsets", moffs))) return rc;
    if (moffs[count] && !msgs) return fail(BLSGPU_E_ARG, "null argument");
  }
  const size_t n0 = m.n, n1 = m.n + count;
  if ((rc = set_grow_base(c, handle, m, n0, n1))) return rc;
  set_grow_or_drop_lines(c, handle, m, n0, n1);
  if ((rc = msgset_apply(c, m, nullptr, n0, msgs, msg_offsets, count))) return rc;
  return set_finish_append(c, handle, m, n1);
}
API_CATCH

/* Self-test hook (include/blsgpu.h): a set whose entries are the given RAW_AFFINE points instead of hash outputs. */
int blsgpu_debug_msgset_from_points(int sig_group, const void* points, size_t n, int flags, uint64_t* out_handle) try {
  if (!initialised()) return NOT_INIT();
  int rc = msgset_kind_check(sig_group, BLSGPU_SCHEME_BASIC);
  if (rc) return rc;
  if (!out_handle || (n && !points)) return fail(BLSGPU_E_ARG, "null argument");
  if (flags & ~BLSGPU_MSGSET_LINES) return fail(BLSGPU_E_ARG, "unknown flag");
  if (n >= 0xffffffffull) return fail(BLSGPU_E_ARG, "more than 2^32 - 2 points");
  *out_handle = 0;
  CTX_ACQUIRE(c);
  MsgSet m;
  m.sig_group = sig_group;
  m.scheme = BLSGPU_SCHEME_BASIC;
  m.flags = flags;
  m.n = n;
  if ((rc = msgset_create_begin(c, m))) return rc;
  if (n && hipMemcpy(m.aff, points, msgset_rec_bytes(m) * n, hipMemcpyDefault) != hipSuccess) {
    (void)hipGetLastError();
    set_free(m);
    return fail(BLSGPU_E_HIP, "the copy of the points failed");
  }
  if ((rc = msgset_create_finish(c, m, out_handle))) set_free(m);
  return rc;
}
API_CATCH

// a message set, and the key set that an indexed call names next to it: the same orientation, on the same device
static int msgset_keyset_find(uint64_t msgset, MsgSet& m, uint64_t keyset, KeySet& k) {
  int rc = set_find(msgset, m);
  if (rc || (rc = set_find(keyset, k))) return rc;
  if (k.sig_group != m.sig_group) return fail(BLSGPU_E_ARG, "the key set belongs to the other orientation");
  if (k.dev != m.dev || k.devidx != m.devidx) return fail(BLSGPU_E_ARG, "the key set and the message set live on different devices");
  return 0;
}
// ---- the verify calls over a message set; keys: item_keys_by_value or item_keys_indexed.  Launch sequence: k_msgset_check (every
// group's index; whether every named entry has rows, one word back to the host where the plan may read rows), k_keyset_gather (the
// groups' stored points), [indexed, the provider's stage: k_keyset_check, k_keyset_gather of the keys], k_prepare_shared,
// k_msgset_mark, run_pairing2, [indexed: k_keyset_fin, k_msgset_mark].  No hash kernel, no k_group_affine, no k_group_lines.
extern "C++" {
template <class Keys>
static int msgset_verify(const MsgSet& m, const Keys& keys, const uint32_t* msg_idx, const void* sigs, const uint64_t* item_offsets, size_t n_groups, int fmt,
                         int32_t* status) {
  const int sg = m.sig_group;
  int rc = check_common(sg, m.scheme, fmt);
  if (rc) return rc;
  if (n_groups == 0) return 0;
  if (!item_offsets) return fail(BLSGPU_E_ARG, "null offsets");
  CTX_ACQUIRE_ON(c, m.devidx);
  std::vector<uint64_t> ioffs;
  if ((rc = read_offsets(item_offsets, n_groups, "item_offsets", ioffs))) return rc;
  if (ioffs[n_groups] >= ((uint64_t)1 << 32)) return fail(BLSGPU_E_ARG, "2^32 or more items in one call");
  if (n_groups >= ((uint64_t)1 << 32)) return fail(BLSGPU_E_ARG, "2^32 or more groups in one call");
  const size_t n = (size_t)ioffs[n_groups];
  if (n == 0) return 0;
  if (!msg_idx || !sigs || !status || keys.null()) return fail(BLSGPU_E_ARG, "null argument");
  // the plan, from the call's shape alone: the row-wide engine reads no rows; the one-wave path reads them in k_pairing_coop_rows, the
  // lane-split path in k_lines2s_shared (BLSGPU_SHARED_LINES_MIN prices a build that has already happened: it does not apply)
  const bool rows_wanted = m.lines && sg == 2 && pair_path_reads_rows(n);
  const size_t asz = point_bytes(sg, BLSGPU_FMT_RAW_AFFINE), sgb = sig_size(sg, fmt) * n;
  if ((rc = arena_reserve(c, keys.arena_bytes(n) + 3 * pad256(4 * n) + pad256(sgb) + pad256(8 * (n_groups + 1)) + 2 * pad256(4 * n_groups) + pad256(asz * n_groups) +
                                 2 * pad256((size_t)WS_PAIRS_WORDS * 4 * n) + 256 + 8192)))
    return rc;
  c->arena_off = 0;
  const void *d_midx, *d_sigs;
  const uint64_t* d_ioffs;
  if ((rc = stage_in(c, msg_idx, 4 * n_groups, &d_midx))) return rc;
  if ((rc = stage_in(c, sigs, sgb, &d_sigs))) return rc;
  if ((rc = upload_offsets(c, ioffs, &d_ioffs))) return drain(c, rc);
  // from here on every way out drains: the upload reads ioffs
  Carver mem{c};
  uint32_t* d_cmsg = mem.take<uint32_t>(4 * n_groups);
  uint8_t* d_haff = mem.take<uint8_t>(asz * n_groups);
  uint32_t* d_group = mem.take<uint32_t>(4 * n);
  uint32_t* d_msg_of = mem.take<uint32_t>(4 * n);
  int32_t* d_status = mem.take<int32_t>(4 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIRS_WORDS * 4 * n);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n);
  uint32_t* d_mwalk = mem.take<uint32_t>(4);
  if (!mem.ok) return drain(c, fail(BLSGPU_E_HIP, "internal: arena too small"));
  if (hipMemsetAsync(d_mwalk, 0, 4, c->stream) != hipSuccess) return drain(c, fail(BLSGPU_E_HIP, "hipMemsetAsync failed"));
  KL(KID_MSGSET_CHECK, k_msgset_check, dim3(blocks_for(n_groups)), dim3(BLS_BLOCK), n_groups, (const uint32_t*)d_midx, (uint64_t)m.n,
     rows_wanted ? (const int32_t*)m.nolines : (const int32_t*)nullptr, d_cmsg, d_mwalk);
  const uint32_t* rows = nullptr;
  if (rows_wanted) {  // one plan per call: a named entry without usable rows makes every item walk
    uint32_t walk;
    if ((rc = word_back(c, d_mwalk, &walk))) return drain(c, rc);
    rows = walk == 0 ? m.lines : nullptr;
  }
  KL(KID_KEYSET_GATHER, k_keyset_gather, dim3(blocks_for(n_groups * (asz / 4))), dim3(BLS_BLOCK), n_groups, asz / 4, (const uint32_t*)d_cmsg, (const uint32_t*)m.aff,
     0, (uint32_t*)d_haff);
  PairTables t = pairs_walked(sg == 1 ? 2 : 0);
  const uint8_t* d_keys;
  if ((rc = keys.stage(c, n, &d_keys, &t.key))) return drain(c, rc);      // t.key: read with fixed_g2 = 2 only
  const bool split_rows = rows && pair_path(n) == PATH_LANE_SPLIT;        // the table form of the line kernel: the signature's pair first
  with_group(sg, [&](auto G) {
    KL(KID_PREPARE_SHARED, k_prepare_shared<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, n_groups, d_ioffs, d_keys, (const uint8_t*)d_sigs, fmt,
       (const uint8_t*)d_haff, d_pairs, d_status, split_rows ? 1 : 0, d_group);
  });
  KL(KID_MSGSET_CHECK, k_msgset_mark, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint32_t*)d_group, (const uint32_t*)d_cmsg, d_status, d_msg_of);
  if (hipGetLastError() != hipSuccess) return drain(c, fail(BLSGPU_E_HIP, "a message set kernel failed to launch"));
  if (rows) {
    TabledG2& role = split_rows ? t.shared : t.msg;
    role.rows = rows;
    role.of = d_msg_of;
  }
  if ((rc = run_pairing2(c, n, d_pairs, d_f, d_status, t))) return drain(c, rc);
  if (keys.fin(c, n, d_status)) {       // the message index's precedence once more, over what the key set had to say
    KL(KID_MSGSET_CHECK, k_msgset_mark, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint32_t*)d_group, (const uint32_t*)d_cmsg, d_status, (uint32_t*)nullptr);
    if (hipGetLastError() != hipSuccess) return drain(c, fail(BLSGPU_E_HIP, "k_keyset_fin launch failed"));
  }
  return status_out_and_sync(c, status, d_status, n);
}
}  // extern "C++"
int blsgpu_verify_msgset_batch(uint64_t msgset, const uint32_t* msg_idx, const void* pks, const void* sigs, const uint64_t* item_offsets, size_t n_groups, int fmt,
                               int32_t* status) try {
  MsgSet m;
  int rc = set_find(msgset, m);
  if (rc) return rc;
  const item_keys_by_value keys = {pks, m.sig_group, fmt};
  return msgset_verify(m, keys, msg_idx, sigs, item_offsets, n_groups, fmt, status);
}
API_CATCH
int blsgpu_verify_msgset_indexed_batch(uint64_t msgset, const uint32_t* msg_idx, uint64_t keyset, const uint32_t* idx, const void* sigs,
                                       const uint64_t* item_offsets, size_t n_groups, int fmt, int32_t* status) try {
  MsgSet m;
  KeySet k;
  int rc = msgset_keyset_find(msgset, m, keyset, k);
  if (rc) return rc;
  const item_keys_indexed keys = {k, idx, fmt};
  return msgset_verify(m, keys, msg_idx, sigs, item_offsets, n_groups, fmt, status);
}
API_CATCH

// ---- aggregate verify by message index (agg_msgset.cuh): the batched aggregate verify with pair i's message named as entry
// msg_idx[i] of a message set.  Every set runs through the segmented kernels (no message bytes exist for the single call's path).
// Launch sequence: [indexed: k_keyset_check, k_keyset_gather], k_aggm_check, k_aggm_insert, [Basic: k_dup_find_seg], k_aggm_reps,
// k_scan_*, k_aggm_number, k_aggm_offsets -- the class count C and the rows word come back to the host -- then, unless every class is
// a singleton (C == T): k_scan_* over the member counts, k_aggm_widen, k_aggm_scatter -- the member offsets come back for the strip
// plan -- k_aggm_sum, k_share_fold; then k_aggm_items and the stages of aggregate_batch_run over M = C + n_sets items: per round
// k_linesp_keyed for the class items when the message set's rows are usable (Bls12381G2Impl; the signature items, contiguous at the
// end of the list, always walk with k_linesp) or k_linesp for all, k_millerfp3; k_f12_fold_seg[_out], k_agg_batch_mark, k_aggm_mark,
// the final exponentiation, k_agg_batch_fin, [indexed: k_keyset_fin_aux], k_aggm_fin.  The rules take their inputs from the pairs
// (k_aggm_insert, k_dup_find_seg), never from the class items: k_first_bad_seg does not run here.
extern "C++" {
template <class Keys>
static int aggregate_msgset_run(Ctx* c, const MsgSet& m, const Keys& keys, const uint32_t* msg_idx, const std::vector<uint64_t>& offs, size_t n_sets,
                                const void* sigs, int fmt, int32_t* status, uint64_t* aux) {
  int rc;
  const int sg = m.sig_group;
  const size_t T = (size_t)offs[n_sets], Tz = T + 1, Mmax = T + n_sets;
  const bool basic = m.scheme == BLSGPU_SCHEME_BASIC, rows_wanted = m.lines != nullptr && sg == 2;
  const size_t ssz = sig_size(sg, fmt), osz = pk_size(sg, BLSGPU_FMT_RAW_PROJ);
  size_t cap = 64;
  while (cap < 2 * T) cap <<= 1;
  uint64_t tmax = 0;
  for (size_t s = 0; s < n_sets; s++) tmax = std::max(tmax, offs[s + 1] - offs[s]);
  const size_t round = 65536, fx_chunk = std::min(n_sets, miller_chunk_items() ? miller_chunk_items() : round);
  rc = arena_reserve(c, keys.arena_bytes + pad256(ssz * n_sets) + 2 * pad256(8 * (n_sets + 1)) + pad256(16 * n_sets) + 8 * pad256(4 * n_sets) +
                            14 * pad256(4 * Tz) + pad256(4 * scan_tiles(Tz)) + 2 * pad256(4 * cap) + 2 * pad256(8 * Tz) + pad256(osz * Tz) + pad256(4 * Mmax) +
                            pad256((size_t)WS_PAIR1_WORDS * 4 * Mmax) + pad256((size_t)WS_F_WORDS * 4 * Mmax) + pad256((size_t)WS_F_WORDS * 4 * n_sets) + 16384);
  if (rc) return rc;
  c->arena_off = 0;
  const void *d_sigs, *d_midx;
  const uint8_t* kp = nullptr;
  const uint32_t *key_table = nullptr, *d_cidx = nullptr;     // (a summed key has no line table: key sets' tables are not used here)
  const uint64_t* o;
  if ((rc = keys.stage(c, &kp, &key_table, &d_cidx))) return rc;
  if ((rc = stage_in(c, msg_idx, 4 * T, &d_midx))) return rc;
  if ((rc = stage_in(c, sigs, ssz * n_sets, &d_sigs))) return rc;
  if ((rc = upload_offsets(c, offs, &o))) return rc;
  Carver mem{c};
  int32_t* d_status = mem.stage_out<int32_t>(status, 4 * n_sets);
  uint64_t* d_aux = aux ? mem.stage_out<uint64_t>(aux, 16 * n_sets) : nullptr;
  uint32_t* d_cmsg = mem.take<uint32_t>(4 * Tz);
  uint32_t* d_sid = mem.take<uint32_t>(4 * Tz);
  uint32_t* d_slot = mem.take<uint32_t>(4 * Tz);
  uint32_t* d_isrep = mem.take<uint32_t>(4 * Tz);        // after the numbering: the member offsets as 32-bit words
  uint32_t* d_rank = mem.take<uint32_t>(4 * Tz);
  uint32_t* d_cid = mem.take<uint32_t>(4 * Tz);
  uint32_t* d_csid = mem.take<uint32_t>(4 * Tz);
  uint32_t* d_cent = mem.take<uint32_t>(4 * Tz);
  uint32_t* d_crep = mem.take<uint32_t>(4 * Tz);
  uint32_t* d_count = mem.take<uint32_t>(4 * Tz);
  uint32_t* d_cursor = mem.take<uint32_t>(4 * Tz);
  uint32_t* d_perm = mem.take<uint32_t>(4 * Tz);
  uint32_t* d_ssid = mem.take<uint32_t>(4 * Tz);
  uint32_t* d_tiles = mem.take<uint32_t>(4 * scan_tiles(Tz));
  uint32_t* d_tab = mem.take<uint32_t>(4 * cap);
  uint32_t* d_minidx = mem.take<uint32_t>(4 * cap);
  uint64_t* d_moffs = mem.take<uint64_t>(8 * Tz);
  uint64_t* d_so = mem.take<uint64_t>(8 * Tz);
  uint64_t* d_coffs = mem.take<uint64_t>(8 * (n_sets + 1));
  uint8_t* d_part = mem.take<uint8_t>(osz * Tz);
  uint32_t* d_skipped = mem.take<uint32_t>(4 * n_sets);
  uint32_t* d_first = mem.take<uint32_t>(4 * n_sets);
  uint32_t* d_best = mem.take<uint32_t>(4 * n_sets);
  uint32_t* d_sigid = mem.take<uint32_t>(4 * n_sets);
  int32_t* d_stb = mem.take<int32_t>(4 * n_sets);
  uint32_t* d_bset = mem.take<uint32_t>(4 * n_sets);
  uint32_t* d_walk = mem.take<uint32_t>(4);
  int32_t* d_bad = mem.take<int32_t>(4 * Mmax);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIR1_WORDS * 4 * Mmax);
  uint32_t* d_f = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * Mmax);
  uint32_t* d_rec = mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n_sets);
  uint32_t* h_back = (uint32_t*)hsmall_take(c, 8);
  if (!mem.ok || !h_back) return fail(BLSGPU_E_HIP, "internal: arena too small");
  std::vector<uint32_t> bset(n_sets);
  std::iota(bset.begin(), bset.end(), 0u);
  std::vector<uint64_t> hm, soffs;
  std::vector<uint32_t> ssid;
  // the ways out through drain(c, rc): the uploads read this frame's vectors
  HIPCK(hipMemcpyAsync(d_bset, bset.data(), 4 * n_sets, hipMemcpyHostToDevice, c->stream));
  HIPCK(hipMemsetAsync(d_skipped, 0, 4 * n_sets, c->stream));
  HIPCK(hipMemsetAsync(d_first, 0xff, 4 * n_sets, c->stream));
  HIPCK(hipMemsetAsync(d_best, 0xff, 4 * n_sets, c->stream));
  HIPCK(hipMemsetAsync(d_tab, 0xff, 4 * cap, c->stream));
  HIPCK(hipMemsetAsync(d_minidx, 0xff, 4 * cap, c->stream));
  HIPCK(hipMemsetAsync(d_isrep, 0, 4 * Tz, c->stream));
  HIPCK(hipMemsetAsync(d_count, 0, 4 * Tz, c->stream));
  HIPCK(hipMemsetAsync(d_cursor, 0, 4 * Tz, c->stream));
  HIPCK(hipMemsetAsync(d_walk, 0, 4, c->stream));
  const uint32_t* best = basic ? d_best : nullptr;
  // a., b. the pairs: entries, the class table, the rules
  if (T) {
    KL(KID_AGGM_CLASS, k_aggm_check, dim3(blocks_for(T)), dim3(BLS_BLOCK), T, n_sets, o, (const uint32_t*)d_midx, (uint64_t)m.n,
       rows_wanted ? (const int32_t*)m.nolines : (const int32_t*)nullptr, d_cmsg, d_sid, d_skipped, d_walk);
    with_group(sg, [&](auto G) {
      KL(KID_AGGM_CLASS, k_aggm_insert<G()>, dim3(blocks_for(T)), dim3(BLS_BLOCK), T, basic ? 1 : 0, (const uint32_t*)d_cmsg, (const uint32_t*)d_sid,
         (const uint32_t*)m.aff, (uint32_t)(cap - 1), d_tab, d_minidx, d_slot, kp, fmt, o, d_first);
    });
    if (basic)
      KL(KID_AGGM_CLASS, k_dup_find_seg, dim3(blocks_for(T)), dim3(BLS_BLOCK), T, (const uint32_t*)d_sid, o, (const uint32_t*)d_slot, (const uint32_t*)d_minidx, d_best);
    KL(KID_AGGM_CLASS, k_aggm_reps, dim3(blocks_for(Tz)), dim3(BLS_BLOCK), T, (const uint32_t*)d_slot, (const uint32_t*)d_tab, d_isrep);
  }
  // c. the classes numbered set after set
  if ((rc = run_scan_u32(c, KID_AGGM_CLASS, Tz, d_isrep, d_rank, d_tiles))) return drain(c, rc);
  if (T)
    KL(KID_AGGM_CLASS, k_aggm_number, dim3(blocks_for(T)), dim3(BLS_BLOCK), T, (const uint32_t*)d_slot, (const uint32_t*)d_tab, (const uint32_t*)d_rank,
       (const uint32_t*)d_sid, (const uint32_t*)d_cmsg, d_cid, d_csid, d_cent, d_crep, d_count);
  KL(KID_AGGM_CLASS, k_aggm_offsets, dim3(blocks_for(n_sets + 1)), dim3(BLS_BLOCK), n_sets, o, (const uint32_t*)d_rank, d_coffs);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h_back, d_rank + T, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipMemcpyAsync(h_back + 1, d_walk, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
    return drain(c, fail(BLSGPU_E_HIP, "the class kernels failed"));
  const size_t C = h_back[0], M = C + n_sets;
  const uint32_t* rows = rows_wanted && h_back[1] == 0 ? m.lines : nullptr;      // one plan per call: a named entry without usable rows makes every item walk
  if (C > T) return fail(BLSGPU_E_HIP, "internal: more classes than pairs");
  // c., d. members in class order and the class key sums -- unless every class is a singleton: then the pairs are the class items
  const bool merged = C < T;
  if (merged) {
    if ((rc = run_scan_u32(c, KID_AGGM_CLASS, C + 1, d_count, d_isrep, d_tiles))) return rc;
    KL(KID_AGGM_CLASS, k_aggm_widen, dim3(blocks_for(C + 1)), dim3(BLS_BLOCK), C + 1, (const uint32_t*)d_isrep, d_moffs);
    KL(KID_AGGM_CLASS, k_aggm_scatter, dim3(blocks_for(T)), dim3(BLS_BLOCK), T, (const uint32_t*)d_cid, (const uint64_t*)d_moffs, d_cursor, d_perm);
    hm.resize(C + 1);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(hm.data(), d_moffs, 8 * (C + 1), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (hm[0] != 0 || hm[C] != T) return fail(BLSGPU_E_HIP, "internal: the class member offsets do not cover the pairs");
    const uint64_t qmax = multi_strip_plan(hm.data(), C, multi_strip_len(T, accumulate_lanes(T), (uint64_t)knobs().multi_strip), soffs, ssid);
    const size_t Q = ssid.size();
    if (Q > T) return fail(BLSGPU_E_HIP, "internal: more strips than pairs");
    HIPCK(hipMemcpyAsync(d_so, soffs.data(), 8 * (C + 1), hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemcpyAsync(d_ssid, ssid.data(), 4 * Q, hipMemcpyHostToDevice, c->stream));
    with_group(key_group(sg), [&](auto G) {
      KL(KID_AGGM_SUM, k_aggm_sum<G()>, dim3(blocks_for(G() * Q)), dim3(BLS_BLOCK), Q, kp, fmt, (const uint32_t*)d_perm, (const uint64_t*)d_moffs,
         (const uint64_t*)d_so, (const uint32_t*)d_ssid, d_part);
      for (uint64_t step = 1; step < qmax; step <<= 1)
        KL(KID_SHARE_FOLD, k_share_fold<G()>, dim3(blocks_for(Q)), dim3(BLS_BLOCK), Q, step, (const uint64_t*)d_so, (const uint32_t*)d_ssid, d_part);
    });
  }
  // e. the flat list: class items, then one signature item per set
  with_group(sg, [&](auto G) {
    KL(KID_AGGM_ITEMS, k_aggm_items<G()>, dim3(blocks_for(M)), dim3(BLS_BLOCK), M, C, (const uint32_t*)d_csid, (const uint32_t*)d_cent, (const uint32_t*)d_crep,
       (const uint32_t*)d_skipped, (const uint32_t*)d_first, best, kp, fmt, merged ? (const uint8_t*)d_part : (const uint8_t*)nullptr, (const uint64_t*)d_so,
       (const uint8_t*)m.aff, (const uint8_t*)d_sigs, d_pairs, d_bad, d_sigid);
  });
  if (hipGetLastError() != hipSuccess) return drain(c, fail(BLSGPU_E_HIP, "a class kernel failed to launch"));
  // f., g. one Miller value per item in rounds of at most one machine round, as aggregate_batch_run forms them
  const size_t per_round = agg_round_size(M, round);
  const size_t lanes_round = row_stride(lanes_for(per_round)), lanes_fx = row_stride(lanes_for(fx_chunk));
  if (lines_reserve(c, std::max((size_t)MILLER_ENTRIES * LINE3_WORDS_H * 4 * lanes_round, (size_t)FX_STORE_WORDS * 4 * lanes_fx)))
    return drain(c, fail(BLSGPU_E_HIP, "no room for the line workspace"));
  for (size_t first = 0; first < M; first += per_round) {
    const size_t cnt = std::min(per_round, M - first), nlanes = lanes_for(cnt), lanes = row_stride(nlanes);
    const size_t cnt_rows = rows && first < C ? std::min(cnt, C - first) : 0, cnt_walk = cnt - cnt_rows, walk0 = first + cnt_rows;
    if (cnt_rows)         // both lines of every step from the entry's rows: lane pair j is flat item first + j
      KL(KID_LINESP_KEYED, k_linesp_keyed, dim3((unsigned)(lanes_for(cnt_rows) / BLS_BLOCK)), dim3(BLS_BLOCK), C, first, cnt_rows, M, (const uint32_t*)d_pairs,
         (const int32_t*)d_bad, c->lines_ws, lanes, rows, (const uint32_t*)d_cent);
    if (cnt_walk) {       // the walk, its lane pairs behind those of the row items (two words per row for each of them)
      uint32_t* lw = c->lines_ws + 2 * cnt_rows;
      KL(KID_LINESP, k_linesp, dim3((unsigned)(lanes_for(cnt_walk) / BLS_BLOCK)), dim3(BLS_BLOCK), cnt_walk, cnt_walk, M, (const uint32_t*)(d_pairs + walk0),
         (const int32_t*)(d_bad + walk0), lw, lw, lanes, (size_t)0, cnt_walk, 1);
    }
    KL(KID_MILLERFP, k_millerfp3, dim3((unsigned)(nlanes / BLS_BLOCK)), dim3(BLS_BLOCK), cnt, cnt, 1, (const int32_t*)(d_bad + first), (const uint32_t*)c->lines_ws,
       lanes, d_f + first, M, (size_t)0);
  }
  // every set's product over its class items (a set has at most as many classes as pairs), times the signature's value
  if (C)
    for (int r = 0, nr = agg_fold_rounds(std::min<uint64_t>(tmax, C)); r < nr; r++)
      KL(KID_AGG_SEG_FOLD, k_f12_fold_seg, dim3(blocks_for(C)), dim3(BLS_BLOCK), C, r, (const uint32_t*)d_csid, (const uint64_t*)d_coffs, d_f, M);
  KL(KID_AGG_SEG_FOLD, k_f12_fold_seg_out, dim3(blocks_for(n_sets)), dim3(BLS_BLOCK), n_sets, C, (const uint64_t*)d_coffs, (const uint32_t*)d_f, M, d_rec);
  // the rules (their inputs: the pairs), the final exponentiation of the sets they leave open, the precedence
  KL(KID_AGG_SEG_FIN, k_agg_batch_mark, dim3(blocks_for(n_sets)), dim3(BLS_BLOCK), n_sets, o, best, (const uint32_t*)d_slot, (const uint32_t*)d_minidx,
     (const uint32_t*)d_first, (const uint32_t*)d_sigid, d_stb);
  KL(KID_AGG_SEG_FIN, k_aggm_mark, dim3(blocks_for(n_sets)), dim3(BLS_BLOCK), n_sets, (const uint32_t*)d_skipped, d_stb);
  for (size_t first = 0; first < n_sets; first += fx_chunk)
    launch_finalexp_chunk(c, n_sets, first, std::min(fx_chunk, n_sets - first), d_rec, d_stb, knobs().finalexp_seg != 0);
  KL(KID_AGG_SEG_FIN, k_agg_batch_fin, dim3(blocks_for(n_sets)), dim3(BLS_BLOCK), n_sets, o, (const uint32_t*)d_bset, best, (const uint32_t*)d_slot,
     (const uint32_t*)d_minidx, (const uint32_t*)d_first, (const uint32_t*)d_sigid, (const int32_t*)d_stb, d_status, d_aux);
  if (hipGetLastError() != hipSuccess) return drain(c, fail(BLSGPU_E_HIP, "a kernel of the aggregate verify failed to launch"));
  if ((rc = keys.fin(c, d_status, d_aux))) return drain(c, rc);
  KL(KID_AGG_SEG_FIN, k_aggm_fin, dim3(blocks_for(n_sets)), dim3(BLS_BLOCK), n_sets, (const uint32_t*)d_skipped, d_status, d_aux);
  if (hipGetLastError() != hipSuccess) return drain(c, fail(BLSGPU_E_HIP, "k_aggm_fin failed to launch"));
  if (aux && (rc = stage_back(c, aux, d_aux, 16 * n_sets))) return drain(c, rc);
  return drain(c, status_out_and_sync(c, status, d_status, n_sets));
}
}  // extern "C++"
static int aggregate_msgset_entry(uint64_t msgset, const uint32_t* msg_idx, bool indexed, uint64_t keyset, const uint32_t* idx, const void* pks,
                                  const uint64_t* set_offsets, size_t n_sets, const void* sigs, int fmt, int32_t* status, uint64_t* aux) {
  MsgSet m;
  KeySet k;
  int rc = indexed ? msgset_keyset_find(msgset, m, keyset, k) : set_find(msgset, m);
  if (rc) return rc;
  const int sg = m.sig_group;
  if ((rc = check_common(sg, m.scheme, fmt))) return rc;
  if (!set_offsets) return fail(BLSGPU_E_ARG, "null set_offsets");
  if (n_sets && (!sigs || !status)) return fail(BLSGPU_E_ARG, "null argument");
  std::vector<uint64_t> offs;
  if ((rc = read_offsets(set_offsets, n_sets, "set_offsets", offs))) return rc;
  const size_t T = (size_t)offs[n_sets];
  if (T >= ((size_t)1 << 32)) return fail(BLSGPU_E_ARG, "2^32 or more pairs in one call");
  if (T && (!msg_idx || (indexed ? !idx : !pks))) return fail(BLSGPU_E_ARG, "null argument");
  if (n_sets == 0) return 0;
  CTX_ACQUIRE_ON(c, m.devidx);                 // on the message set's device, without sharding
  if (indexed) {
    const agg_keys_indexed keys = {k, idx, offs, n_sets, fmt, false, agg_keys_indexed::bytes_for(k, T, n_sets, fmt)};
    return aggregate_msgset_run(c, m, keys, msg_idx, offs, n_sets, sigs, fmt, status, aux);
  }
  const size_t psz = pk_size(sg, fmt);
  const agg_keys_by_value keys = {pks, psz * T, pad256(psz * T)};
  return aggregate_msgset_run(c, m, keys, msg_idx, offs, n_sets, sigs, fmt, status, aux);
}
int blsgpu_aggregate_verify_msgset_batch(uint64_t msgset, const uint32_t* msg_idx, const void* pks, const uint64_t* set_offsets, size_t n_sets, const void* sigs,
                                         int fmt, int32_t* status, uint64_t* aux) try {
  return aggregate_msgset_entry(msgset, msg_idx, false, 0, nullptr, pks, set_offsets, n_sets, sigs, fmt, status, aux);
}
API_CATCH
int blsgpu_aggregate_verify_msgset_indexed_batch(uint64_t msgset, const uint32_t* msg_idx, uint64_t keyset, const uint32_t* idx, const uint64_t* set_offsets,
                                                 size_t n_sets, const void* sigs, int fmt, int32_t* status, uint64_t* aux) try {
  return aggregate_msgset_entry(msgset, msg_idx, true, keyset, idx, nullptr, set_offsets, n_sets, sigs, fmt, status, aux);
}
API_CATCH

/* Self-test hook of k_pairing_coop_rows (include/blsgpu.h): the records of blsgpu_debug_coop_pairing with fixed_g2 = 0, pair 0's G2
 * member being entry msg_of[i] of a set with rows.  The kernel goes through run_pairing2's launcher (debug_pairing_coop): mode 1 the verdict,
 * mode 0 the export of the easy-part value. */
int blsgpu_debug_coop_pairing_rows(int mode, uint64_t msgset, const uint32_t* msg_of, const int32_t* in, size_t n, int32_t* status, int32_t* out_f12) try {
  MsgSet m;
  int rc = set_find(msgset, m);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!in || !msg_of || !status || mode < 0 || mode > 1 || n > 4096 || (mode == 0 && !out_f12) || is_device_ptr(in) || is_device_ptr(msg_of) ||
      is_device_ptr(status) || is_device_ptr(out_f12))
    return fail(BLSGPU_E_ARG, "bad argument");
  if (!m.lines || m.sig_group != 2) return fail(BLSGPU_E_ARG, "the message set has no rows");
  for (size_t i = 0; i < n; i++)
    if ((uint64_t)msg_of[i] >= (uint64_t)m.n) return fail(BLSGPU_E_ARG, "index outside the message set");
  CTX_ACQUIRE_ON(c, m.devidx);
  if ((rc = arena_reserve(c, pad256((size_t)WS_PAIRS_WORDS * 4 * n) + 2 * pad256(4 * n) + pad256((size_t)WIDE_EASY_WORDS * 4 * n) + 4096))) return rc;
  c->arena_off = 0;
  DebugStaged s;
  if ((rc = debug_stage(c, in, WS_PAIRS_WORDS, n, status, &s, msg_of, n))) return rc;
  PairTables t;
  t.msg.rows = m.lines;
  t.msg.of = s.of;
  return debug_pairing_coop(c, mode, t, s, n, status, out_f12);
}
API_CATCH

// =========================================================================================================
// Registered signature sets (sigset.cuh): a table of round SIGNATURES that stays on the device, items named by positions in it
static size_t sigset_rec_bytes(const SigSet& s) { return point_bytes(s.sig_group, BLSGPU_FMT_RAW_AFFINE); }
static int sigset_fmt_check(int fmt) {
  if (fmt != BLSGPU_FMT_RAW_PROJ && fmt != BLSGPU_FMT_RAW_AFFINE && fmt != BLSGPU_FMT_COMPRESSED && fmt != BLSGPU_FMT_LEGACY)
    return fail(BLSGPU_E_ARG, "fmt must be one of the four BLSGPU_FMT_* point formats");
  return 0;
}
// `count` signatures become the entries [first, first + count) of s, whose arrays have room for them: k_decompress on the wire formats
// (the creation status), k_sigset_seal, the tags, and for a set that has rows k_keyset_lines on those entries alone, through a
// scratch that lives for this call only and is allocated before anything is written.  status (may be null): the new entries' statuses.
static int sigset_apply(Ctx* c, const SigSet& s, size_t first, const void* sigs, const uint8_t* schemes, size_t count, int fmt, int32_t* status) {
  const bool wire = fmt == BLSGPU_FMT_COMPRESSED || fmt == BLSGPU_FMT_LEGACY;
  const size_t sb = point_bytes(s.sig_group, fmt) * count, raw = point_bytes(s.sig_group, BLSGPU_FMT_RAW_PROJ) * count;
  int rc = arena_reserve(c, pad256(sb) + pad256(count) + (wire ? pad256(raw) + pad256(4 * count) : 0) + 4096);
  if (rc) return rc;
  c->arena_off = 0;
  DevBuf scratch;
  if (s.lines) HIPCK(hipMalloc(&scratch.p, set_lines_scratch_bytes(count)));
  const void *d_sigs, *d_tags;
  if ((rc = stage_in(c, sigs, sb, &d_sigs))) return rc;
  if ((rc = stage_in(c, schemes, count, &d_tags))) return rc;
  Carver mem{c};
  uint8_t* d_raw = wire ? mem.take<uint8_t>(raw) : nullptr;
  int32_t* d_dec = wire ? mem.take<int32_t>(4 * count) : nullptr;
  if (!mem.ok) return fail(BLSGPU_E_HIP, "internal: arena too small");
  int kfmt = fmt;
  if (wire) {
    const int legacy = fmt == BLSGPU_FMT_LEGACY;
    with_group(s.sig_group, [&](auto G) {
      KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(count)), dim3(BLS_BLOCK), count, (const uint8_t*)d_sigs, legacy, d_raw, d_dec, 0);
    });
    d_sigs = d_raw;
    kfmt = BLSGPU_FMT_RAW_PROJ;
  }
  with_group(s.sig_group, [&](auto G) {
    KL(KID_SIGSET_SEAL, k_sigset_seal<G()>, dim3(blocks_for(count)), dim3(BLS_BLOCK), count, (const uint8_t*)d_sigs, kfmt, (const int32_t*)d_dec, first, s.aff, s.status);
  });
  HIPCK(hipMemcpyAsync(s.tags + first, d_tags, count, hipMemcpyDeviceToDevice, c->stream));
  if (s.lines) set_launch_lines(c, s, nullptr, first, count, scratch.p);
  HIPCK(hipGetLastError());
  if (status && (rc = copy_out(c, status, s.status + first, 4 * count))) return rc;
  SYNC_FLUSH(c);                      // before the scratch goes
  return 0;
}

int blsgpu_sigset_create(int sig_group, const void* sigs, const uint8_t* schemes, size_t n, int fmt, int flags, int32_t* status, uint64_t* out_handle) try {
  if (!initialised()) return NOT_INIT();
  if (sig_group != 1 && sig_group != 2) return fail(BLSGPU_E_ARG, "sig_group must be 1 (Bls12381G1Impl) or 2 (Bls12381G2Impl)");
  int rc = sigset_fmt_check(fmt);
  if (rc) return rc;
  if (!out_handle || (n && (!sigs || !schemes))) return fail(BLSGPU_E_ARG, "null argument");
  if (flags & ~BLSGPU_SIGSET_LINES) return fail(BLSGPU_E_ARG, "unknown flag");
  if (n >= 0xffffffffull) return fail(BLSGPU_E_ARG, "more than 2^32 - 2 signatures");
  *out_handle = 0;
  CTX_ACQUIRE(c);
  SigSet s;
  s.sig_group = sig_group;
  s.flags = flags;
  s.n = n;
  s.devidx = t_devidx;
  s.dev = c->dev;
  const size_t room = std::max<size_t>(n, 1);
  if (hipMalloc((void**)&s.aff, sigset_rec_bytes(s) * room) != hipSuccess || hipMalloc((void**)&s.tags, room) != hipSuccess ||
      hipMalloc((void**)&s.status, 4 * room) != hipSuccess) {
    (void)hipGetLastError();
    set_free(s);
    return fail(BLSGPU_E_HIP, "no device memory for the signature set");
  }
  s.bytes = set_bytes(s);
  if ((n && (rc = sigset_apply(c, s, 0, sigs, schemes, n, fmt, status))) || (n && (flags & BLSGPU_SIGSET_LINES) && (rc = set_build_lines(c, s)))) {
    set_free(s);
    return rc;
  }
  *out_handle = set_issue(s);
  return 0;
}
API_CATCH

int blsgpu_sigset_destroy(uint64_t handle) try { return set_destroy<SigSet>(handle); }
API_CATCH

int blsgpu_sigset_info(uint64_t handle, int* sig_group, uint64_t* n, int* has_lines, uint64_t* device_bytes) try {
  SigSet s;
  int rc = set_find(handle, s);
  if (rc) return rc;
  if (sig_group) *sig_group = s.sig_group;
  if (n) *n = s.n;
  if (has_lines) *has_lines = s.lines ? 1 : 0;
  if (device_bytes) *device_bytes = s.bytes;
  return 0;
}
API_CATCH

int blsgpu_sigset_append(uint64_t handle, const void* sigs, const uint8_t* schemes, size_t count, int fmt, int32_t* status, uint64_t* out_first) try {
  SigSet s;
  int rc = set_find(handle, s);
  if (rc) return rc;
  if ((rc = sigset_fmt_check(fmt))) return rc;
  if (count && (!sigs || !schemes)) return fail(BLSGPU_E_ARG, "null argument");
  if (keyset_positions_check(nullptr, count, s.n) != KEYSET_POS_OK) return fail(BLSGPU_E_ARG, "more than 2^32 - 2 signatures");
  if (out_first) *out_first = s.n;
  if (count == 0) return 0;
  CTX_ACQUIRE_ON(c, s.devidx);
  const size_t n0 = s.n, n1 = s.n + count;
  if ((rc = set_grow_base(c, handle, s, n0, n1))) return rc;
  set_grow_or_drop_lines(c, handle, s, n0, n1);
  if ((rc = sigset_apply(c, s, n0, sigs, schemes, count, fmt, status))) return rc;
  return set_finish_append(c, handle, s, n1);
}
API_CATCH

// ---- the two calls over a signature set.  Launch sequence: k_decompress of the callers' points (wire formats only), k_sigset_prepare
// (index check, statuses up to the identity checks, the pair made affine, the item's entry, and one word back to the host where the
// plan may read rows: whether any named entry lacks usable rows), run_pairing_values -- with the rows of a Bls12381G2Impl set whose
// named entries all have them, else walked --, and for the opening call k_timecrypt_open unchanged.  ct == false: blsgpu_pairing_sigset_batch.
static int sigset_run(uint64_t sigset, const uint32_t* idx, const void* us, bool ct, const uint8_t* vs, const uint8_t* ws, const uint64_t* w_offsets,
                      const uint8_t* ct_schemes, size_t n, int fmt, uint8_t* out_gt, uint8_t* frames, uint64_t* pt_range, int32_t* status) {
  SigSet s;
  int rc = set_find(sigset, s);
  if (rc) return rc;
  if ((rc = sigset_fmt_check(fmt))) return rc;
  if (n == 0) return 0;
  if (n >= ((uint64_t)1 << 32)) return fail(BLSGPU_E_ARG, "2^32 or more items in one call");
  CTX_ACQUIRE_ON(c, s.devidx);
  std::vector<uint64_t> woffs;
  size_t total = 0;
  if (ct) {
    if (!w_offsets) return fail(BLSGPU_E_ARG, "null w_offsets");
    if ((rc = read_offsets(w_offsets, n, "w_offsets", woffs))) return rc;
    total = (size_t)woffs[n];
    for (size_t i = 0; i < n; i++)
      if ((woffs[i + 1] - woffs[i]) >> 29) return fail(BLSGPU_E_ARG, "a w of 512 MiB or more");
    if (!vs || !ct_schemes || !pt_range || (total && (!ws || !frames))) return fail(BLSGPU_E_ARG, "null argument");
  } else if (!out_gt) {
    return fail(BLSGPU_E_ARG, "null argument");
  }
  if (!idx || !us || !status) return fail(BLSGPU_E_ARG, "null argument");
  const int sg = s.sig_group, pg = key_group(sg);
  const bool wire = fmt == BLSGPU_FMT_COMPRESSED || fmt == BLSGPU_FMT_LEGACY;
  const size_t ub = point_bytes(pg, fmt) * n, u_raw = point_bytes(pg, BLSGPU_FMT_RAW_PROJ) * n;
  size_t need = pad256(4 * n) + pad256(ub) + 4 * pad256(4 * n) + pad256((size_t)WS_PAIR1_WORDS * 4 * n) + pad256((size_t)GT_BYTES * n) + 512 + 8192;
  if (ct) need += pad256(32 * n) + 2 * pad256(total) + pad256(8 * (n + 1)) + pad256(n) + pad256(16 * n);
  if (wire) need += pad256(u_raw) + pad256(4 * n);
  const bool split = value_split_wanted(n);
  if (split) need += pad256((size_t)WS_F_WORDS * 4 * n);
  if ((rc = arena_reserve(c, need))) return rc;
  c->arena_off = 0;
  const void *d_idx, *d_us, *d_vs = nullptr, *d_ws = nullptr, *d_cs = nullptr;
  const uint64_t* d_woffs = nullptr;
  if ((rc = stage_in(c, idx, 4 * n, &d_idx))) return rc;
  if ((rc = stage_in(c, us, ub, &d_us))) return rc;
  // the ways out through drain(c, rc): the upload reads woffs
  if (ct) {
    if ((rc = stage_in(c, vs, 32 * n, &d_vs))) return rc;
    if ((rc = stage_in(c, ws, total, &d_ws))) return rc;
    if ((rc = stage_in(c, ct_schemes, n, &d_cs))) return rc;
    if ((rc = upload_offsets(c, woffs, &d_woffs))) return drain(c, rc);
  }
  Carver mem{c};
  uint8_t* d_frames = ct ? (total ? mem.stage_out<uint8_t>(frames, total) : c->arena) : nullptr;
  uint64_t* d_range = ct ? mem.stage_out<uint64_t>(pt_range, 16 * n) : nullptr;
  uint8_t* d_gt = ct ? mem.take<uint8_t>((size_t)GT_BYTES * n) : mem.stage_out<uint8_t>(out_gt, (size_t)GT_BYTES * n);
  int32_t* d_status = ct ? mem.take<int32_t>(4 * n) : mem.stage_out<int32_t>(status, 4 * n);
  int32_t* d_flag = mem.take<int32_t>(4 * n);
  uint32_t* d_ent = mem.take<uint32_t>(4 * n);
  uint32_t* d_pairs = mem.take<uint32_t>((size_t)WS_PAIR1_WORDS * 4 * n);
  uint32_t* d_walk = mem.take<uint32_t>(4);
  uint8_t* d_u_raw = wire ? mem.take<uint8_t>(u_raw) : nullptr;
  int32_t* d_dec_u = wire ? mem.take<int32_t>(4 * n) : nullptr;
  uint32_t* d_f = split ? mem.take<uint32_t>((size_t)WS_F_WORDS * 4 * n) : nullptr;
  if (!mem.ok) return drain(c, fail(BLSGPU_E_HIP, "internal: arena too small"));
  if (ct && total && d_frames != frames && hipMemsetAsync(d_frames, 0, total, c->stream) != hipSuccess)   // an item that is not opened hands back zeros
    return drain(c, fail(BLSGPU_E_HIP, "hipMemsetAsync failed"));
  if (hipMemsetAsync(d_walk, 0, 4, c->stream) != hipSuccess) return drain(c, fail(BLSGPU_E_HIP, "hipMemsetAsync failed"));
  int kfmt = fmt;
  if (wire) {
    const int legacy = fmt == BLSGPU_FMT_LEGACY;
    with_group(pg, [&](auto G) { KL(KID_DECOMPRESS, k_decompress<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_us, legacy, d_u_raw, d_dec_u, 0); });
    d_us = d_u_raw;
    kfmt = BLSGPU_FMT_RAW_PROJ;
  }
  const bool rows_wanted = s.lines && sg == 2;
  with_group(sg, [&](auto G) {
    KL(KID_SIGSET_PREP, k_sigset_prepare<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint32_t*)d_idx, (uint64_t)s.n, (const uint8_t*)s.aff,
       (const uint8_t*)s.tags, (const int32_t*)s.status, rows_wanted ? (const int32_t*)s.nolines : (const int32_t*)nullptr, (const uint8_t*)d_us, kfmt,
       (const int32_t*)d_dec_u, (const uint8_t*)d_cs, d_pairs, d_flag, d_status, d_ent, d_walk);
  });
  const uint32_t* rows = nullptr;
  if (rows_wanted) {  // one plan per call: a named entry without usable rows makes every item walk
    uint32_t walk;
    if ((rc = word_back(c, d_walk, &walk))) return drain(c, rc);
    rows = walk == 0 ? s.lines : nullptr;
  }
  run_pairing_values(c, n, d_pairs, d_flag, d_gt, d_f, rows, d_ent, (size_t)s.n * SIGSET_ENTRY_LINE_BYTES);
  if (!ct) {
    if (hipGetLastError() != hipSuccess) return drain(c, fail(BLSGPU_E_HIP, "a pairing-value kernel failed to launch"));
    if ((rc = stage_back(c, out_gt, d_gt, (size_t)GT_BYTES * n))) return drain(c, rc);
    if ((rc = stage_back(c, status, d_status, 4 * n))) return drain(c, rc);
    SYNC_FLUSH(c);
    return 0;
  }
  with_group(sg, [&](auto G) {
    KL(KID_TIMECRYPT_OPEN, k_timecrypt_open<G()>, dim3(blocks_for(n)), dim3(BLS_BLOCK), n, (const uint8_t*)d_gt, (const uint8_t*)d_us, kfmt, (const uint8_t*)d_vs,
       (const uint8_t*)d_ws, d_woffs, d_frames, d_range, d_status);
  });
  if (hipGetLastError() != hipSuccess) return drain(c, fail(BLSGPU_E_HIP, "k_timecrypt_open failed to launch"));
  if (total && (rc = stage_back(c, frames, d_frames, total))) return drain(c, rc);
  if ((rc = stage_back(c, pt_range, d_range, 16 * n))) return drain(c, rc);
  return status_out_and_sync(c, status, d_status, n);
}

int blsgpu_pairing_sigset_batch(uint64_t sigset, const uint32_t* idx, const void* points, size_t n, int fmt, uint8_t* out_gt, int32_t* status) try {
  return sigset_run(sigset, idx, points, false, nullptr, nullptr, nullptr, nullptr, n, fmt, out_gt, nullptr, nullptr, status);
}
API_CATCH

int blsgpu_timecrypt_open_indexed_batch(uint64_t sigset, const uint32_t* idx, const void* us, const uint8_t* vs, const uint8_t* ws, const uint64_t* w_offsets,
                                        const uint8_t* ct_schemes, size_t n, int fmt, uint8_t* frames, uint64_t* pt_range, int32_t* status) try {
  return sigset_run(sigset, idx, us, true, vs, ws, w_offsets, ct_schemes, n, fmt, nullptr, frames, pt_range, status);
}
API_CATCH
}  // extern "C"
