// Threshold signcryption, the decryption-share side (reference src/traits/sign_crypt.rs:101-150,192-207) for many ciphertexts at
// once: blsgpu_signcrypt_share_verify_batch and blsgpu_signcrypt_open_batch.  The per-item functions, shared by the kernels
// (tu_signcrypt.inc) and the host harness (tests/hostsim_signcrypt):
//   * signcrypt_keystream_xor: frame = SHAKE128(compressed G) xor v (compute_v, :139-150), one sponge per lane (keccak.cuh),
//     8-byte words where the addresses allow and bytes at the edges;
//   * signcrypt_parse_frame: the length prefix of the opened frame (decrypt, :122-136) -- the ONE place that knows the varint rule.
#pragma once
#include "keccak.cuh"

#define BLS_ERR_INVALID_DECRYPTION_SHARE 14   // BlsError::InvalidDecryptionShare (include/blsgpu.h)
#define BLS_ERR_BAD_FRAME 15                  // decrypt returned None: no length prefix, or a length beyond the frame
#ifndef BLS_ERR_VSSS
#define BLS_ERR_VSSS 13
#endif

typedef uint64_t __attribute__((may_alias, aligned(8))) signcrypt_u64;

// The frame is varint(len) || message || padding.  The varint is the unsigned encoding of the uint-zigzag crate as this library
// assumes it (include/blsgpu.h): seven value bits per byte, least significant group first, the top bit set on every byte but the
// last; `peek` looks at up to 19 bytes (the longest encoding of a u128) and fails when none of them terminates or the frame ends
// first; the value is taken modulo 2^64 (`as usize`).  Success iff len <= frame_len - overhead.
#define SIGNCRYPT_VARINT_MAX 19
// The two ways a frame has no message are told apart for the time-lock call (timecrypt.cuh), whose reference goes on with an EMPTY
// message when `peek` fails (src/traits/time_crypt.rs:89-102) and returns None only for a length beyond the frame.
#define SIGNCRYPT_FRAME_OK 0          // *pt_off, *pt_len are set
#define SIGNCRYPT_FRAME_NO_PREFIX 1   // `peek` fails: no byte of the first 19 (or of the frame) ends a varint
#define SIGNCRYPT_FRAME_BEYOND 2      // a length beyond the frame
KECCAK_FN int signcrypt_parse_frame_kind(const uint8_t* frame, uint64_t frame_len, uint64_t* pt_off, uint64_t* pt_len) {
  uint64_t value = 0;
  for (int i = 0; i < SIGNCRYPT_VARINT_MAX; i++) {
    if ((uint64_t)i >= frame_len) return SIGNCRYPT_FRAME_NO_PREFIX;
    const uint8_t b = frame[i];
    if (7 * i < 64) value |= (uint64_t)(b & 0x7f) << (7 * i);
    if (!(b & 0x80)) {
      const uint64_t overhead = (uint64_t)i + 1;
      if (value > frame_len - overhead) return SIGNCRYPT_FRAME_BEYOND;
      *pt_off = overhead;
      *pt_len = value;
      return SIGNCRYPT_FRAME_OK;
    }
  }
  return SIGNCRYPT_FRAME_NO_PREFIX;
}
KECCAK_FN bool signcrypt_parse_frame(const uint8_t* frame, uint64_t frame_len, uint64_t* pt_off, uint64_t* pt_len) {
  return signcrypt_parse_frame_kind(frame, frame_len, pt_off, pt_len) == SIGNCRYPT_FRAME_OK;
}

// frame[0, len) = SHAKE128(g[0, GLEN)) xor v[0, len).  A long frame is a sequential squeeze: one permutation per 168 bytes.
// When frame and v are equally (mis)aligned, everything after the first 1 .. 8 bytes moves as aligned 8-byte words: memory word m
// holds keystream bytes a + 8 m .., the top 8 - a bytes of keystream word m and the low a bytes of word m + 1 (one funnel shift).
// Writes nothing outside frame[0, len).
template <int GLEN>
KECCAK_FN void signcrypt_keystream_xor(uint8_t* frame, const uint8_t* v, uint64_t len, const uint8_t* g) {
  if (len == 0) return;
  keccak_state st;
  shake128_absorb_short<GLEN>(st, g);
  const bool words = (((uintptr_t)frame ^ (uintptr_t)v) & 7) == 0;
  const int a = 8 - (int)((uintptr_t)frame & 7);         // 1 .. 8 head bytes
  uint64_t prev = 0;
  for (uint64_t base = 0;; base += SHAKE128_RATE) {
#pragma unroll
    for (int j = 0; j < SHAKE128_RATE_WORDS; j++) {
      const uint64_t cur = st.s[j];
      const uint64_t k0 = base + 8 * (uint64_t)j;         // keystream index of cur's first byte
      if (!words) {
        if (k0 < len) {
          for (int k = 0; k < 8; k++)
            if (k0 + k < len) frame[k0 + k] = v[k0 + k] ^ (uint8_t)(cur >> (8 * k));
        }
      } else if (k0 == 0) {
        for (int k = 0; k < 8; k++)
          if (k < a && (uint64_t)k < len) frame[k] = v[k] ^ (uint8_t)(cur >> (8 * k));
      } else {
        const uint64_t p = k0 - 8 + (uint64_t)a;          // frame offset of the aligned word that ends inside cur
        if (p < len) {
          const uint64_t ks = ((prev >> (8 * a - 1)) >> 1) | (cur << (64 - 8 * a));
          if (p + 8 <= len) {
            *(signcrypt_u64*)(frame + p) = *(const signcrypt_u64*)(v + p) ^ ks;
          } else {
            for (int k = 0; k < 8; k++)
              if (p + k < len) frame[p + k] = v[p + k] ^ (uint8_t)(ks >> (8 * k));
          }
        }
      }
      prev = cur;
    }
    if (base + SHAKE128_RATE - 8 + (uint64_t)(words ? a : 8) >= len) break;
    keccak_f1600(st);
  }
}

#if defined(__HIPCC__)
// n_ct ciphertexts: msgs[v_offs[c] + c K, ..) <- compressed u_c (K = 48 / 96 bytes, the public-key group of SG), the first half of
// the message U.to_bytes() || V of compute_w; k_signcrypt_hash_copy moves the v bytes behind it
template <int SG>
__global__ void k_signcrypt_hash_prefix(size_t n_ct, const uint8_t* us, int fmt, const uint64_t* v_offs, uint8_t* msgs);
__global__ void k_signcrypt_hash_copy(size_t total, size_t n_ct, const uint8_t* vs, const uint64_t* v_offs, size_t K, uint8_t* msgs);
// share i of ciphertext c -> the two-pair record (-W'_c, share_i) (w_c, pk_i) in the layout run_pairing2 reads (G1 member first);
// status[i] = BLS_OK, or BLS_ERR_INVALID_DECRYPTION_SHARE when the share, its key share or w_c is the identity
template <int SG>
__global__ void k_signcrypt_share_pairs(size_t n, size_t n_ct, const uint64_t* share_offs, const uint8_t* shares, const uint8_t* pks,
                                        const uint8_t* ws, int fmt, const uint8_t* wt, uint32_t* pairs, int32_t* status);
// after the pairing stages: every verdict that is not OK becomes BLS_ERR_INVALID_DECRYPTION_SHARE (a device-side failure stays)
__global__ void k_signcrypt_share_status(size_t n, int32_t* status);
// one ciphertext per lane: frame = SHAKE128(gbytes[c]) xor v, the prefix parse, pt_range and the merged status (status holds the
// validity verdicts on entry).  share_offs == nullptr: a key per ciphertext, no share-count rule.
__global__ void k_signcrypt_keystream(size_t n_ct, const uint64_t* v_offs, const uint8_t* vs, const uint8_t* gbytes, int glen,
                                      const uint64_t* share_offs, uint8_t* frames, uint64_t* pt_range, int32_t* status);

// ---- blsgpu_signcrypt_share_verify_indexed_batch: the key shares are entries of a registered key set (tu_signcrypt_indexed.hip)
// Bls12381G2Impl's table plan.  Both G2 members of a share's check belong to its CIPHERTEXT, so their normalised rows are built once per
// ciphertext (verify_shared.cuh k_group_lines over 2 n_ct points) and a share walks nothing.  aff: 192-byte affine records, -W'_c at
// 2 c and w_c at 2 c + 1 (an identity w_c: -W'_c again -- its shares are decided before any row is read and must not look like an
// entry without rows)
__global__ void k_signcrypt_ct_affine(size_t n_ct, const uint8_t* ws, int fmt, const uint8_t* wt, uint8_t* aff);
// share i of ciphertext c reads the entries t0[i] = 2 c and t1[i] = 2 c + 1
__global__ void k_signcrypt_tab_of(size_t n, size_t n_ct, const uint64_t* share_offs, uint32_t* t0, uint32_t* t1);
// Bls12381G1Impl over a set with line rows, one-wave path: k_pairing_coop_rows takes its tabled pair FIRST, so the two pairs of every
// record trade places (the lane-split k_lines2s_shared takes it second, which is the order k_signcrypt_share_pairs writes)
__global__ void k_signcrypt_swap_pairs(size_t n, uint32_t* pairs);
// The Miller loop of two TABLED pairs whose rows both lie in `table` (68 rows of 4 FP_NL words per entry, the *_LINES_N layout): pair k
// of item i is (P_k, entry tk[i]); the records' Q members are not read.  One wave per item (tu_coop_tables2.hip; easy as in
// k_pairing_coop_keyed), and the lane-split line kernel whose line5 stream k_millerf2s consumes (tu_lines_tables2.hip).
__global__ void k_pairing_coop_tables2(size_t n, const uint32_t* pairs, int32_t* status, const uint32_t* table, const uint32_t* t0, const uint32_t* t1,
                                       uint32_t* easy);
__global__ void k_lines2s_tables2(size_t n, size_t first, size_t count, const uint32_t* pairs, const int32_t* status, uint32_t* lines, size_t lanes,
                                  const uint32_t* table, const uint32_t* t0, const uint32_t* t1);
#endif
