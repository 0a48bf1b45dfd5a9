// TEST-ONLY harness for tests/test_hostsim_signcrypt.py: compiles the signcryption headers (agora-blsful_amd/csrc/keccak.cuh,
// signcrypt.cuh) as plain host C++, so that the `-m "not gpu"` suite checks the SHAKE128 sponge, the keystream xor (word and byte
// paths, every alignment) and the frame parser without a GPU.  Never linked into libblsgpu.so.
#include <string.h>
#include "../../agora-blsful_amd/csrc/signcrypt.cuh"

extern "C" {
// out[0, len) = SHAKE128(g[0, glen)) xor v[0, len); glen = 48 or 96.  The caller chooses the alignment of out and v.
void hs_keystream_xor(uint8_t* out, const uint8_t* v, uint64_t len, const uint8_t* g, int glen) {
  if (glen == 48) signcrypt_keystream_xor<48>(out, v, len, g);
  else signcrypt_keystream_xor<96>(out, v, len, g);
}
// 1 and (*off, *plen) on success, 0 otherwise
int hs_parse_frame(const uint8_t* frame, uint64_t len, uint64_t* off, uint64_t* plen) {
  return signcrypt_parse_frame(frame, len, off, plen) ? 1 : 0;
}
// one permutation of a 200-byte state (little-endian words), in place
void hs_keccak_f1600(uint64_t* s) {
  keccak_state st;
  memcpy(st.s, s, 200);
  keccak_f1600(st);
  memcpy(s, st.s, 200);
}
}
