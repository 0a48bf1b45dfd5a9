// tools/bench_pok_timestamp.py, leg (e): what a caller of blsgpu_sig_proof_verify_batch did before the challenge was derived on the
// device -- per proof, on one host thread: the commitment to affine form (one field inversion), its compressed encoding, HKDF-SHA-256
// over encoding || LE64(t), the reduction modulo r.  The arithmetic is the library's own portable field code compiled for the host
// (csrc/hkdf.cuh and below), not an assembly-tuned field library: read the figure as an upper bound of that order.
#include <string.h>
#include "../agora-blsful_amd/csrc/verify.cuh"
#include "../agora-blsful_amd/csrc/hkdf.cuh"

extern "C" void pok_host_derive(int sg, const uint32_t* pts, const uint64_t* ts, size_t n, uint8_t* out) {
  uint8_t in[96 + 8];
  for (size_t i = 0; i < n; i++) {
    const uint32_t* p = pts + (size_t)36 * sg * i;
    const int nb = 48 * sg;
    if (sg == 1) {
      g1_jac a;
      g1_aff f;
      fp_from_raw(a.x, p); fp_from_raw(a.y, p + 12); fp_from_raw(a.z, p + 24);
      jac_to_aff(f, a);
      g1_compress(in, f, false);
    } else {
      g2_jac a;
      g2_aff f;
      fp_from_raw(a.x.c0, p); fp_from_raw(a.x.c1, p + 12); fp_from_raw(a.y.c0, p + 24); fp_from_raw(a.y.c1, p + 36);
      fp_from_raw(a.z.c0, p + 48); fp_from_raw(a.z.c1, p + 60);
      jac_to_aff(f, a);
      g2_compress(in, f, false);
    }
    for (int k = 0; k < 8; k++) in[nb + k] = (uint8_t)(ts[i] >> (8 * k));
    hkdf_scalar(out + 32 * i, in, nb + 8, (const uint8_t*)POK_SALT, POK_SALT_LEN);
  }
}
