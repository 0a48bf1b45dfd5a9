// translation unit: the shared-message verify kernels (verify_shared.cuh) -- Bls12381G2Impl and its per-group line tables
#define BLS_TU_VERIFY_SHARED 2
#include "tu_verify_shared.inc"
