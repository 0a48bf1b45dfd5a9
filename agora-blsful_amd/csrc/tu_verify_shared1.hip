// translation unit: the shared-message verify kernels (verify_shared.cuh) -- Bls12381G1Impl and the group-independent kernel
#define BLS_TU_VERIFY_SHARED 1
#include "tu_verify_shared.inc"
