// translation unit: the threshold-signcryption kernels (signcrypt.cuh) -- Bls12381G2Impl
#define BLS_TU_SIGNCRYPT 2
#include "tu_signcrypt.inc"
