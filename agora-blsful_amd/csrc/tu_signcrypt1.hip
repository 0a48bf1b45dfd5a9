// translation unit: the threshold-signcryption kernels (signcrypt.cuh) -- Bls12381G1Impl and the group-independent kernels
#define BLS_TU_SIGNCRYPT 1
#include "tu_signcrypt.inc"
