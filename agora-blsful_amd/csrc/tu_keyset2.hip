// translation unit: the registered key set kernels (keyset.cuh) -- G2 keys (Bls12381G1Impl)
#define BLS_TU_KEYSET 2
#include "tu_keyset.inc"
