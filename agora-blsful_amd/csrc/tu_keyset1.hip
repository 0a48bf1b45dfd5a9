// translation unit: the registered key set kernels (keyset.cuh) -- the group-independent kernels and G1 keys (Bls12381G2Impl)
#define BLS_TU_KEYSET 1
#include "tu_keyset.inc"
