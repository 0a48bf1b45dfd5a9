// translation unit: the registered message set kernels (msgset.cuh) -- Bls12381G2Impl
#define BLS_TU_MSGSET 2
#include "tu_msgset.inc"
