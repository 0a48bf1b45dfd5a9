// translation unit: the registered message set kernels (msgset.cuh) -- the group-independent kernels and Bls12381G1Impl
#define BLS_TU_MSGSET 1
#include "tu_msgset.inc"
