// translation unit: the ElGamal kernels (elgamal.cuh) -- key group G1 (Bls12381G2Impl)
#define BLS_TU_ELGAMAL 1
#include "tu_elgamal.inc"
