// translation unit: the ElGamal kernels (elgamal.cuh) -- key group G2 (Bls12381G1Impl)
#define BLS_TU_ELGAMAL 2
#include "tu_elgamal.inc"
