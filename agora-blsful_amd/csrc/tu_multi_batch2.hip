// translation unit: the batched multi verify kernels (multi_batch.cuh) -- G2 keys (Bls12381G1Impl): the strip sums
#define BLS_TU_MULTI_BATCH 2
#include "tu_multi_batch.inc"
