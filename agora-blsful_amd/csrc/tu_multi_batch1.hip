// translation unit: the batched multi verify kernels (multi_batch.cuh) -- G1 keys (Bls12381G2Impl): the strip sums
#define BLS_TU_MULTI_BATCH 1
#include "tu_multi_batch.inc"
