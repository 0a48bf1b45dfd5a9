// translation unit: the batched multi verify kernels (multi_batch.cuh) -- G2 keys (Bls12381G1Impl): the strip sums, k_multi_out<1>
#define BLS_TU_MULTI_BATCH 2
#include "tu_multi_batch.inc"
