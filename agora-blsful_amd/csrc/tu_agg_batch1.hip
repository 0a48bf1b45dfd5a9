// translation unit: the batched aggregate verify kernels (agg_batch.cuh) -- Bls12381G1Impl's prepare, the index kernels
#define BLS_TU_AGG_BATCH 1
#include "tu_agg_batch.inc"
