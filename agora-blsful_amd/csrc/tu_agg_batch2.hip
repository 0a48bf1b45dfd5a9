// translation unit: the batched aggregate verify kernels (agg_batch.cuh) -- Bls12381G2Impl's prepare, the segmented Fp12 product
#define BLS_TU_AGG_BATCH 2
#include "tu_agg_batch.inc"
