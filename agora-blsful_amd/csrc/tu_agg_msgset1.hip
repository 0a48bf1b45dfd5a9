// translation unit: aggregate verify by message index (agg_msgset.cuh) -- the group-independent kernels and Bls12381G1Impl
#define BLS_TU_AGG_MSGSET 1
#include "tu_agg_msgset.inc"
