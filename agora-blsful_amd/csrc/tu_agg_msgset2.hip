// translation unit: aggregate verify by message index (agg_msgset.cuh) -- Bls12381G2Impl
#define BLS_TU_AGG_MSGSET 2
#include "tu_agg_msgset.inc"
