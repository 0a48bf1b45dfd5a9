// translation unit: the threshold-recovery kernels (shares.cuh) -- the G2 instances
#define BLS_TU_SHARES 2
#include "tu_shares.inc"
