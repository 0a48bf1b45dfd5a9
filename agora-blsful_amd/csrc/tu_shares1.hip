// translation unit: the threshold-recovery kernels (shares.cuh) -- the Lagrange coefficients and the G1 instances
#define BLS_TU_SHARES 1
#include "tu_shares.inc"
