// translation unit: the batched verify_secure kernels (secure.cuh) -- the per-set signature and key records
#define BLS_TU_SECURE 2
#include "tu_secure.inc"
