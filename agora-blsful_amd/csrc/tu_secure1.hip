// translation unit: the batched verify_secure kernels (secure.cuh) -- the segmented key sort, the stream digests, the coefficients
#define BLS_TU_SECURE 1
#include "tu_secure.inc"
