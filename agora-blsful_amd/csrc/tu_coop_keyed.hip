// translation unit: kernels of the BLS_TU_COOP_KEYED section of kernels.cuh
#define BLS_TU_COOP_KEYED 1
#include "kernels.cuh"
