// edge-mode instantiations of the packed pruning kernels (strips of 256 / 512 / 1024 / 2048 rows)
#define PK16_PART 9
#include "sw_kernel_pk16.inc"
