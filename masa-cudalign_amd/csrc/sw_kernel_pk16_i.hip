// goal-mode instantiations of the packed pruning kernels (strips of 256 / 512 rows, batches of 256 / 1024 rows)
#define PK16_PART 8
#include "sw_kernel_pk16.inc"
