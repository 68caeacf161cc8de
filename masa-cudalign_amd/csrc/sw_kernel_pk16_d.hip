// packed strip kernel, instantiation part 3 of 8 (see the end of sw_kernel_pk16.inc)
#define PK16_PART 3
#include "sw_kernel_pk16.inc"
