// packed strip kernel, instantiation part 2 of 8 (see the end of sw_kernel_pk16.inc)
#define PK16_PART 2
#include "sw_kernel_pk16.inc"
