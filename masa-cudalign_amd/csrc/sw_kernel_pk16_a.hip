// packed strip kernel, instantiation part 0 of 8 (see the end of sw_kernel_pk16.inc)
#define PK16_PART 0
#include "sw_kernel_pk16.inc"
