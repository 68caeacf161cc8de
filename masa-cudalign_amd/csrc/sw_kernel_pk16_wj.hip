// wide-alphabet twin of sw_kernel_pk16_j.hip: the same instantiations with the equality scoring form (PK16_WIDE)
#define PK16_WIDE 1
#define PK16_PART 9
#include "sw_kernel_pk16.inc"
