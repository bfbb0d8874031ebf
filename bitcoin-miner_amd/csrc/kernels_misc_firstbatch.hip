// kernels_misc_firstbatch.hip -- the first-hit batch (MODE 5, gpuhash_first_below_batch) k_scan
// instances of the classic straddling layout (C2 = 1, J = 1), the two-word uniform loop (C2 = 2)
// and the extra-padding-block layouts (EX, J = 13..15).  Same flags as kernels_misc.hip
// (MISCFLAGS); a TU of their own so that kernels_misc.o keeps its contents.
#include "scan_decl.h"
#include "scan_kernel.h"

GPUHASH_INSTANTIATE_SCAN(1, 1, false, 5);
GPUHASH_INSTANTIATE_SCAN(1, 2, false, 5);
GPUHASH_INSTANTIATE_SCAN(13, 0, true, 5);
GPUHASH_INSTANTIATE_SCAN(14, 0, true, 5);
GPUHASH_INSTANTIATE_SCAN(15, 0, true, 5);
