// kernels_ut_firstbatch.hip -- the first-hit batch (MODE 5, gpuhash_first_below_batch) k_scan
// instances of the K+W-table layout (C2 = 1, J = 0) and the lane-table layout (C2 = 3).  Same flags
// as kernels_ut.hip (UTFLAGS); a TU of their own so that kernels_ut.o keeps its contents.
#include "scan_decl.h"
#include "scan_kernel.h"

GPUHASH_INSTANTIATE_SCAN(0, 1, false, 5);
GPUHASH_INSTANTIATE_SCAN(1, 3, false, 5);
