// kernels_plain_firstbatch.hip -- the first-hit batch (MODE 5, gpuhash_first_below_batch) k_scan
// instances of the plain layouts, J = 0..13.  Same flags as kernels_plain.hip (PLAINFLAGS); a TU of
// their own so that kernels_plain.o and the other modes' objects keep their contents.
#include "scan_decl.h"
#include "scan_kernel.h"

#define PLAIN_FIRSTBATCH(J) GPUHASH_INSTANTIATE_SCAN(J, 0, false, 5)
PLAIN_FIRSTBATCH(0);
PLAIN_FIRSTBATCH(1);
PLAIN_FIRSTBATCH(2);
PLAIN_FIRSTBATCH(3);
PLAIN_FIRSTBATCH(4);
PLAIN_FIRSTBATCH(5);
PLAIN_FIRSTBATCH(6);
PLAIN_FIRSTBATCH(7);
PLAIN_FIRSTBATCH(8);
PLAIN_FIRSTBATCH(9);
PLAIN_FIRSTBATCH(10);
PLAIN_FIRSTBATCH(11);
PLAIN_FIRSTBATCH(12);
PLAIN_FIRSTBATCH(13);
