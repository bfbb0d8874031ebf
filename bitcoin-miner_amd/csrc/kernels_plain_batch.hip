// kernels_plain_batch.hip -- the batch (MODE 4, gpuhash_min_batch) k_scan instances of the
// plain layouts, J = 0..13.  Same flags as kernels_plain.hip (PLAINFLAGS); a TU of their own so
// that kernels_plain.o, kernels_plain_first.o and kernels_plain_collect.o keep their contents.
#include "scan_decl.h"
#include "scan_kernel.h"

#define PLAIN_BATCH(J) GPUHASH_INSTANTIATE_SCAN(J, 0, false, 4)
PLAIN_BATCH(0);
PLAIN_BATCH(1);
PLAIN_BATCH(2);
PLAIN_BATCH(3);
PLAIN_BATCH(4);
PLAIN_BATCH(5);
PLAIN_BATCH(6);
PLAIN_BATCH(7);
PLAIN_BATCH(8);
PLAIN_BATCH(9);
PLAIN_BATCH(10);
PLAIN_BATCH(11);
PLAIN_BATCH(12);
PLAIN_BATCH(13);
