// kernels_plain_collect.hip -- the collecting (MODE 3, gpuhash_collect_below) k_scan
// instances of the plain layouts, J = 0..13.  Same flags as kernels_plain.hip (PLAINFLAGS); a
// TU of their own so that kernels_plain.o and kernels_plain_first.o keep their contents.
#include "scan_decl.h"
#include "scan_kernel.h"

#define PLAIN_COLLECT(J) GPUHASH_INSTANTIATE_SCAN(J, 0, false, 3)
PLAIN_COLLECT(0);
PLAIN_COLLECT(1);
PLAIN_COLLECT(2);
PLAIN_COLLECT(3);
PLAIN_COLLECT(4);
PLAIN_COLLECT(5);
PLAIN_COLLECT(6);
PLAIN_COLLECT(7);
PLAIN_COLLECT(8);
PLAIN_COLLECT(9);
PLAIN_COLLECT(10);
PLAIN_COLLECT(11);
PLAIN_COLLECT(12);
PLAIN_COLLECT(13);
