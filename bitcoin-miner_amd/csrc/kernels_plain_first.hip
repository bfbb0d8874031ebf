// kernels_plain_first.hip -- the first-hit (MODE 2, gpuhash_first_below) k_scan instances
// of the plain layouts, J = 0..13.  Same flags as kernels_plain.hip (PLAINFLAGS); a TU of
// their own so that kernels_plain.o keeps its contents.
#include "scan_decl.h"
#include "scan_kernel.h"

#define PLAIN_FIRST(J) GPUHASH_INSTANTIATE_SCAN(J, 0, false, 2)
PLAIN_FIRST(0);
PLAIN_FIRST(1);
PLAIN_FIRST(2);
PLAIN_FIRST(3);
PLAIN_FIRST(4);
PLAIN_FIRST(5);
PLAIN_FIRST(6);
PLAIN_FIRST(7);
PLAIN_FIRST(8);
PLAIN_FIRST(9);
PLAIN_FIRST(10);
PLAIN_FIRST(11);
PLAIN_FIRST(12);
PLAIN_FIRST(13);
