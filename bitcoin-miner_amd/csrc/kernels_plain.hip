// kernels_plain.hip -- k_scan instances of the plain layouts (C2 = 0, no extra block):
// loop word W_J of the only nonce-bearing block, J = 0..13, for the mode group of this compile
// (scan_decl.h).  Built with -DGPUHASH_WAVES_PER_EU=8 (Makefile): 8 waves/SIMD in 63 VGPRs
// without spills, +0.3% on config 2 and +4% on J = 2 over the unconstrained build
// (profiles/r01_variants.jsonl).
#include "scan_decl.h"
#include "scan_kernel.h"

#define GPUHASH_PLAIN_LAYOUTS(X) \
    X(0, 0, false) X(1, 0, false) X(2, 0, false) X(3, 0, false) X(4, 0, false) X(5, 0, false)   \
    X(6, 0, false) X(7, 0, false) X(8, 0, false) X(9, 0, false) X(10, 0, false) X(11, 0, false) \
    X(12, 0, false) X(13, 0, false)
GPUHASH_PLAIN_LAYOUTS(GPUHASH_INSTANTIATE_LAYOUT)
