// kernels_misc.hip -- k_scan instances of the classic straddling layout (C2 = 1, J = 1),
// the two-word uniform loop (C2 = 2) and the extra-padding-block layouts (EX, J = 13..15), for
// the mode group of this compile (scan_decl.h).
// Built with -mllvm -amdgpu-sched-strategy=max-ilp (Makefile): classic +2.6%, EX +0.7%,
// C2 = 2 -0.2% vs defaults; 8 waves/SIMD costs EX 3% (profiles/r01_variants.jsonl).
#include "scan_decl.h"
#include "scan_kernel.h"

#define GPUHASH_MISC_LAYOUTS(X) \
    X(1, 1, false) X(1, 2, false) X(13, 0, true) X(14, 0, true) X(15, 0, true)
GPUHASH_MISC_LAYOUTS(GPUHASH_INSTANTIATE_LAYOUT)
