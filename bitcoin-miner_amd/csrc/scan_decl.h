// scan_decl.h -- the scan kernels' declarations for the dispatch TU (kernels.hip), and the
// instantiation macros of the three family sources, kernels_{plain,ut,misc}.hip.  Each names its
// layouts and is built with the code-generation options that family measured best with
// (tools/variant_bench.py).
// A family source states its layouts once and is compiled once per mode group, into a code
// object each (Makefile, MODE_GROUPS): MODE 0 and 1 of every layout without GPUHASH_MODE, MODE N
// alone with -DGPUHASH_MODE=N (2..6).  kernels.hip launches the kernels through these
// declarations only, so nothing is implicitly instantiated there.
#pragma once
#include <stdint.h>

#include "kernels.h"
#include "plan.h"

// k_scan's parameters, for its declaration, its definition (scan_kernel.h) and its instantiations
#define GPUHASH_SCAN_PARAMS                                                                          \
    const gpuhash::LaunchDesc* __restrict__ descs, const unsigned long long* __restrict__ offs,      \
        int ndesc, unsigned long long* __restrict__ work, unsigned int gmin, unsigned int gmax,      \
        unsigned long long* __restrict__ thresh, gpuhash::Cand* __restrict__ cands,                  \
        unsigned int* __restrict__ ncand, unsigned long long* __restrict__ dump,                     \
        unsigned long long dump_lo, const uint32_t* __restrict__ ktab

namespace gpuhash {

template <int J, int C2, bool EX, int MODE>
__global__ void k_scan(GPUHASH_SCAN_PARAMS);

__global__ void k_ktab(const LaunchDesc* __restrict__ desc, uint32_t* __restrict__ tab, uint32_t R);
__global__ void k_ptab(const LaunchDesc* __restrict__ descs, uint32_t* __restrict__ tab);

}  // namespace gpuhash

#define GPUHASH_INSTANTIATE_SCAN(J, C2, EX, MODE) \
    template __global__ void gpuhash::k_scan<J, C2, EX, MODE>(GPUHASH_SCAN_PARAMS);
// One layout of a family source's list, for the mode group this compile is for.
#ifdef GPUHASH_MODE
#define GPUHASH_INSTANTIATE_LAYOUT(J, C2, EX) GPUHASH_INSTANTIATE_SCAN(J, C2, EX, GPUHASH_MODE)
#else
#define GPUHASH_INSTANTIATE_LAYOUT(J, C2, EX) \
    GPUHASH_INSTANTIATE_SCAN(J, C2, EX, 0) GPUHASH_INSTANTIATE_SCAN(J, C2, EX, 1)
#endif
