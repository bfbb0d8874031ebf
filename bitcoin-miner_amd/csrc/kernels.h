// kernels.h -- host-side entry points of kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "plan.h"

namespace gpuhash {

// One search candidate: a (hash, nonce) key, compared lexicographically.
struct Cand {
    unsigned long long hash;
    unsigned long long nonce;
};

// The arguments of one scan launch.  thresh, cands, ncand and dump_lo mean different things per
// mode; how the host sets them is stated once, at kWiring in gpuhash.cpp, and how the kernels
// read them in scan_kernel.h.
struct ScanArgs {
    hipStream_t stream;
    const LaunchDesc* descs;         // device: the group's launch descriptors
    const unsigned long long* offs;  // device: ndesc+1 prefix offsets in row-iterations
    int ndesc;
    unsigned long long* work;        // device: guided-scheduling counter (zeroed per launch),
                                     // followed by 4 clock words the kernel fills: s_memtime /
                                     // s_memrealtime of workgroup 0 at its start and its end
    unsigned int gmin, gmax;         // piece size bounds (r values per grab; stage.h)
    unsigned long long* thresh;      // the shared 64-bit word: a bound or the hit counter
                                     // (batch: one pruning word per job; first-hit batch: a
                                     // bound and a target per job; collect batch: a hit
                                     // counter, a target and a list flag per job)
    Cand* cands;                     // appended candidates, or the hit list (batch: the result
                                     // list, BatchEntry)
    unsigned int* ncand;             // append counter, or the hit list's capacity
    unsigned long long* dump;        // MODE 1 only: per-nonce hashes
    unsigned long long dump_lo;      // nonce of dump[0], or the target
    const uint32_t* ktab;            // C2/J=0 only: per-r K+W tables (see LaunchDesc::tab_off)
    unsigned int grid;               // workgroups (<= resident capacity, see grid_for)
};

// The scan kernels' MODE template parameter (scan_kernel.h), by name on the host.
enum ScanMode : int {
    kScanMin = 0, kScanDump = 1, kScanFirst = 2, kScanCollect = 3, kScanBatch = 4, kScanFirstBatch = 5,
    kScanCollectBatch = 6
};

// Resident workgroups of 256 threads for the (J, C2, EX, mode) kernel on this device.
unsigned int grid_for(int J, int C2, int EX, int mode, int device);

// One persistent launch of the (J, C2, EX) variant over a.descs[0..ndesc).  mode 0: argmin
// search, 1: per-nonce dump, 2: first hit at or below a target (gpuhash_first_below), 3: every
// hit at or below a target, counted and listed (gpuhash_collect_below), 4: the argmin search of
// every job of a batch (gpuhash_min_batch), 5: the first hit of every job of a batch
// (gpuhash_first_below_batch), 6: every hit of every job of a batch, counted per job and listed
// (gpuhash_collect_below_batch).
hipError_t launch_scan(int J, int C2, int EX, int mode, const ScanArgs& a);
// Fills the uniform K+W table of a C2/J=0 descriptor: tab[64*r + t] = K[t] + W_t(r),
// r in [0, D.R), for block B's words U with the loop digits of r inserted into W_0.
hipError_t launch_ktab(const LaunchDesc* d_desc, uint32_t* tab, uint32_t R, hipStream_t stream);
// Fills the p-tables of ndesc lane-table (C2 = 3) descriptors: for descriptor i and k < R,
// tab[desc.tab_off + 16k ...] = block B-1's chaining value for p = lt_p0 + k, then round 0's
// partial sums inv0, t20 of block B (scan_row_lt).
hipError_t launch_ptab(const LaunchDesc* d_descs, int ndesc, uint32_t* tab, hipStream_t stream);
hipError_t launch_reduce(Cand* cands, unsigned int* ncand, Cand* best, hipStream_t stream);

// The packed group of a batch stage (stage.h, C2 = 4; pack_kernel.hip): one persistent launch of
// k_pack over the group's tiles.  thresh, list and head are the batch stage's per-job words,
// result list and list head, as kScanBatch / kScanCollectBatch wire them (gpuhash.cpp, kWiring).
struct PackArgs {
    hipStream_t stream;
    const void* recs;                // device: the packed jobs' records (pack.h, PackJob)
    const void* segs;                // device: the segments, by class (PackSeg)
    const void* tiles;               // device: the tiles (PackTile)
    unsigned long long ntiles;       // the group's total
    unsigned long long* work;        // device: the group's counter block, as ScanArgs::work
    unsigned long long* thresh;
    BatchEntry* list;
    unsigned int* head;
    unsigned int grid;
};
// Resident workgroups of 256 threads of k_pack for the mode (kScanBatch or kScanCollectBatch).
unsigned int pack_grid_for(int mode, int device);
hipError_t launch_pack(int mode, const PackArgs& a);

// The packed group of a first-hit batch stage, a round of gpuhash_first_below_batch_early
// (pack_first_kernel.hip, a code object of its own): one persistent launch of k_pack_first over
// the group's tiles.  thresh, list and head are kScanFirstBatch's: {bound, target} per job, the
// result list and its head.
unsigned int pack_first_grid_for(int device);
hipError_t launch_pack_first(const PackArgs& a);

}  // namespace gpuhash
