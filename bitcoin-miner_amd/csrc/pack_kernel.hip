// pack_kernel.hip -- k_pack, the kernel of a batch stage's packed group (stage.h, C2 = 4; pack.h;
// DESIGN.md 3.15), and its launch.  A code object of its own: no scan kernel's code depends on it.
//
// Persistent, 256 threads.  A workgroup takes pieces of clamp(remaining / (2 * grid), 1,
// kPackMaxPiece) tiles with one atomicAdd on the group's counter and leaves when the value it
// got is >= total -- k_scan's protocol, so a drain (control.h) ends it within one piece.  No
// workgroup waits on another, and a workgroup's loop runs at most `total` times.  Workgroup 0
// writes the four clock words as k_scan does.
//
// Per tile every lane takes one item: it finds its segment between the tile's first and last,
// loads the segment and its job's record (neighbouring lanes mostly share both), and hashes its
// nonce with pack.h's block building and compression.  Lanes past the class's end are idle.
// Within a wave the lanes of one job are one unbroken run (a class's space is its segments end
// to end, and a job has one segment per class), which the two modes reduce per run:
//
//   kScanBatch (min)  thresh, list and head are MODE 4's.  A segmented minimum by the (hash,
//     nonce) key, lowest nonce on ties, leaves each run's best in its first lane, which appends
//     BatchEntry{hash, nonce, job} when hash <= old, old = atomicMin(thresh + job, hash) -- and
//     skips the atomic when a plain read of the word is already below its hash.  thresh[job] only
//     ever holds a hash some nonce of the job achieved, so it never falls below the job's least
//     hash: the run that holds the job's argmin (and every run that ties with it) finds hash <=
//     the word at the read and at the atomic alike, and appends; the host's fold by (hash, nonce)
//     picks the lowest nonce.  One atomic per (wave, job) at most, which is what the proved list
//     bound counts (pack.h, pack_seg_entries); the store is guarded by the head's capacity all
//     the same.
//   kScanCollectBatch  thresh, list and head are MODE 6's.  Per lane the exact 64-bit hash <=
//     target[job]; per run one atomic add of its hit count on the job's counter and, if the job
//     lists, one on the list's 64-bit append counter, then the hits are stored in lane order
//     while the slot is below the capacity.  Hits past it are counted, not stored.
// All stores are ordinary vector stores.
#include <atomic>

#include "kernels.h"
#include "pack.h"

namespace gpuhash {

template <int MODE>
__global__ __launch_bounds__(256) void k_pack(const PackJob* __restrict__ recs, const PackSeg* __restrict__ segs,
                                              const PackTile* __restrict__ tiles, unsigned long long total,
                                              unsigned long long* __restrict__ work,
                                              unsigned long long* __restrict__ thresh, BatchEntry* __restrict__ list,
                                              unsigned int* __restrict__ head) {
    static_assert(MODE == kScanBatch || MODE == kScanCollectBatch, "the min and the collect mode");
    __shared__ unsigned long long sh_grab[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    unsigned long long* const clk = work + 1;
    if (blockIdx.x == 0 && tid == 0) {
        clk[0] = __builtin_amdgcn_s_memtime();
        clk[1] = __builtin_amdgcn_s_memrealtime();
    }
    for (;;) {
        if (tid == 0) {
            const unsigned long long cur = __hip_atomic_load(work, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long rem = cur < total ? total - cur : 0ull;
            unsigned long long g = rem / (2ull * gridDim.x);
            g = g < 1ull ? 1ull : (g > kPackMaxPiece ? kPackMaxPiece : g);
            sh_grab[0] = atomicAdd(work, g);
            sh_grab[1] = g;
        }
        __syncthreads();
        unsigned long long x = sh_grab[0];
        const unsigned long long g = sh_grab[1];
        __syncthreads();
        if (x >= total) break;
        const unsigned long long end = x + g < total ? x + g : total;
        for (; x < end; x++) {
            const PackTile& T = tiles[x];
            const uint32_t o = __builtin_amdgcn_readfirstlane(T.o), d = __builtin_amdgcn_readfirstlane(T.d);
            const uint32_t sf = __builtin_amdgcn_readfirstlane(T.seg_first);
            const uint32_t sl = __builtin_amdgcn_readfirstlane(T.seg_last);
            const unsigned long long item = T.item0 + tid;
            const PackSeg& S = segs[pack_find_seg(segs, sf, sl, item)];
            const unsigned long long idx = item - S.start;
            const bool live = idx < S.count;
            const unsigned long long n = S.n0 + idx;
            const PackJob& rec = recs[S.rec];
            uint32_t H0, H1;
            pack_hash(rec, o, d, n, H0, H1);
#ifdef GPUHASH_TIE_TEST_BITS
            H0 >>= (32 - GPUHASH_TIE_TEST_BITS);
            H1 = 0;
#endif
            const uint32_t job = live ? rec.job : kPackNoJob;
            // the runs of lanes of one job: a run's first lane, and for every lane its run's last
            const uint32_t before = __shfl_up(job, 1);
            const bool first = lane == 0 || before != job;
            const unsigned long long heads = __builtin_amdgcn_ballot_w64(first);
            const unsigned long long rest = lane == 63u ? 0ull : heads >> (lane + 1u);
            const uint32_t last = rest ? lane + (uint32_t)__builtin_ctzll(rest) : 63u;
            if constexpr (MODE == kScanBatch) {
                unsigned long long h = live ? ((unsigned long long)H0 << 32) | H1 : ~0ull;
                unsigned long long bn = live ? n : ~0ull;
#pragma unroll
                for (uint32_t off = 1; off < 64; off <<= 1) {
                    const unsigned long long oh = __shfl_down(h, off), on = __shfl_down(bn, off);
                    if (lane + off <= last && (oh < h || (oh == h && on < bn))) { h = oh; bn = on; }
                }
                if (first && live) {
                    const unsigned long long seen =
                        __hip_atomic_load(thresh + job, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (h <= seen && h <= atomicMin(thresh + job, h)) {
                        const unsigned int at = atomicAdd(head, 1u);
                        if (at < head[1]) {
                            BatchEntry* const e = list + at;
                            e->hash = h;
                            e->nonce = bn;
                            e->job = job;
                        }
                    }
                }
            } else {
                const unsigned long long hv = ((unsigned long long)H0 << 32) | H1;
                const unsigned long long* const words = thresh + (unsigned long long)kCollectJobWords * (live ? job : 0u);
                const bool hit = live && hv <= words[1];
                const bool lists = live && words[2] != 0ull;
                const unsigned long long hits = __builtin_amdgcn_ballot_w64(hit);
                // the run's first lane: the highest set bit of `heads` at or below this lane
                const uint32_t lead = 63u - (uint32_t)__builtin_clzll(heads & (~0ull >> (63u - lane)));
                const unsigned long long upto_last = last == 63u ? ~0ull : (1ull << (last + 1u)) - 1ull;
                const unsigned long long run = hits & upto_last & ~((1ull << lead) - 1ull);
                unsigned long long base = 0ull;
                if (first && live && run) {
                    const unsigned long long c = (unsigned long long)__builtin_popcountll(run);
                    atomicAdd(thresh + (unsigned long long)kCollectJobWords * job, c);
                    if (lists) base = atomicAdd(reinterpret_cast<unsigned long long*>(head), c);
                }
                base = __shfl(base, (int)lead);
                if (hit && lists) {
                    const unsigned long long slot = base + (unsigned long long)__builtin_popcountll(run & ((1ull << lane) - 1ull));
                    if (slot < (unsigned long long)head[2]) {
                        BatchEntry* const e = list + slot;
                        e->hash = hv;
                        e->nonce = n;
                        e->job = job;
                    }
                }
            }
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        clk[2] = __builtin_amdgcn_s_memtime();
        clk[3] = __builtin_amdgcn_s_memrealtime();
    }
}

template <int MODE>
static unsigned int pack_occ(int device) {
    // cached per device, as kernels.hip caches the scan kernels': resident blocks per CU x CUs
    static std::atomic<unsigned int> cache[64];
    if (device < 0 || device >= 64) return 0;
    unsigned int v = cache[device].load(std::memory_order_relaxed);
    if (!v) {
        int nb = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)&k_pack<MODE>, 256, 0) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
            return 0;
        v = (unsigned int)(nb > 0 ? nb : 1) * (unsigned int)cus;
        cache[device].store(v, std::memory_order_relaxed);
    }
    return v;
}

unsigned int pack_grid_for(int mode, int device) {
    if (mode == kScanBatch) return pack_occ<kScanBatch>(device);
    if (mode == kScanCollectBatch) return pack_occ<kScanCollectBatch>(device);
    return 0;
}

template <int MODE>
static hipError_t pack_go(const PackArgs& a, unsigned long long total) {
    hipLaunchKernelGGL((k_pack<MODE>), dim3(a.grid), dim3(256), 0, a.stream, (const PackJob*)a.recs,
                       (const PackSeg*)a.segs, (const PackTile*)a.tiles, total, a.work, a.thresh, a.list, a.head);
    return hipGetLastError();
}

hipError_t launch_pack(int mode, const PackArgs& a) {
    if (!a.grid || !a.ntiles || !a.recs || !a.segs || !a.tiles || !a.work || !a.thresh || !a.head)
        return hipErrorInvalidValue;
    if (mode == kScanBatch) return a.list ? pack_go<kScanBatch>(a, a.ntiles) : hipErrorInvalidValue;
    if (mode == kScanCollectBatch) return pack_go<kScanCollectBatch>(a, a.ntiles);  // list null: no job lists
    return hipErrorInvalidValue;
}

}  // namespace gpuhash
