// pack_first_kernel.hip -- k_pack_first, the kernel of a round of gpuhash_first_below_batch_early:
// the packed group {J = -1, C2 = 4} of a first-hit batch stage (stage.h, Stage::by_digits; pack.h;
// DESIGN.md 3.16), and its launch.  A code object of its own: neither k_pack's code nor any scan
// kernel's depends on it.
//
// k_pack's frame (pack_kernel.hip): persistent, 256 threads, pieces of clamp(remaining / (2 * grid),
// 1, kPackMaxPiece) tiles per atomicAdd on the group's counter, out when the value it got is >=
// total, so a drain (control.h) ends it within one piece.  No workgroup waits on another, there is
// no barrier inside the tile loop, and workgroup 0 writes the four clock words.
//
// thresh is MODE 5's per-job pair {bound, target}: the bound is the lowest qualifying nonce of the
// job found so far, armed to all ones.  Per tile every live lane loads its job's pair (the bound
// with a relaxed agent-scope load) and needs its hash only while its nonce n is <= the bound; a
// wave none of whose lanes needs its hash skips the tile.  Else hit = live && n <= bound && hash
// <= target, an exact 64-bit compare.  Within a wave the lanes of one job are one unbroken run
// (a class's space is its segments end to end), and inside a run the nonces ascend with the lane
// (a run is one segment's consecutive items): the run's lowest-nonce hit is its lowest hit lane,
// read off the ballot.  That one lane does old = atomicMin(bound + job, n) and, when n <= old (a
// nonce is hashed once, so equal only for 2^64-1 against the word as armed),
// appends BatchEntry{hash, n, job} with one atomicAdd on the list's head, the store guarded by the
// capacity in head[1].  At most one append per (wave, job), which is what the proved list bound
// counts (pack.h, pack_seg_entries).
//
// Exact: bound[job] only ever holds a qualifying nonce of the job, so it never falls below the
// job's answer A among the round's nonces; the lane of A is therefore never skipped, it is its
// run's lowest hit (nothing lower qualifies), and every tile is taken once, so old >= A there, equal
// only to the armed word, and it appends.  The host folds a job's entries by the lowest nonce.
// All stores are ordinary vector stores.
#include <atomic>

#include "kernels.h"
#include "pack.h"

namespace gpuhash {

__global__ __launch_bounds__(256) void k_pack_first(const PackJob* __restrict__ recs, const PackSeg* __restrict__ segs,
                                                    const PackTile* __restrict__ tiles, unsigned long long total,
                                                    unsigned long long* __restrict__ work,
                                                    unsigned long long* __restrict__ thresh,
                                                    BatchEntry* __restrict__ list, unsigned int* __restrict__ head) {
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
            const uint32_t job = live ? rec.job : kPackNoJob;
            unsigned long long* const words = thresh + 2ull * (live ? job : 0u);
            const unsigned long long bound = __hip_atomic_load(words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long target = words[1];
            const bool wanted = live && n <= bound;
            if (__builtin_amdgcn_ballot_w64(wanted) == 0ull) continue;  // wave-uniform: nothing here can answer
            uint32_t H0, H1;
            pack_hash(rec, o, d, n, H0, H1);
            const unsigned long long hv = ((unsigned long long)H0 << 32) | H1;
            const bool hit = wanted && hv <= target;
            const unsigned long long hits = __builtin_amdgcn_ballot_w64(hit);
            if (hits == 0ull) continue;
            // the runs of lanes of one job, as k_pack cuts them: this lane's run from `lead` to `last`
            const uint32_t before = __shfl_up(job, 1);
            const bool first = lane == 0 || before != job;
            const unsigned long long heads = __builtin_amdgcn_ballot_w64(first);
            const unsigned long long rest = lane == 63u ? 0ull : heads >> (lane + 1u);
            const uint32_t last = rest ? lane + (uint32_t)__builtin_ctzll(rest) : 63u;
            const uint32_t lead = 63u - (uint32_t)__builtin_clzll(heads & (~0ull >> (63u - lane)));
            const unsigned long long upto_last = last == 63u ? ~0ull : (1ull << (last + 1u)) - 1ull;
            const unsigned long long run = hits & upto_last & ~((1ull << lead) - 1ull);
            // the run's lowest hit lane holds its lowest qualifying nonce
            if (hit && (run & ((1ull << lane) - 1ull)) == 0ull) {
                const unsigned long long old = atomicMin(words, n);
                if (n <= old) {  // equal only at 2^64-1, a legal answer, against the word as armed
                    const unsigned int at = atomicAdd(head, 1u);
                    if (at < head[1]) {
                        BatchEntry* const e = list + at;
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

unsigned int pack_first_grid_for(int device) {
    // cached per device, as pack_kernel.hip caches k_pack's: resident blocks per CU x CUs
    static std::atomic<unsigned int> cache[64];
    if (device < 0 || device >= 64) return 0;
    unsigned int v = cache[device].load(std::memory_order_relaxed);
    if (!v) {
        int nb = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)&k_pack_first, 256, 0) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
            return 0;
        v = (unsigned int)(nb > 0 ? nb : 1) * (unsigned int)cus;
        cache[device].store(v, std::memory_order_relaxed);
    }
    return v;
}

hipError_t launch_pack_first(const PackArgs& a) {
    if (!a.grid || !a.ntiles || !a.recs || !a.segs || !a.tiles || !a.work || !a.thresh || !a.list || !a.head)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pack_first, dim3(a.grid), dim3(256), 0, a.stream, (const PackJob*)a.recs,
                       (const PackSeg*)a.segs, (const PackTile*)a.tiles, a.ntiles, a.work, a.thresh, a.list, a.head);
    return hipGetLastError();
}

}  // namespace gpuhash
