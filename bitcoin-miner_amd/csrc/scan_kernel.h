// scan_kernel.h -- gfx950 nonce-scan kernel template (included by kernels_*.hip).
//
// One workgroup = 256 lanes × one chunk of loop values r.  Each lane owns one lane
// value p (its digits fill message words J-1 / J-2, or block B-1 for C2 layouts) and
// iterates r (the digits of the LAST digit-bearing word W_J of the final block):
//
//   per work item (once):  lane words, the lane-only rounds before J, block B-1 for
//                           C2, and every schedule/round term that does not read W_J
//                           (compile-time dependency analysis `kDep` + LICM)
//   per nonce (hot loop):   W_J = U_J | ascii(r) << shift  -- wave-UNIFORM, SALU
//                           rounds J..63 on VALU, schedule words that depend on W_J,
//                           H0 = IV/CV-folded a64; one v_cmp against a wave-uniform
//                           pruning threshold T; rare slow path does the exact
//                           lexicographic (hash, nonce) update in scalar registers.
//
// Everything is integer VALU: v_alignbit_b32 rotates, v_bitop3_b32 (XOR3 0x96, CH
// 0xCA, MAJ 0xE8), v_add3_u32.  No LDS or HBM traffic in the loop; one 16-byte
// candidate per workgroup at the end (appended only if it beats the threshold).
//
// Semantics: bitcoin.Hash (src/github.com/cmu440/bitcoin/hash.go:11-15), argmin over
// the inclusive range with the lowest nonce winning ties (spec'd loop p1.pdf pp.12-14,
// north_star).  The pruning is exact: T only ever holds the high word of a hash some
// valid nonce already achieved, and ties on the high word take the slow path.
//
// MODE 2 (kScanFirst) is the other question, gpuhash_first_below: the LOWEST nonce whose hash is
// at or below a target.  Per nonce it costs what MODE 0 costs (the same v_cmp and ballot, T = the
// target's high word); the word `thresh` points to holds the lowest qualifying nonce found
// so far, and parts of the work that lie wholly above it are skipped unhashed (k_scan, at
// the grab).
//
// MODE 3 (kScanCollect) is the third, gpuhash_collect_below: EVERY nonce whose hash is at or below
// a target, counted exactly and listed while the device list has room (CollectState, below).  The
// same per-nonce compare and ballot; the slow path appends.
//
// MODE 4 (kScanBatch) is MODE 0 for a batch of independent jobs, gpuhash_min_batch (BatchState,
// below).
//
// MODE 5 (kScanFirstBatch) is MODE 2 for a batch of independent jobs, gpuhash_first_below_batch:
// MODE 2's per-nonce test, slow path, skip and drain rules against the CURRENT JOB's bound and
// target, and MODE 4's descriptor lookup, job change and result list (first_batch_flush, below).
//
// MODE 6 (kScanCollectBatch) is MODE 3 for a batch of independent jobs, gpuhash_collect_below_batch:
// MODE 3's per-nonce test and append path against the CURRENT JOB's target and counter, and MODE
// 4's descriptor lookup and job change (CollectBatchState, below).
//
// Every mode group is a code object of its own (scan_decl.h), and each mode compiles to the same
// machine code whatever the others hold: tests/golden/kernel_manifest.txt pins every kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "scan_decl.h"

// Code phase of the per-nonce loop bodies.  The same instruction stream runs ~3.5% faster
// when the loop body starts at 4 mod 8 bytes than at 0 mod 8 (measured on config 2, J = 2,
// J = 13 and config 3, profiles/r01_loop_phase.jsonl; the mechanism is in the instruction
// fetch of the mixed 4-/8-byte encodings).  Without this, any edit before the loop flips
// the phase at random.  ".p2align 3" + one s_nop pins it at 4 mod 8 for one or two s_nop
// per iteration (~0.1%).  -DGPUHASH_LOOP_PHASE=0 / -1 selects phase 0 / no pinning; the
// kernels_misc.hip layouts (classic straddle, extra block), insensitive to the phase,
// build with -1.
#ifndef GPUHASH_LOOP_PHASE
#define GPUHASH_LOOP_PHASE 4
#endif
#if GPUHASH_LOOP_PHASE == 4
#define GPUHASH_LOOP_ALIGN() asm volatile(".p2align 3\n\ts_nop 0")
#elif GPUHASH_LOOP_PHASE == 0
#define GPUHASH_LOOP_ALIGN() asm volatile(".p2align 3")
#else
#define GPUHASH_LOOP_ALIGN() ((void)0)
#endif

namespace gpuhash {

// MODE is a ScanMode (kernels.h).  The first-hit modes share the per-nonce test and the skip
// rule, the batch modes the descriptor lookup and the result list.
constexpr bool is_first_mode(int mode) { return mode == kScanFirst || mode == kScanFirstBatch; }
constexpr bool is_batch_mode(int mode) {
    return mode == kScanBatch || mode == kScanFirstBatch || mode == kScanCollectBatch;
}

namespace dev {

__device__ constexpr uint32_t K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u,
    0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u,
    0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u,
    0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
    0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u,
    0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu,
    0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au,
    0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
    0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

// Per-lane (VGPR) primitives: one VALU op each on gfx950.
__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) {
    return __builtin_amdgcn_alignbit(x, x, n);
}
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}
__device__ __forceinline__ uint32_t ch(uint32_t e, uint32_t f, uint32_t g) {
    return __builtin_amdgcn_bitop3_b32(e, f, g, 0xCA);
}
__device__ __forceinline__ uint32_t maj(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
}
__device__ __forceinline__ uint32_t bS0(uint32_t a) { return xor3(rotr(a, 2), rotr(a, 13), rotr(a, 22)); }
__device__ __forceinline__ uint32_t bS1(uint32_t e) { return xor3(rotr(e, 6), rotr(e, 11), rotr(e, 25)); }
__device__ __forceinline__ uint32_t bs0(uint32_t x) { return xor3(rotr(x, 7), rotr(x, 18), x >> 3); }
__device__ __forceinline__ uint32_t bs1(uint32_t x) { return xor3(rotr(x, 17), rotr(x, 19), x >> 10); }

// Wave-uniform primitives: plain C so the compiler keeps them on SALU.
__device__ __forceinline__ uint32_t urotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
// (LLVM issues the uniform sigma0(W_J) as v_alignbit with SGPR sources; pinning it on
// SALU measured 2.6% slower on config 2: tools/tuning_hooks.patch)
__device__ __forceinline__ uint32_t us0(uint32_t x) { return urotr(x, 7) ^ urotr(x, 18) ^ (x >> 3); }
__device__ __forceinline__ uint32_t us1(uint32_t x) { return urotr(x, 17) ^ urotr(x, 19) ^ (x >> 10); }

__device__ __forceinline__ uint32_t ascii4(uint32_t x) {
    uint32_t x1 = x / 10u, x2 = x1 / 10u, x3 = x2 / 10u;
    uint32_t d0 = x - x1 * 10u, d1 = x1 - x2 * 10u, d2 = x2 - x3 * 10u, d3 = x3 % 10u;
    return 0x30303030u | (d3 << 24) | (d2 << 16) | (d1 << 8) | d0;
}

// kDep<J>[t]: does schedule word W_t depend on the per-nonce word W_J?
template <int J>
struct DepTable {
    bool v[64];
    constexpr DepTable() : v() {
        for (int t = 0; t < 16; t++) v[t] = (t == J);
        for (int t = 16; t < 64; t++) v[t] = v[t - 2] || v[t - 7] || v[t - 15] || v[t - 16];
    }
};

template <int B, int E, class F>
__device__ __forceinline__ void sfor(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        sfor<B + 1, E>(f);
    }
}

struct State {
    uint32_t a, b, c, d, e, f, g, h;
};

// One generic round with K[t] + W folded into `kw`.
__device__ __forceinline__ void round_kw(State& s, uint32_t kw) {
    uint32_t t1 = s.h + kw + ch(s.e, s.f, s.g) + bS1(s.e);
    uint32_t t2 = bS0(s.a) + maj(s.a, s.b, s.c);
    s.h = s.g; s.g = s.f; s.f = s.e; s.e = s.d + t1;
    s.d = s.c; s.c = s.b; s.b = s.a; s.a = t1 + t2;
}

// A round whose K+W is wave-uniform (an SGPR) and whose h is per-lane.  A 2-input VALU
// add with a scalar operand issues at the slow rate; left to itself LLVM
// reads `kw` in the 2-input h + kw.  Here it goes into the 3-input add, slow class
// anyway, so the round's 2-input adds read VGPRs only.  The K+W-table layout (config 3)
// runs +1.8% with it; the plain, extra-block and lane-table rounds with a uniform K+W run
// 0.3-3.8% SLOWER with it (tools/tuning_hooks.patch; profiles/r04_fold_variants.jsonl),
// so only ut_hash's table rounds use it.
__device__ __forceinline__ void round_ukw(State& s, uint32_t kw) {
    uint32_t x;
    asm("v_add3_u32 %0, %1, %2, %3" : "=v"(x) : "v"(s.h), "s"(kw), "v"(ch(s.e, s.f, s.g)));
    uint32_t t1 = x + bS1(s.e);
    uint32_t t2 = bS0(s.a) + maj(s.a, s.b, s.c);
    s.h = s.g; s.g = s.f; s.f = s.e; s.e = s.d + t1;
    s.d = s.c; s.c = s.b; s.b = s.a; s.a = t1 + t2;
}

// Message expansion of a block whose words are all per-lane or uniform (no W_J):
// used for block B-1 of C2 layouts, once per work item.
__device__ __forceinline__ void expand_full(uint32_t (&w)[64]) {
    sfor<16, 64>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        w[t] = w[t - 16] + bs0(w[t - 15]) + w[t - 7] + bs1(w[t - 2]);
    });
}

}  // namespace dev

// Running best of one wave (wave-uniform, lives in SGPRs): exact lexicographic
// (hash, nonce) key and the pruning word T (high word of the best hash seen anywhere).
struct WaveBest {
    unsigned long long h, n;
    uint32_t T;
};

// MODE 2 (first hit, gpuhash_first_below).  wb.T is the high word of the target, and the
// rest of the mode's state lives in LDS, touched only by the rare slow path and at grabs:
// the search kernels' SGPR budget is full (one more live pair spills), and this frees the
// four that MODE 0 keeps its running best in.  A nonce of 2^64-1 is a legal hit, so
// `found` says whether a wave has one; no nonce value stands for "none".
struct FirstState {
    unsigned long long target;
    unsigned long long* bound;  // the word `thresh` points to: lowest qualifying nonce anywhere
    unsigned long long grab_bound;  // that word as thread 0 read it at this grab: ONE value
                                    // for the whole workgroup (see k_scan)
    unsigned long long n[4], h[4];  // per wave: its lowest-nonce hit
    unsigned int found[4];
};
__device__ __forceinline__ FirstState& first_state() {
    __shared__ FirstState fs;
    return fs;
}

// MODE 2 slow path: the exact 64-bit test of one candidate (hh, nn wave-uniform) that
// passed the high-word prune.  The wave keeps its lowest-nonce hit; a new one also lowers
// the shared bound, which every workgroup reads at its next grab to skip the parts that
// lie wholly above it.
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v);  // below

// Every word read from LDS goes straight back to scalar registers (uniform64 /
// readfirstlane) and the tests run in order, so the path holds one or two VGPRs at a time:
// it sits inside the per-nonce loop, where the plain kernels' 64 VGPRs are all taken.
__device__ __forceinline__ void first_hit(unsigned long long hh, unsigned long long nn) {
    FirstState& fs = first_state();
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (hh > uniform64(fs.target)) return;
    if (__builtin_amdgcn_readfirstlane(fs.found[w]) && nn >= uniform64(fs.n[w])) return;
    if ((threadIdx.x & 63u) == 0) {
        fs.n[w] = nn;
        fs.h[w] = hh;
        fs.found[w] = 1u;
        atomicMin(fs.bound, nn);
    }
}

// MODE 3 (collect, gpuhash_collect_below): every nonce whose hash is at or below a target is
// counted, and appended to a device list while the list has room.  k_scan's arguments are
// reused, none is added:
//   thresh   the 64-bit hit counter (the host zeroes it): the number of qualifying nonces
//   cands    the hit list, Cand{hash, nonce}
//   *ncand   the list's capacity in entries, READ-ONLY here (0: count only)
//   dump_lo  the target; wb.T is its high word, as in MODE 2
// The per-nonce test is MODE 2's compare and ballot.  The slow path has no bound, no skip
// rule and no per-wave state: one atomic add per ballot reserves popcount(ballot) consecutive
// slots, and the hits of the ballot are stored at them in lane order while slot < capacity.
// Hits past the capacity are counted, not stored, so the counter is exact whatever the list
// holds, and the host re-runs a range whose count exceeds the capacity (collect.h).  The
// counter is 64-bit: a 2^38-nonce slice under a dense target passes 2^32 hits.
// As in MODE 2 the state lives in LDS and every word read from it goes straight back to
// scalar registers, so nothing new is live across the per-nonce loop.  The stores are lane 0's
// ordinary vector stores of wave-uniform values.
struct CollectState {
    unsigned long long* count;
    Cand* list;
    uint32_t cap;
    uint32_t target_lo;
};
__device__ __forceinline__ CollectState& collect_state() {
    __shared__ CollectState cs;
    return cs;
}

// The lanes that hold a hit: inside the launch's edges (`ok`) and hash <= target, all 64 bits
// (T is the target's high word).
__device__ __forceinline__ unsigned long long collect_ballot(uint32_t H0, uint32_t H1, uint32_t T, bool ok) {
    const uint32_t tlo = __builtin_amdgcn_readfirstlane(collect_state().target_lo);
    return __builtin_amdgcn_ballot_w64(ok && (H0 < T || (H0 == T && H1 <= tlo)));
}

// Counts the hits of ballot m (non-empty) and returns the slot of its first one.
__device__ __forceinline__ unsigned long long collect_reserve(unsigned long long m) {
    unsigned long long old = 0;
    if ((threadIdx.x & 63u) == 0)
        old = atomicAdd(collect_state().count, (unsigned long long)__builtin_popcountll(m));
    return uniform64(old);
}

__device__ __forceinline__ bool collect_room(unsigned long long slot) {
    return slot < __builtin_amdgcn_readfirstlane(collect_state().cap);
}

// slot < capacity (collect_room); hh, nn wave-uniform.
__device__ __forceinline__ void collect_store(unsigned long long slot, unsigned long long hh,
                                              unsigned long long nn) {
    if ((threadIdx.x & 63u) == 0) {
        Cand* const e = collect_state().list + slot;
        e->hash = hh;
        e->nonce = nn;
    }
}

// MODE 4 (batch, gpuhash_min_batch): MODE 0's question for many independent jobs in one launch.
// Every descriptor names its job (LaunchDesc::job) and a group's descriptors lie in ascending
// job order.  Per nonce nothing differs from MODE 0: the compare of H0 against wb.T, the ballot
// and MODE 0's slow path.  What is per launch in MODE 0 is per job here, and k_scan's arguments
// are reused:
//   thresh   an array of pruning words, one per job (armed to all ones): thresh[job] only ever
//            holds a hash some nonce of that job achieved
//   cands    the result list, BatchEntry{hash, nonce, job}
//   ncand    the list's append counter (armed to 0); the word after it is the list's capacity
// A workgroup's WaveBest belongs to one job at a time.  When the next part's descriptor names
// another job the workgroup FLUSHES -- merges its four waves through LDS, lowers thresh[job]
// and appends one entry, if it holds a candidate at all -- and re-arms wb from the new job's
// word; it flushes once more at the end of the kernel.  Parts, pieces and descriptor order are
// workgroup-uniform, so the flush's barriers are met by all four waves (between rows, never
// inside one).  The host folds the list per job by the (hash, nonce) key: the wave that hashes
// a job's argmin keeps it (T never falls below the high word of a hash of that job, and ties
// take the slow path), its workgroup appends it, and the fold finds it.  No workgroup waits on
// another.  The capacity is a proved bound (stage.h, batch_job_entries); the store is guarded
// by it all the same.
// The mode's words live in LDS and come back to scalar registers on these cold paths only, so
// nothing but MODE 0's WaveBest is live across the per-nonce loop.
constexpr uint32_t kNoJob = 0xFFFFFFFFu;
struct BatchState {
    unsigned long long* thresh;
    BatchEntry* list;
    unsigned int* count;
    // The job the workgroup's WaveBest belongs to (kNoJob: none yet).  Thread 0 writes it at a
    // job change, between two barriers: every wave has read the old value before, and reads
    // the new one after.  One word for the workgroup, at a constant LDS address: a slot per
    // wave, indexed by threadIdx.x >> 6, kept that index alive in a VGPR across the per-nonce
    // loop, and the plain kernels have none to spare (one K+W sum then moved into the loop).
    uint32_t job;
    // A HINT for the next descriptor lookup: the descriptor some wave found last.  The waves
    // write it unsynchronised (they find the same descriptors, but not at the same time), so
    // batch_find trusts no more of it than that it is an index.
    uint32_t idx;
};
__device__ __forceinline__ BatchState& batch_state() {
    __shared__ BatchState bs;
    return bs;
}
// The state at the start of a launch, from k_scan's arguments: no job yet.  Thread 0 alone.
__device__ __forceinline__ void batch_arm(unsigned long long* thresh, Cand* cands, unsigned int* ncand) {
    BatchState& bs = batch_state();
    bs.thresh = thresh;
    bs.list = reinterpret_cast<BatchEntry*>(cands);
    bs.count = ncand;
    bs.job = kNoJob;
    bs.idx = 0u;
}

// The pruning word of `job`, its high half: the T to arm or tighten a WaveBest with.
__device__ __forceinline__ uint32_t batch_T(uint32_t job) {
    unsigned long long* const th = (unsigned long long*)uniform64((unsigned long long)batch_state().thresh);
    const unsigned long long tv = __hip_atomic_load(th + job, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __builtin_amdgcn_readfirstlane((uint32_t)(tv >> 32));
}

// Leaves `job`: the workgroup's best for it, one list entry if it has any.  Every wave of the
// workgroup calls this at the same point.
// (The four-wave fold below is also the end of k_scan for MODE 0, and first_batch_flush's is the
// end for MODE 2, as copies: a shared helper -- with out-parameters, a returned struct or a
// callback -- changed the register assignment of one user or the other each time it was tried.)
__device__ __forceinline__ void batch_flush(const WaveBest& wb, uint32_t job,
                                            unsigned long long (&sh_best)[4][2]) {
    const uint32_t tid = threadIdx.x;
    if ((tid & 63u) == 0) { sh_best[tid >> 6][0] = wb.h; sh_best[tid >> 6][1] = wb.n; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long bh = sh_best[0][0], bn = sh_best[0][1];
#pragma unroll
        for (int i = 1; i < 4; i++) {
            if (sh_best[i][0] < bh || (sh_best[i][0] == bh && sh_best[i][1] < bn)) {
                bh = sh_best[i][0];
                bn = sh_best[i][1];
            }
        }
        if (bh != ~0ull || bn != ~0ull) {
            BatchState& bs = batch_state();
            atomicMin(bs.thresh + job, bh);
            const unsigned int idx = atomicAdd(bs.count, 1u);
            if (idx < bs.count[1]) {
                BatchEntry* const e = bs.list + idx;
                e->hash = bh;
                e->nonce = bn;
                e->job = job;
            }
        }
    }
    __syncthreads();  // sh_best is free again
}

// MODE 5 (first-hit batch, gpuhash_first_below_batch): MODE 2's question for many independent jobs
// in launches that run in ascending digit order (stage.h, Stage::by_digits).  k_scan's arguments
// are MODE 4's, except that `thresh` holds TWO words per job: thresh[2 * job] is the job's bound,
// the lowest qualifying nonce found so far (armed to all ones), thresh[2 * job + 1] its target.
// The workgroup's FirstState belongs to one job at a time: `bound` and `target` are the current
// job's, and a wave's `found`, `n`, `h` its lowest-nonce hit FOR THAT JOB.  Per nonce nothing
// differs from MODE 2 (wb.T is the high word of the current job's target); first_hit lowers the
// job's bound at the hit.  At a job change (MODE 4's place: between rows, all four waves meeting
// the barriers) the workgroup appends its lowest-nonce hit for the job it leaves, if it has one,
// and thread 0 publishes the new job's bound and target through LDS; one more flush ends the
// kernel.  The host folds the list per job by the lowest nonce.  Exactness is MODE 2's, job by job:
// a job's bound only ever holds a qualifying nonce of that job, so it never drops below the job's
// answer; a part is skipped, and the rest of its descriptor (one job's) taken off the work
// counter, only when all its nonces lie above the bound; so the answer is hashed, the wave that
// hashes it keeps it (no lower nonce qualifies), and its workgroup appends it when it leaves the job.
// Every wave of the workgroup calls this at the same point; job == kNoJob appends nothing.
__device__ __forceinline__ void first_batch_flush(uint32_t job) {
    __syncthreads();  // every wave's hits for `job` are in LDS
    if (threadIdx.x == 0 && job != kNoJob) {
        const FirstState& fs = first_state();
        unsigned long long bn = 0, bh = 0;
        unsigned int any = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (fs.found[i] && (!any || fs.n[i] < bn)) {
                bn = fs.n[i];
                bh = fs.h[i];
                any = 1;
            }
        }
        if (any) {
            BatchState& bs = batch_state();
            const unsigned int idx = atomicAdd(bs.count, 1u);
            if (idx < bs.count[1]) {
                BatchEntry* const e = bs.list + idx;
                e->hash = bh;
                e->nonce = bn;
                e->job = job;
            }
        }
    }
}

// MODE 5, at a skipped part of descriptor i: how far the work counter may move.  Every later part
// of descriptor i lies above its job's bound (k_scan); wave 0 looks at the up to 64 descriptors
// after it as well, one per lane, and takes with it the unbroken run of those whose EVERY nonce
// lies above their own job's bound (desc_min_nonce against that job's word, read here): once the
// low digit counts have answered most jobs, a launch of a higher digit count is descriptors of
// this kind end to end, and moving the counter one descriptor per grab made such a launch cost
// 20 us per descriptor.  The same rule as the part's, applied to whole descriptors:
// a job's bound never drops below its answer, so nothing at or below an answer is left out.
// Returns the end position of the last descriptor taken; called by wave 0 only, all 64 lanes.
template <int C2>
__device__ __forceinline__ unsigned long long first_batch_drain_end(const LaunchDesc* __restrict__ descs,
                                                                    const unsigned long long* __restrict__ offs,
                                                                    int ndesc, int i) {
    const int k = i + 1 + (int)(threadIdx.x & 63u);
    bool above = false;
    if (k < ndesc) {
        const LaunchDesc& N = descs[k];
        const unsigned long long b =
            __hip_atomic_load(batch_state().thresh + 2ull * N.job, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        above = desc_min_nonce(N, C2) > b;
    }
    const unsigned long long m = ~__builtin_amdgcn_ballot_w64(above);
    const int run = m ? __builtin_ctzll(m) : 64;
    return offs[i + 1 + run];
}

// The descriptor that owns position x: the largest i with offs[i] <= x (offs[0] = 0 and the
// offsets rise strictly).  A workgroup's positions only rise, so the search starts from the
// hint, the descriptor of a previous part: usually it is that one or the next, else a binary
// search of the descriptors after it -- or before it, if the hint came from a wave that is
// already further on.  O(log ndesc) scalar loads at worst, two at best.
__device__ __forceinline__ int batch_find(const unsigned long long* __restrict__ offs, int ndesc,
                                          unsigned long long x) {
    BatchState& bs = batch_state();
    int i = (int)__builtin_amdgcn_readfirstlane(bs.idx);
    int lo = 0, hi = ndesc - 1;
    if (offs[i] > x) {
        hi = i - 1;
    } else if (i + 1 < ndesc && offs[i + 1] <= x) {
        i++;
        if (i + 1 < ndesc && offs[i + 1] <= x) lo = i + 1;
        else lo = hi = i;
    } else {
        return i;
    }
    while (lo < hi) {  // offs[lo] <= x
        const int mid = (lo + hi + 1) >> 1;
        if (offs[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    i = lo;
    if ((threadIdx.x & 63u) == 0) bs.idx = (uint32_t)i;
    return i;
}

// MODE 6 (collect batch, gpuhash_collect_below_batch): MODE 3's question for many independent jobs
// in one launch per kernel variant, in MODE 4's job-major stage.  k_scan's arguments are MODE 4's,
// except:
//   thresh   THREE 64-bit words per job (kCollectJobWords): thresh[3 * job] is the job's exact hit
//            counter (armed to 0), thresh[3 * job + 1] its target, thresh[3 * job + 2] whether the
//            job lists at all (cap_k > 0), both READ-ONLY here
//   cands    the ONE list all listing jobs share, BatchEntry{hash, nonce, job}
//   ncand    the list's head: a 64-bit append counter (armed to 0), then its capacity (a uint32)
// Per nonce nothing differs from MODE 3 (wb.T is the high word of the current job's target).  The
// slow path adds the ballot's popcount to the JOB's counter, and, if the job lists, reserves that
// many slots with one atomic add on the list's append counter and stores its hits at them, tagged
// with the job, each only while its slot is below the capacity.  The append counter is 64 bits
// wide and slots are compared as 64-bit: a run's hits are bounded only by its nonces (2^16 jobs of
// 2^38), so a 32-bit counter could wrap back into the list.  A job's counter is exact whatever the
// list holds; each hit is stored once or not at all, so a job whose tagged entries number its
// counter has all its hits in the list, and the host re-runs alone a job that has not.
// No per-wave state belongs to a job: at a job change (MODE 4's place: between rows, all four waves
// at the barriers) nothing is flushed, thread 0 publishes the new job's counter address, target
// and list flag through LDS between two barriers, and every wave re-arms wb.T.  Nothing happens at
// the end of the kernel; no workgroup waits on another.
// As in MODE 3 the words live in LDS and come back to scalar registers on the slow path only, so
// nothing new is live across the per-nonce loop.  The stores are lane 0's ordinary vector stores
// of wave-uniform values.
struct CollectBatchState {
    unsigned long long* count;  // the current job's hit counter
    uint32_t target_hi, target_lo;
    uint32_t cap;  // the list's capacity in entries if the current job lists, else 0
};
__device__ __forceinline__ CollectBatchState& collect_batch_state() {
    __shared__ CollectBatchState cbs;
    return cbs;
}

// collect_ballot for the current job's target.
__device__ __forceinline__ unsigned long long collect_batch_ballot(uint32_t H0, uint32_t H1, uint32_t T, bool ok) {
    const uint32_t tlo = __builtin_amdgcn_readfirstlane(collect_batch_state().target_lo);
    return __builtin_amdgcn_ballot_w64(ok && (H0 < T || (H0 == T && H1 <= tlo)));
}

// Counts the hits of ballot m (non-empty) for the current job and returns the list slot of its
// first one; a job that does not list reserves nothing and gets a slot no capacity is above.
__device__ __forceinline__ unsigned long long collect_batch_reserve(unsigned long long m) {
    unsigned long long slot = ~0ull;
    if ((threadIdx.x & 63u) == 0) {
        const CollectBatchState& cbs = collect_batch_state();
        const unsigned long long n = (unsigned long long)__builtin_popcountll(m);
        atomicAdd(cbs.count, n);
        if (cbs.cap) slot = atomicAdd(reinterpret_cast<unsigned long long*>(batch_state().count), n);
    }
    return uniform64(slot);
}

__device__ __forceinline__ bool collect_batch_room(unsigned long long slot) {
    return slot < (unsigned long long)__builtin_amdgcn_readfirstlane(collect_batch_state().cap);
}

// slot < capacity (collect_batch_room); hh, nn wave-uniform.
__device__ __forceinline__ void collect_batch_store(unsigned long long slot, unsigned long long hh,
                                                    unsigned long long nn) {
    if ((threadIdx.x & 63u) == 0) {
        const BatchState& bs = batch_state();
        BatchEntry* const e = bs.list + slot;
        e->hash = hh;
        e->nonce = nn;
        e->job = bs.job;
    }
}

// Rounds 0..63 of block B when its whole message schedule is wave-uniform (C2 layouts
// whose loop digits are the only digits in block B): kw[t] = K[t] + W_t comes from a
// table, the per-lane input is the state s after block B-1 (= cv), so a nonce costs 64
// rounds and no schedule work.  Round 0 reuses the per-row part `inv0` (everything but
// kw[0]); round 63 skips e and folds CV0.
// Rounds t in [SK0, SK1) have a wave-uniform kw(t) (scalar loads) and a per-lane h.
template <int SK0, int SK1, class KW>
__device__ __forceinline__ void ut_hash(const dev::State& s, const uint32_t (&cv)[8], uint32_t inv0,
                                        uint32_t t20, KW&& kw, uint32_t& H0, uint32_t& H1) {
    using namespace dev;
    dev::State x = s;
    const uint32_t k0 = kw(0);
    x.h = x.g; x.g = x.f; x.f = x.e; x.e = (x.d + inv0) + k0;
    x.d = x.c; x.c = x.b; x.b = x.a; x.a = (inv0 + t20) + k0;
    sfor<1, 63>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        if constexpr (t >= SK0 && t < SK1) round_ukw(x, kw(t));
        else round_kw(x, kw(t));
    });
    const uint32_t t1 = x.h + kw(63) + cv[0] + ch(x.e, x.f, x.g) + bS1(x.e);
    H0 = t1 + bS0(x.a) + maj(x.a, x.b, x.c);
    H1 = cv[1] + x.a;
}

// One row of one launch: 256 consecutive lane values p (row) x loop values [r0, r1).
//
// C2 = 0: lane digits in words J-2, J-1 of block B, loop digits in W_J.
// C2 = 1: lane digits spill into block B-1 (compressed per lane, once per row); for J = 0
//         block B holds only loop digits, so its schedule is the per-r table `ktab`
//         (built by k_ktab, read with scalar loads).
// C2 = 2: (J = 1) block B's W_0 and W_1 hold only LOOP digits (r = W_0 digits * R1 + W_1
//         digits) and the lanes vary block B-1 only; the uniform schedules of 64 loop
//         values at a time are built by wave 0 into LDS and shared by the 4 waves.
template <int J, int C2, bool EX, int MODE>
__device__ __forceinline__ void scan_row(const LaunchDesc& D, uint32_t row, uint32_t r0, uint32_t r1,
                                         WaveBest& wb, unsigned long long* __restrict__ dump,
                                         unsigned long long dump_lo, const uint32_t* __restrict__ ktab) {
    using namespace dev;
    constexpr DepTable<J> kDep{};
    constexpr bool UT = C2 == 2 || (C2 == 1 && J == 0);  // uniform block-B schedule
    const uint32_t p = D.p_first + row * 256u + threadIdx.x;
    // A wave whose 64 lanes all lie past the launch's last lane value (the tail of a
    // partial last row) has no nonce to hash: it skips the row (up to 3.4x on one-row
    // C2 = 2 searches, profiles/r02_partial_rows.jsonl).  Only the C2 = 2 loop has
    // barriers (its LDS batches), so there an idle wave still walks the batches but
    // hashes nothing.  (Rotating which wave takes which 64-lane block per workgroup, to
    // spread the idle slots over the SIMDs, measured 1-4% slower on partial rows.)
    const bool wave_idle =
        __builtin_amdgcn_readfirstlane(D.p_first + row * 256u + (threadIdx.x & ~63u)) > D.p_last;
    if constexpr (C2 != 2) {
        if (wave_idle) return;
    }

    // ---- once per row: lane words and everything that does not read W_J ----
    const uint32_t alo = ascii4(p % 10000u);
    const uint32_t ahi = ascii4((p / 10000u) % 10000u);
    uint32_t W[16];
#pragma unroll
    for (int i = 0; i < 16; i++) W[i] = D.U[i];
    State s;
    uint32_t cv[8];
    if constexpr (C2 != 0) {
        uint32_t V[64];
#pragma unroll
        for (int i = 0; i < 16; i++) V[i] = D.U1[i];
        if constexpr (UT) {  // every lane digit sits at the end of block B-1
            V[15] |= alo & D.mask_lo;
            V[14] |= ahi & D.mask_hi;
        } else {
            V[15] |= ahi & D.mask_hi;
            W[0] |= alo & D.mask_lo;
        }
        expand_full(V);
        s = State{D.S1[0], D.S1[1], D.S1[2], D.S1[3], D.S1[4], D.S1[5], D.S1[6], D.S1[7]};
        sfor<14, 64>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            round_kw(s, K[t] + V[t]);
        });
        cv[0] = D.CV1[0] + s.a; cv[1] = D.CV1[1] + s.b; cv[2] = D.CV1[2] + s.c; cv[3] = D.CV1[3] + s.d;
        cv[4] = D.CV1[4] + s.e; cv[5] = D.CV1[5] + s.f; cv[6] = D.CV1[6] + s.g; cv[7] = D.CV1[7] + s.h;
        s = State{cv[0], cv[1], cv[2], cv[3], cv[4], cv[5], cv[6], cv[7]};
        if constexpr (!UT && J == 1) round_kw(s, K[0] + W[0]);
    } else {
        s = State{D.S0[0], D.S0[1], D.S0[2], D.S0[3], D.S0[4], D.S0[5], D.S0[6], D.S0[7]};
#pragma unroll
        for (int i = 0; i < 8; i++) cv[i] = D.CV[i];
        if constexpr (J >= 2) {
            W[J - 2] |= ahi & D.mask_hi;
            W[J - 1] |= alo & D.mask_lo;
            round_kw(s, K[J - 2] + W[J - 2]);
            round_kw(s, K[J - 1] + W[J - 1]);
        } else if constexpr (J == 1) {
            W[0] |= alo & D.mask_lo;
            round_kw(s, K[0] + W[0]);
        }
    }
    // UT layouts: round 0 of block B without its K+W term (per row)
    uint32_t inv0 = 0, t20 = 0;
    if constexpr (UT) {
        inv0 = s.h + bS1(s.e) + ch(s.e, s.f, s.g);
        t20 = bS0(s.a) + maj(s.a, s.b, s.c);
    }

    // Edge handling: only the first / last lane of a launch has a partial r range, and
    // lanes past p_last are idle.  Checked only in the (rare) slow path.
    const bool lane_ok = p <= D.p_last;
    const uint32_t rlo = (p == D.p_first) ? D.r_first : 0u;
    const uint32_t rhi = (p == D.p_last) ? D.r_last : D.R - 1u;

    // Per-nonce bookkeeping: dump (MODE 1) or the exact lexicographic running best with
    // the wave-uniform pruning test (MODE 0).
    // The ballot-and-readlane walk is written out per mode, here and in scan_row_lt, on purpose:
    // sharing it (a hit_test<MODE> taking the edge predicate and the nonce formula, or the
    // predicate inside the ballot) reordered the hot loops of 12 to 76 of the kernels when tried.
    // Do not fold it without GPU measurements of every kernel whose code changes.
    auto finish = [&](uint32_t r, uint32_t H0, uint32_t H1) {
#ifdef GPUHASH_TIE_TEST_BITS
        // Test-only build (libgpuhash_tietest.so): keep only the top bits of the hash so
        // equal keys are common and every reduction level's lowest-nonce rule is exercised.
        H0 >>= (32 - GPUHASH_TIE_TEST_BITS);
        H1 = 0;
#endif
        if constexpr (MODE == kScanDump) {
            if (lane_ok && r >= rlo && r <= rhi) {
                // k = D.base + p·R + r; nonce = k·stride + tail (tail-digit launches, plan.h)
                unsigned long long n = (D.base + (unsigned long long)p * D.R + r) * D.stride + D.tail;
                dump[n - dump_lo] = ((unsigned long long)H0 << 32) | H1;
            }
        } else if constexpr (is_first_mode(MODE)) {
            // first hit: the same wave-uniform prune, against the target's high word
            // (dump_lo carries the target); the rare slow path tests all 64 bits
            unsigned long long m = __builtin_amdgcn_ballot_w64(H0 <= wb.T);
            if (m) {
                const bool ok = lane_ok && r >= rlo && r <= rhi;
                m = __builtin_amdgcn_ballot_w64(H0 <= wb.T && ok);
                while (m) {
                    const int l = __builtin_ctzll(m);
                    m &= m - 1;
                    const uint32_t h0 = __builtin_amdgcn_readlane(H0, l);
                    const uint32_t h1 = __builtin_amdgcn_readlane(H1, l);
                    const uint32_t pl = __builtin_amdgcn_readlane(p, l);
                    const unsigned long long hh = ((unsigned long long)h0 << 32) | h1;
                    const unsigned long long nn = (D.base + (unsigned long long)pl * D.R + r) * D.stride + D.tail;
                    first_hit(hh, nn);
                }
            }
        } else if constexpr (MODE == kScanCollect) {
            // collect: MODE 2's prune; the slow path appends every lane that passes the
            // edge masks and the exact 64-bit test
            unsigned long long m = __builtin_amdgcn_ballot_w64(H0 <= wb.T);
            if (m) {
                const bool ok = lane_ok && r >= rlo && r <= rhi;
                m = collect_ballot(H0, H1, wb.T, ok);
                if (m) {
                    unsigned long long slot = collect_reserve(m);
                    while (m && collect_room(slot)) {
                        const int l = __builtin_ctzll(m);
                        m &= m - 1;
                        const uint32_t h0 = __builtin_amdgcn_readlane(H0, l);
                        const uint32_t h1 = __builtin_amdgcn_readlane(H1, l);
                        const uint32_t pl = __builtin_amdgcn_readlane(p, l);
                        const unsigned long long hh = ((unsigned long long)h0 << 32) | h1;
                        const unsigned long long nn = (D.base + (unsigned long long)pl * D.R + r) * D.stride + D.tail;
                        collect_store(slot++, hh, nn);
                    }
                }
            }
        } else if constexpr (MODE == kScanCollectBatch) {
            // collect batch: MODE 3's walk, against the current job's target, counter and list flag
            unsigned long long m = __builtin_amdgcn_ballot_w64(H0 <= wb.T);
            if (m) {
                const bool ok = lane_ok && r >= rlo && r <= rhi;
                m = collect_batch_ballot(H0, H1, wb.T, ok);
                if (m) {
                    unsigned long long slot = collect_batch_reserve(m);
                    while (m && collect_batch_room(slot)) {
                        const int l = __builtin_ctzll(m);
                        m &= m - 1;
                        const uint32_t h0 = __builtin_amdgcn_readlane(H0, l);
                        const uint32_t h1 = __builtin_amdgcn_readlane(H1, l);
                        const uint32_t pl = __builtin_amdgcn_readlane(p, l);
                        const unsigned long long hh = ((unsigned long long)h0 << 32) | h1;
                        const unsigned long long nn = (D.base + (unsigned long long)pl * D.R + r) * D.stride + D.tail;
                        collect_batch_store(slot++, hh, nn);
                    }
                }
            }
        } else {
            unsigned long long m = __builtin_amdgcn_ballot_w64(H0 <= wb.T);
            if (m) {  // wave-uniform, rare once T has settled
                const bool ok = lane_ok && r >= rlo && r <= rhi;
                m = __builtin_amdgcn_ballot_w64(H0 <= wb.T && ok);
                while (m) {
                    const int l = __builtin_ctzll(m);
                    m &= m - 1;
                    const uint32_t h0 = __builtin_amdgcn_readlane(H0, l);
                    const uint32_t h1 = __builtin_amdgcn_readlane(H1, l);
                    const uint32_t pl = __builtin_amdgcn_readlane(p, l);
                    const unsigned long long hh = ((unsigned long long)h0 << 32) | h1;
                    const unsigned long long nn = (D.base + (unsigned long long)pl * D.R + r) * D.stride + D.tail;
                    if (hh < wb.h || (hh == wb.h && nn < wb.n)) {
                        wb.h = hh;
                        wb.n = nn;
                        wb.T = h0 < wb.T ? h0 : wb.T;
                    }
                }
            }
        }
    };

    if constexpr (C2 == 2) {
        // 64 loop values per batch: wave 0 lane j builds the K+W schedule of r = rb + j
        // (row stride 68 words keeps 16-byte alignment for the broadcast reads).
        __shared__ uint4 sh_kw[64][17];
        for (uint32_t rb = r0; rb < r1; rb += 64u) {
            const uint32_t nb = r1 - rb < 64u ? r1 - rb : 64u;
            __syncthreads();  // the previous batch has been consumed by every wave
            if (threadIdx.x < nb) {
                const uint32_t r = rb + threadIdx.x;
                const uint32_t m = r / D.R1, q = r - m * D.R1;
                uint32_t w[64];
#pragma unroll
                for (int i = 0; i < 16; i++) w[i] = D.U[i];
                w[0] |= ascii4(m);
                w[1] |= (ascii4(q) & D.qmask) << D.loop_shift;
                expand_full(w);
#pragma unroll
                for (int i = 0; i < 16; i++)
                    sh_kw[threadIdx.x][i] = make_uint4(K[4 * i] + w[4 * i], K[4 * i + 1] + w[4 * i + 1],
                                                       K[4 * i + 2] + w[4 * i + 2], K[4 * i + 3] + w[4 * i + 3]);
            }
            __syncthreads();
            for (uint32_t j = 0; j < (wave_idle ? 0u : nb); j++) {
                const uint4* kr = sh_kw[j];
                uint32_t H0, H1;
                ut_hash<0, 0>(s, cv, inv0, t20, [&](int t) {   // kw from LDS: per-lane
                    const uint4 v = kr[t >> 2];
                    return (t & 3) == 0 ? v.x : (t & 3) == 1 ? v.y : (t & 3) == 2 ? v.z : v.w;
                }, H0, H1);
                finish(rb + j, H0, H1);
            }
        }
        return;
    }

#pragma unroll 1  // one nonce per iteration (unrolling x2 measured no gain, r01_variants)
    for (uint32_t r = r0; r < r1; r++) {
        GPUHASH_LOOP_ALIGN();
        uint32_t H0, H1;
        if constexpr (UT) {
            const uint32_t* __restrict__ kw = ktab + D.tab_off + 64u * r;
            ut_hash<1, 63>(s, cv, inv0, t20, [&](int t) { return kw[t]; }, H0, H1);
        } else {
            const uint32_t WJ = D.U[J] | ((ascii4(r) & D.qmask) << D.loop_shift);
            uint32_t w[64];
#pragma unroll
            for (int i = 0; i < 16; i++) w[i] = W[i];
            w[J] = WJ;
            // schedule word t, computed just before round t uses it (so only the ~16
            // words of the sliding window are live, not all 48): loop-invariant terms
            // are summed first so LICM hoists them out of the r-loop
            auto sched = [&](auto tc) {
                constexpr int t = decltype(tc)::value;
                constexpr bool d2 = kDep.v[t - 2], d7 = kDep.v[t - 7], d15 = kDep.v[t - 15], d16 = kDep.v[t - 16];
                uint32_t x2, x15;
                if constexpr (t - 2 == J) x2 = us1(w[t - 2]); else x2 = bs1(w[t - 2]);
                if constexpr (t - 15 == J) x15 = us0(w[t - 15]); else x15 = bs0(w[t - 15]);
                uint32_t inv = (d2 ? 0u : x2) + (d7 ? 0u : w[t - 7]) + (d15 ? 0u : x15) + (d16 ? 0u : w[t - 16]);
                uint32_t var = (d2 ? x2 : 0u) + (d7 ? w[t - 7] : 0u) + (d15 ? x15 : 0u) + (d16 ? w[t - 16] : 0u);
                w[t] = inv + var;
            };
            State x = s;
            {   // round J: everything but W_J is loop-invariant
                uint32_t inv = x.h + bS1(x.e) + ch(x.e, x.f, x.g) + K[J];
                uint32_t t2 = bS0(x.a) + maj(x.a, x.b, x.c);
                x.h = x.g; x.g = x.f; x.f = x.e; x.e = (x.d + inv) + WJ;
                x.d = x.c; x.c = x.b; x.b = x.a; x.a = (inv + t2) + WJ;
            }
            sfor<J + 1, 63>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                if constexpr (t < 16) {
                    round_kw(x, K[t] + w[t]);   // uniform word: K+W folds
                } else {
                    sched(tc);
                    round_kw(x, w[t] + K[t]);
                }
            });
            sched(std::integral_constant<int, 63>{});
            if constexpr (!EX) {
                // round 63: e is dead; fold CV0 into the constant so a64 + CV0 is free
                uint32_t t1 = x.h + w[63] + (K[63] + cv[0]) + ch(x.e, x.f, x.g) + bS1(x.e);
                H0 = t1 + bS0(x.a) + maj(x.a, x.b, x.c);
                H1 = cv[1] + x.a;
            } else {
                round_kw(x, w[63] + K[63]);
                State y{cv[0] + x.a, cv[1] + x.b, cv[2] + x.c, cv[3] + x.d,
                        cv[4] + x.e, cv[5] + x.f, cv[6] + x.g, cv[7] + x.h};
                const uint32_t y0 = y.a, y1 = y.b;
                sfor<0, 63>([&](auto tc) {
                    constexpr int t = decltype(tc)::value;
                    round_kw(y, D.KWX[t]);
                });
                uint32_t t1 = y.h + D.KWX[63] + ch(y.e, y.f, y.g) + bS1(y.e);
                H0 = y0 + t1 + bS0(y.a) + maj(y.a, y.b, y.c);
                H1 = y1 + y.a;
            }
        }
        finish(r, H0, H1);
    }
}

// C2 = 3 (lane table): one row = 256 consecutive values x of block B's W_0/W_1 digits,
// one per lane, x loop values r = the block B-1 digits, p = p_a + r.  Per row each lane
// builds block B's K+W schedule for its x ONCE (kept in registers: the rows of C2 = 2
// could share one schedule across a wave only because its lanes varied block B-1); per
// loop value the wave reads block B-1's chaining value and round 0's partial sums from
// the host's p-table (scalar loads) and every lane runs block B's 64 rounds, as ut_hash.
// nonce = D.base + r * D.RQ + x.
template <int MODE>
__device__ __forceinline__ void scan_row_lt(const LaunchDesc& D, uint32_t row, uint32_t r0, uint32_t r1,
                                            WaveBest& wb, unsigned long long* __restrict__ dump,
                                            unsigned long long dump_lo, const uint32_t* __restrict__ ptab) {
    using namespace dev;
    const uint32_t x = D.p_first + row * 256u + threadIdx.x;
    const bool wave_idle =
        __builtin_amdgcn_readfirstlane(D.p_first + row * 256u + (threadIdx.x & ~63u)) > D.p_last;
    if (wave_idle) return;
    const bool lane_ok = x <= D.p_last;
    uint32_t kw[64];
    {
        const uint32_t hi4 = x / D.R1, lo = x - hi4 * D.R1;
        uint32_t w[64];
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = D.U[i];
        w[0] |= ascii4(hi4);
        w[1] |= (ascii4(lo) & D.qmask) << D.loop_shift;
        expand_full(w);
#pragma unroll
        for (int t = 0; t < 64; t++) kw[t] = K[t] + w[t];
    }
#pragma unroll 1
    for (uint32_t r = r0; r < r1; r++) {
        const uint32_t* __restrict__ P = ptab + D.tab_off + 16u * r;
        uint32_t cv[8];
#pragma unroll
        for (int i = 0; i < 8; i++) cv[i] = P[i];
        const State s{cv[0], cv[1], cv[2], cv[3], cv[4], cv[5], cv[6], cv[7]};
        uint32_t H0, H1;
        ut_hash<0, 0>(s, cv, P[8], P[9], [&](int t) { return kw[t]; }, H0, H1);
#ifdef GPUHASH_TIE_TEST_BITS
        H0 >>= (32 - GPUHASH_TIE_TEST_BITS);
        H1 = 0;
#endif
        if constexpr (MODE == kScanDump) {
            if (lane_ok) dump[D.base + (unsigned long long)r * D.RQ + x - dump_lo] = ((unsigned long long)H0 << 32) | H1;
        } else if constexpr (is_first_mode(MODE)) {
            unsigned long long m = __builtin_amdgcn_ballot_w64(H0 <= wb.T);
            if (m) {  // first hit: as scan_row's MODE 2
                m = __builtin_amdgcn_ballot_w64(H0 <= wb.T && lane_ok);
                while (m) {
                    const int l = __builtin_ctzll(m);
                    m &= m - 1;
                    const uint32_t h0 = __builtin_amdgcn_readlane(H0, l);
                    const uint32_t h1 = __builtin_amdgcn_readlane(H1, l);
                    const uint32_t xl = __builtin_amdgcn_readlane(x, l);
                    const unsigned long long hh = ((unsigned long long)h0 << 32) | h1;
                    const unsigned long long nn = D.base + (unsigned long long)r * D.RQ + xl;
                    first_hit(hh, nn);
                }
            }
        } else if constexpr (MODE == kScanCollect) {
            unsigned long long m = __builtin_amdgcn_ballot_w64(H0 <= wb.T);
            if (m) {  // collect: as scan_row's MODE 3
                m = collect_ballot(H0, H1, wb.T, lane_ok);
                if (m) {
                    unsigned long long slot = collect_reserve(m);
                    while (m && collect_room(slot)) {
                        const int l = __builtin_ctzll(m);
                        m &= m - 1;
                        const uint32_t h0 = __builtin_amdgcn_readlane(H0, l);
                        const uint32_t h1 = __builtin_amdgcn_readlane(H1, l);
                        const uint32_t xl = __builtin_amdgcn_readlane(x, l);
                        const unsigned long long hh = ((unsigned long long)h0 << 32) | h1;
                        const unsigned long long nn = D.base + (unsigned long long)r * D.RQ + xl;
                        collect_store(slot++, hh, nn);
                    }
                }
            }
        } else if constexpr (MODE == kScanCollectBatch) {
            unsigned long long m = __builtin_amdgcn_ballot_w64(H0 <= wb.T);
            if (m) {  // collect batch: as scan_row's MODE 6
                m = collect_batch_ballot(H0, H1, wb.T, lane_ok);
                if (m) {
                    unsigned long long slot = collect_batch_reserve(m);
                    while (m && collect_batch_room(slot)) {
                        const int l = __builtin_ctzll(m);
                        m &= m - 1;
                        const uint32_t h0 = __builtin_amdgcn_readlane(H0, l);
                        const uint32_t h1 = __builtin_amdgcn_readlane(H1, l);
                        const uint32_t xl = __builtin_amdgcn_readlane(x, l);
                        const unsigned long long hh = ((unsigned long long)h0 << 32) | h1;
                        const unsigned long long nn = D.base + (unsigned long long)r * D.RQ + xl;
                        collect_batch_store(slot++, hh, nn);
                    }
                }
            }
        } else {
            unsigned long long m = __builtin_amdgcn_ballot_w64(H0 <= wb.T);
            if (m) {  // wave-uniform, rare once T has settled
                m = __builtin_amdgcn_ballot_w64(H0 <= wb.T && lane_ok);
                while (m) {
                    const int l = __builtin_ctzll(m);
                    m &= m - 1;
                    const uint32_t h0 = __builtin_amdgcn_readlane(H0, l);
                    const uint32_t h1 = __builtin_amdgcn_readlane(H1, l);
                    const uint32_t xl = __builtin_amdgcn_readlane(x, l);
                    const unsigned long long hh = ((unsigned long long)h0 << 32) | h1;
                    const unsigned long long nn = D.base + (unsigned long long)r * D.RQ + xl;
                    if (hh < wb.h || (hh == wb.h && nn < wb.n)) {
                        wb.h = hh;
                        wb.n = nn;
                        wb.T = h0 < wb.T ? h0 : wb.T;
                    }
                }
            }
        }
    }
}

__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// a < b for wave-uniform 64-bit values, as scalar compares of the halves.  A 64-bit less-than is a
// VALU instruction here and keeps a VGPR copy of an operand that outlives the per-nonce loop alive
// through it (the plain kernels have none to spare: at J = 13 the pair went to scratch); the empty
// asm keeps the halves from being re-joined.
__device__ __forceinline__ bool uniform_lt64(unsigned long long a, unsigned long long b) {
    uint32_t ah = (uint32_t)(a >> 32), al = (uint32_t)a, bh = (uint32_t)(b >> 32), bl = (uint32_t)b;
    asm volatile("" : "+s"(ah), "+s"(al), "+s"(bh), "+s"(bl));
    return ah < bh || (ah == bh && al < bl);
}

// Persistent scan over every launch descriptor of one kernel variant.
//
// Work = rows x loop values, linearised in "row-iterations" (one r value for a whole
// 256-lane row): descriptor i owns [offs[i], offs[i+1]).  Workgroups (a grid sized to
// the resident capacity) grab contiguous pieces with one atomicAdd -- guided
// self-scheduling: piece = clamp(remaining / (2 * grid), gmin, gmax) -- so early pieces
// amortise the per-row setup and the last ones are short, which keeps the tail of the
// launch to ~gmin iterations.  The wave-uniform best (and its pruning word) persists
// across pieces; each workgroup appends one 16-byte candidate at the end if it found one.
// Tuning hook (tools/build_variants.sh): -DGPUHASH_WAVES_PER_EU=N asks for >= N waves per
// SIMD, i.e. a VGPR budget of 512/N.  Off in the product build.
#ifdef GPUHASH_WAVES_PER_EU
#define GPUHASH_SCAN_ATTR __attribute__((amdgpu_waves_per_eu(GPUHASH_WAVES_PER_EU)))
#else
#define GPUHASH_SCAN_ATTR
#endif
template <int J, int C2, bool EX, int MODE>
__global__ __launch_bounds__(256) GPUHASH_SCAN_ATTR void k_scan(GPUHASH_SCAN_PARAMS) {
    static_assert(J >= 0 && J < 16, "loop word index");
    static_assert(!C2 || J <= 1, "C2 layouts have the loop word at J <= 1");
    static_assert(C2 != 2 || J == 1, "two-word uniform loop only with the loop word at J = 1");
    static_assert(C2 != 3 || (J == 1 && !EX), "lane table only with the loop word at J = 1");
    static_assert(!EX || J >= 13, "extra padding block only when the last digit is at byte >= 55");
    __shared__ unsigned long long sh_grab[2];
    __shared__ unsigned long long sh_best[4][2];
    const uint32_t tid = threadIdx.x;
    const unsigned long long total = offs[ndesc];

    // clock evidence: workgroup 0 (resident for the whole persistent launch) samples the
    // shader clock counter and the 100 MHz real-time counter at its start and its end,
    // into the 4 words after the group's work counter (no extra kernel argument: one
    // measurably changed the hot loop's SGPR assignment and cost 3.5%)
    unsigned long long* const clk = work + 1;
    if (blockIdx.x == 0 && tid == 0) {
        clk[0] = __builtin_amdgcn_s_memtime();
        clk[1] = __builtin_amdgcn_s_memrealtime();
    }
    WaveBest wb{~0ull, ~0ull, 0xFFFFFFFFu};
    if constexpr (MODE == kScanFirst) {  // dump_lo = the target
        wb.T = (uint32_t)(dump_lo >> 32);
        FirstState& fs = first_state();
        if (tid == 0) { fs.target = dump_lo; fs.bound = thresh; }
        if ((tid & 63u) == 0) fs.found[tid >> 6] = 0u;
        __syncthreads();
    }
    if constexpr (MODE == kScanCollect) {  // dump_lo = the target; thresh, cands, ncand: see CollectState
        wb.T = (uint32_t)(dump_lo >> 32);
        if (tid == 0) {
            CollectState& cs = collect_state();
            cs.count = thresh;
            cs.list = cands;
            cs.cap = *ncand;
            cs.target_lo = (uint32_t)dump_lo;
        }
        __syncthreads();
    }
    if constexpr (MODE == kScanBatch) {  // thresh, cands, ncand: see BatchState
        if (tid == 0) batch_arm(thresh, cands, ncand);
        __syncthreads();
    }
    if constexpr (MODE == kScanFirstBatch) {  // thresh, cands, ncand: see first_batch_flush
        FirstState& fs = first_state();
        if (tid == 0) {
            batch_arm(thresh, cands, ncand);
            fs.grab_bound = ~0ull;  // no job yet: the first part changes to one
        }
        if ((tid & 63u) == 0) fs.found[tid >> 6] = 0u;
        __syncthreads();
    }
    if constexpr (MODE == kScanCollectBatch) {  // thresh, cands, ncand: see CollectBatchState
        if (tid == 0) batch_arm(thresh, cands, ncand);  // no job yet: the first part changes to one
        __syncthreads();
    }
    for (;;) {
        // MODE 5 keeps the bound of the grab in LDS alone (grab_bound) and every wave reads it
        // back at each part: no wave may still be among the parts of the last piece when thread 0
        // overwrites it
        if constexpr (MODE == kScanFirstBatch) __syncthreads();
        if (tid == 0) {
            const unsigned long long cur = __hip_atomic_load(work, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long rem = cur < total ? total - cur : 0ull;
            unsigned long long g = rem / (2ull * gridDim.x);
            g = g < gmin ? gmin : (g > gmax ? gmax : g);
            sh_grab[0] = atomicAdd(work, g);
            sh_grab[1] = g;
            if constexpr (MODE == kScanFirst)  // the bound of this grab, broadcast with the grab itself
                first_state().grab_bound = __hip_atomic_load(thresh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if constexpr (MODE == kScanFirstBatch) {  // the same, of the job the workgroup is in
                const uint32_t cur = batch_state().job;
                if (cur != kNoJob)
                    first_state().grab_bound =
                        __hip_atomic_load(thresh + 2ull * cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
        unsigned long long x = uniform64(sh_grab[0]);
        const unsigned long long g = uniform64(sh_grab[1]);
        unsigned long long grab_bound = ~0ull;
        if constexpr (MODE == kScanFirst) grab_bound = uniform64(first_state().grab_bound);
        __syncthreads();
        unsigned long long end;
        // the same two tests, on the scalar unit (MODE 6 as well: the VGPR copy of `total` that
        // the 64-bit compares keep went to scratch at J = 7, 8, 12 and 13)
        if constexpr (MODE == kScanFirstBatch || MODE == kScanCollectBatch) {
            if (!uniform_lt64(x, total)) break;
            end = uniform_lt64(x + g, total) ? x + g : total;
        } else {
            if (x >= total) break;
            end = x + g < total ? x + g : total;
        }
        if constexpr (MODE == kScanMin) {
            const unsigned long long tv = __hip_atomic_load(thresh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t t = __builtin_amdgcn_readfirstlane((uint32_t)(tv >> 32));
            wb.T = t < wb.T ? t : wb.T;
        }
        if constexpr (MODE == kScanBatch) {  // the same, from the word of the job the workgroup is in
            const uint32_t cur = __builtin_amdgcn_readfirstlane(batch_state().job);
            if (cur != kNoJob) {
                const uint32_t t = batch_T(cur);
                wb.T = t < wb.T ? t : wb.T;
            }
        }
        // MODE 2: `thresh` holds the lowest qualifying nonce found so far by any workgroup
        // (all ones: none yet).  Thread 0 read it once, at the grab, and every wave took
        // that one value between the grab's two barriers: the skip decisions below MUST be
        // the same in all four waves, because scan_row<.., C2 = 2, ..> synchronises the
        // workgroup (its LDS batches), and a wave that loaded the word itself could see
        // another workgroup's atomicMin that its neighbours missed.
        // The bound never drops below the answer, so a part whose every nonce lies above it
        // cannot hold the answer and is skipped unhashed; every nonce below the answer is
        // still hashed, in whatever order the workgroups run.  Nothing is added per nonce:
        // work is left out only here, part by part, and (below) by taking the rest of a
        // descriptor off the work counter, on the same test.
        // The bound is held and compared as two 32-bit halves, scalar compares both: a 64-bit
        // compare is a VALU instruction here and would keep a VGPR copy of the bound alive
        // through the per-nonce loop (the empty asm keeps the halves from being re-joined).
        // (MODE 5 reads the halves back from LDS at every part instead: with MODE 4's descriptor
        // index live as well, the pair held across the loop spilled two VGPRs at J = 13.)
        uint32_t bound_hi = ~0u, bound_lo = ~0u;
        if constexpr (MODE == kScanFirst) {
            bound_hi = (uint32_t)(grab_bound >> 32);
            bound_lo = (uint32_t)grab_bound;
            asm volatile("" : "+s"(bound_hi), "+s"(bound_lo));
        }
        while (x < end) {
            int i = 0;
            if constexpr (is_batch_mode(MODE)) {  // thousands of descriptors per group: no linear walk
                i = batch_find(offs, ndesc, x);
                // held as a scalar from here on: without this LLVM moves part of the loop's
                // uniform ascii4(r) onto the VALU (+4 VALU instructions per nonce at J = 4)
                asm volatile("" : "+s"(i));
            } else {
                while (i + 1 < ndesc && offs[i + 1] <= x) i++;
            }
            const LaunchDesc& D = descs[i];
            const uint32_t rel = (uint32_t)(x - offs[i]);  // < rows * R <= 2^32 (plan.h)
            if constexpr (MODE == kScanBatch) {
                // a part of another job: leave the current one, re-arm from the new job's word
                BatchState& bs = batch_state();
                const uint32_t job = __builtin_amdgcn_readfirstlane(D.job);
                const uint32_t cur = __builtin_amdgcn_readfirstlane(bs.job);
                if (job != cur) {
                    if (cur != kNoJob) batch_flush(wb, cur, sh_best);
                    else __syncthreads();
                    if (tid == 0) bs.job = job;
                    __syncthreads();
                    wb = WaveBest{~0ull, ~0ull, batch_T(job)};
                }
            }
            if constexpr (MODE == kScanFirstBatch) {
                // a part of another job: append the hit for the current one, then the new job's
                // bound and target.  Thread 0 loads them between the barriers, the bound as at a
                // grab: ONE value for the workgroup, which every wave reads from LDS at each part.
                BatchState& bs = batch_state();
                const uint32_t job = __builtin_amdgcn_readfirstlane(D.job);
                const uint32_t cur = __builtin_amdgcn_readfirstlane(bs.job);
                if (job != cur) {
                    first_batch_flush(cur);
                    FirstState& fs = first_state();
                    if (tid == 0) {
                        unsigned long long* const words = bs.thresh + 2ull * job;
                        bs.job = job;
                        fs.bound = words;
                        fs.grab_bound = __hip_atomic_load(words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        fs.target = __hip_atomic_load(words + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                        for (int w = 0; w < 4; w++) fs.found[w] = 0u;
                    }
                    __syncthreads();
                    wb.T = __builtin_amdgcn_readfirstlane((uint32_t)(fs.target >> 32));
                }
            }
            if constexpr (MODE == kScanCollectBatch) {
                // a part of another job: nothing to flush (no per-wave state belongs to a job).
                // Thread 0 publishes the new job's counter address, target and list flag between
                // the barriers: every wave has left the old job before, and reads the new words after.
                BatchState& bs = batch_state();
                const uint32_t job = __builtin_amdgcn_readfirstlane(D.job);
                const uint32_t cur = __builtin_amdgcn_readfirstlane(bs.job);
                if (job != cur) {
                    __syncthreads();
                    CollectBatchState& cbs = collect_batch_state();
                    if (tid == 0) {
                        unsigned long long* const words = bs.thresh + (unsigned long long)kCollectJobWords * job;
                        const unsigned long long target = words[1];
                        bs.job = job;
                        cbs.count = words;
                        cbs.target_hi = (uint32_t)(target >> 32);
                        cbs.target_lo = (uint32_t)target;
                        cbs.cap = words[2] ? bs.count[2] : 0u;
                    }
                    __syncthreads();
                    wb.T = __builtin_amdgcn_readfirstlane(cbs.target_hi);
                }
            }
            const uint32_t row = rel / D.R, r0 = rel - row * D.R;
            const unsigned long long left = end - x;
            const uint32_t r1 = (unsigned long long)(D.R - r0) < left ? D.R : r0 + (uint32_t)left;
            if constexpr (is_first_mode(MODE)) {
                unsigned long long lb = part_min_nonce(D, C2, row, r0);
                if constexpr (MODE == kScanFirstBatch) {  // never below the descriptor's first nonce (plan.h)
                    const unsigned long long dl = desc_min_nonce(D, C2);
                    lb = lb < dl ? dl : lb;
                    const unsigned long long gb = uniform64(first_state().grab_bound);
                    bound_hi = (uint32_t)(gb >> 32);
                    bound_lo = (uint32_t)gb;
                }
                const uint32_t lh = (uint32_t)(lb >> 32), ll = (uint32_t)lb;
                if (lh > bound_hi || (lh == bound_hi && ll > bound_lo)) {  // lb > bound
                    if constexpr (C2 != 3) {
                        // The second way work is left out.  Within a descriptor a part's
                        // smallest nonce only grows with its position (row, then r), so every
                        // later part of this descriptor lies above the bound too: thread 0
                        // takes them off the work counter in one step, and a launch drains in
                        // a few grabs per descriptor once a hit is known.  Only
                        // positions from this part on, in this descriptor, are cancelled.
                        // At the top of uint64 part_min_nonce can wrap for a LATER part, but
                        // only where its exact value passes 2^64-1, i.e. where the part holds
                        // no nonce of the range (plan.h), so cancelling it loses nothing; this
                        // part's own value, being above the bound, has not wrapped below it.
                        const unsigned long long dend = offs[i + 1];
                        if constexpr (MODE == kScanFirstBatch) {  // and the descriptors after it that drain whole
                            if (tid < 64u) {
                                const unsigned long long far = first_batch_drain_end<C2>(descs, offs, ndesc, i);
                                if (tid == 0) atomicMax(work, far);
                            }
                        } else {
                            if (tid == 0) atomicMax(work, dend);
                        }
                        x = dend < end ? dend : end;
                    } else {
                        x += r1 - r0;  // lane table: the next row starts lower again
                    }
                    continue;
                }
            }
            if constexpr (C2 == 3) scan_row_lt<MODE>(D, row, r0, r1, wb, dump, dump_lo, ktab);
            else scan_row<J, C2, EX, MODE>(D, row, r0, r1, wb, dump, dump_lo, ktab);
            x += r1 - r0;
        }
    }

    if (blockIdx.x == 0 && tid == 0) {
        clk[2] = __builtin_amdgcn_s_memtime();
        clk[3] = __builtin_amdgcn_s_memrealtime();
    }
    if constexpr (MODE == kScanMin) {
        const uint32_t wave = tid >> 6;
        if ((tid & 63u) == 0) { sh_best[wave][0] = wb.h; sh_best[wave][1] = wb.n; }
        __syncthreads();
        if (tid == 0) {
            unsigned long long bh = sh_best[0][0], bn = sh_best[0][1];
#pragma unroll
            for (int i = 1; i < 4; i++) {
                if (sh_best[i][0] < bh || (sh_best[i][0] == bh && sh_best[i][1] < bn)) {
                    bh = sh_best[i][0];
                    bn = sh_best[i][1];
                }
            }
            if (bh != ~0ull || bn != ~0ull) {
                atomicMin(thresh, bh);
                const unsigned int idx = atomicAdd(ncand, 1u);
                cands[idx].hash = bh;
                cands[idx].nonce = bn;
            }
        }
    }
    if constexpr (MODE == kScanBatch) {  // leave the last job
        const uint32_t cur = __builtin_amdgcn_readfirstlane(batch_state().job);
        if (cur != kNoJob) batch_flush(wb, cur, sh_best);
    }
    if constexpr (MODE == kScanFirstBatch)  // leave the last job
        first_batch_flush(__builtin_amdgcn_readfirstlane(batch_state().job));
    if constexpr (MODE == kScanFirst) {
        // the workgroup's lowest-nonce hit, appended only if it has one (the host reads
        // "found" off the append counter).  The pair is stored SWAPPED, nonce in .hash, so
        // k_reduce's lexicographic minimum picks the lowest nonce.
        const FirstState& fs = first_state();
        __syncthreads();
        if (tid == 0) {
            unsigned long long bn = 0, bh = 0;
            unsigned int any = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (fs.found[i] && (!any || fs.n[i] < bn)) {
                    bn = fs.n[i];
                    bh = fs.h[i];
                    any = 1;
                }
            }
            if (any) {
                const unsigned int idx = atomicAdd(ncand, 1u);
                cands[idx].hash = bn;
                cands[idx].nonce = bh;
            }
        }
    }
}

}  // namespace gpuhash
