// gpuhash.cpp -- C-ABI host library: contexts, per-device streams, static sharding,
// launch sequencing and the host argmin.  See include/gpuhash.h for the contract and
// the reference call sites it replaces.
#include "gpuhash.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "collect.h"
#include "control.h"
#include "kernels.h"
#include "plan.h"
#include "stage.h"

using namespace gpuhash;

namespace {

// The device hit list of gpuhash_collect_below holds the kernels' Cand entries.
static_assert(sizeof(Hit) == sizeof(Cand) && offsetof(Hit, hash) == offsetof(Cand, hash) &&
                  offsetof(Hit, nonce) == offsetof(Cand, nonce),
              "collect.h's Hit is the layout of the device hit list");

struct Dev {
    int ord = -1;
    int shard = -1;        // position in gpuhash_open's device list
    int stream_dev = -1;   // ordinal the runtime reports for `stream` (hipStreamGetDevice)
    hipStream_t stream = nullptr;
    unsigned long long* d_thresh = nullptr;
    Cand* d_cands = nullptr;
    unsigned int* d_ncand = nullptr;
    Cand* d_best = nullptr;
    Cand* h_best = nullptr;  // pinned
    unsigned int* h_nhit = nullptr;  // pinned: first-hit mode's candidate count (0 = no hit)
    size_t cands_cap = 0;
    // collecting mode's hit list: allocated on the entry's first collecting call that asks
    // for a list (GPUHASH_COLLECT_MAX entries, 16 MB, unless GPUHASH_COLLECT_BUFFER says
    // otherwise), grow-only
    Cand* d_hits = nullptr;
    size_t hits_cap = 0;
    // launch descriptors + prefix offsets + per-launch work counters, staged through a
    // pinned host buffer and copied once per call
    uint8_t* d_meta = nullptr;
    uint8_t* h_meta = nullptr;
    size_t meta_cap = 0, h_meta_cap = 0;
    // uniform K+W tables of C2/J=0 descriptors (one per digit count), grow-only
    uint32_t* d_ktab = nullptr;
    size_t ktab_cap = 0;  // words
    // pinned copy of the per-group work counters + clock samples (kCounterBytes each)
    unsigned long long* h_clk = nullptr;
    size_t clk_cap = 0;  // words
    std::vector<hipEvent_t> ev;
    hipEvent_t done = nullptr;  // blocking-sync event: the end of a call's work (host_wait)
    // the control side (control.h): a second stream that never carries a kernel, for the copies
    // that must run while a persistent grid holds the device -- the drain word onto the stage's
    // work counters, and the counters back for gpuhash_progress
    Control* ctl = nullptr;          // the context's
    hipStream_t ctl_stream = nullptr;
    uint8_t* h_prog = nullptr;       // pinned, kControlCopyBytes: the head of d_meta, for progress
    hipEvent_t uploaded = nullptr;   // on `stream`, after the stage upload: the control copies wait for it
    hipEvent_t prog_done = nullptr;  // on ctl_stream, after a progress copy
    int wait_mode = 0;          // HostWait
    // per-call results
    int rc = GPUHASH_OK;
    uint64_t best_h = ~0ull, best_n = ~0ull;
    bool found = false;  // first-hit mode: (best_h, best_n) is a hit
    uint64_t hit_count = 0;  // collecting mode: qualifying nonces of the shard, exact
    std::vector<Hit> hits;   // collecting mode: all of them, unordered, if the list held them all
    // batch mode: the run's result list as it came back, and its fold, one (hash, nonce) per job
    // of the run
    std::vector<BatchEntry> bat_list;
    std::vector<uint64_t> bat_h, bat_n;
    std::vector<uint8_t> bat_found;  // first-hit batch: the job has an entry
    // collect batch: the ONE list its listing jobs share (GPUHASH_COLLECT_MAX BatchEntry, 24 MB,
    // unless GPUHASH_COLLECT_BUFFER says otherwise), allocated on the entry's first batch with a
    // listing job, grow-only; and the jobs' exact hit counters as they came back (bat_list then
    // holds the first min(appended, capacity) entries of the list)
    BatchEntry* d_blist = nullptr;
    size_t blist_cap = 0;
    std::vector<uint64_t> bat_counts;
    bool used = false;
    double kernel_ms = 0;
    uint32_t launches = 0;
    std::vector<gpuhash_launch_record> recs;

    void reset() {  // before every batch of a call (Call::run)
        rc = GPUHASH_OK;
        found = used = false;
        hit_count = launches = 0;
        kernel_ms = 0;
        hits.clear();
        recs.clear();
    }
};

}  // namespace

struct gpuhash_ctx {
    // One search at a time per context (a miner runs one job at a time, p1.pdf p.13);
    // concurrent callers, e.g. several goroutines sharing an Engine, are serialised here.
    std::mutex mu;
    std::vector<Dev> devs;
    std::unique_ptr<Control> ctl;  // cancel latch and progress mailbox: used without `mu`
    int policy = kLayoutAuto;
    gpuhash_stats last{};
    std::vector<gpuhash_launch_record> recs;
};

// Restores the calling thread's current HIP device on scope exit.  The ABI runs device
// work on the caller's thread for single-device contexts, and a host sharing that thread
// (a cgo-locked goroutine, a torch process on another device) must not find its current
// device changed by a gpuhash call.
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

#define HIPCHK(expr)                                \
    do {                                            \
        if ((expr) != hipSuccess) return GPUHASH_EHIP; \
    } while (0)

// Runs f() for an ABI entry point: no C++ exception crosses the C ABI into a Go or Python host.
template <class F>
static int guarded(F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return GPUHASH_ENOMEM;
    } catch (...) {
        return GPUHASH_EHIP;
    }
}

// How the host waits for a call's work (GPUHASH_HOST_WAIT, read at gpuhash_open):
//   poll    (default) hipEventQuery on a completion event: back to back for the first
//           0.5 ms (short calls return at once), then every 100 us with the thread asleep
//   stream  hipStreamSynchronize on the device's stream
//   event   hipEventSynchronize on the event, created with hipEventBlockingSync
// A miner spends almost all its life inside this wait (a 2^34-nonce job is ~0.5 s of GPU
// time, ~4 s with 8 miners on one GPU).  On this ROCm both `stream` and `event` keep the
// waiting thread running: 8 miners sharing one MI355X burned 1.0 host core each (8 of the
// box's 16-CPU quota), `poll` 0.007 core each, at the same GPU throughput and the same
// bench GH/s (tools/host_wait_probe.py, profiles/r05_host_wait.jsonl).
enum HostWait { kWaitPoll = 0, kWaitStream = 1, kWaitEvent = 2 };

static int host_wait_mode() {
    const char* e = std::getenv("GPUHASH_HOST_WAIT");
    if (e && !std::strcmp(e, "stream")) return kWaitStream;
    if (e && !std::strcmp(e, "event")) return kWaitEvent;
    return kWaitPoll;
}

// While it polls, the waiting thread also serves the context's control side (control.h): it
// drains the stage's work counters once when the cancel latch is seen, and answers progress
// requests from a copy of those counters.  Both are copies on the entry's control stream, which
// never carries a kernel, enqueued only after the host has seen the stage's upload complete (the
// upload zeroes the counters) and ordered after nothing else.  They are kControlCopyBytes long at
// least, because that is what makes the runtime hand them to a copy engine, which runs beside
// the persistent grid; a shorter copy is a shader blit and waits for the grid (control.h).
// The drain is therefore the head of the pinned metadata image, uploaded again with the drain
// word in the counters: the prefix offsets and descriptors it rewrites are the bytes already
// there, and what else it touches -- the clock words, the p-table room, a batch's per-job words
// and list -- only feeds results, which a cancelled call discards; no index or bound is among
// them but a list's head, which it sets back to empty.
// Nothing is enqueued unless somebody cancelled or asked.  `stream` and `event` do not poll: there
// the latch is honoured and progress known at launch boundaries only.
static int poll_wait(Dev& d, const Stage& st) {
    Control& C = *d.ctl;
    const size_t slot = (size_t)d.shard, ng = st.groups.size();
    // both buffers hold max(their stage bytes, kControlCopyBytes) at least (stage_upload), and a
    // stage's bytes include every counter block
    const size_t drain_bytes = std::max(kControlCopyBytes, kCounterBytes * ng);
    bool drained = false, copying = false;
    uint64_t ticket = 0;
    C.poll_enter(slot);
    int rc = GPUHASH_OK;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipEventQuery(d.done);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) { rc = GPUHASH_EHIP; break; }
        const bool asked = !copying && (ticket = C.wanted(slot)) != 0;
        const bool cancel = !drained && C.observe();
        if ((cancel || asked) && hipEventQuery(d.uploaded) != hipSuccess) {
            // the stage has not begun (entries that share a device run one after the other): none
            // of its work is handed out, and its drain has to wait for the upload
            if (asked) C.publish(slot, ticket, 0);
        } else if (cancel || asked) {
            if (cancel) {
                drained = true;  // one drain per stage: later groups find their counters drained
                for (const StageGroup& G : st.groups) std::memcpy(d.h_meta + G.work_at, &kDrainWord, sizeof kDrainWord);
                if (hipStreamWaitEvent(d.ctl_stream, d.uploaded, 0) != hipSuccess ||
                    hipMemcpyAsync(d.d_meta, d.h_meta, drain_bytes, hipMemcpyHostToDevice, d.ctl_stream) != hipSuccess) {
                    rc = GPUHASH_EHIP;
                    break;
                }
            }
            if (asked) {
                if (hipStreamWaitEvent(d.ctl_stream, d.uploaded, 0) != hipSuccess ||
                    hipMemcpyAsync(d.h_prog, d.d_meta, kControlCopyBytes, hipMemcpyDeviceToHost, d.ctl_stream) != hipSuccess ||
                    hipEventRecord(d.prog_done, d.ctl_stream) != hipSuccess) {
                    rc = GPUHASH_EHIP;
                    break;
                }
                copying = true;
            }
        } else if (copying) {
            const hipError_t p = hipEventQuery(d.prog_done);
            if (p == hipSuccess) {
                uint64_t part = 0;  // a group whose counter lies past the copy counts when the stage is over
                for (const StageGroup& G : st.groups) {
                    if (G.work_at + sizeof(uint64_t) > kControlCopyBytes) break;
                    uint64_t counter;
                    std::memcpy(&counter, d.h_prog + G.work_at, sizeof counter);
                    part = sat_add(part, handed_out(G.nonces, counter, G.total));
                }
                C.publish(slot, ticket, part);
                copying = false;
            } else if (p != hipErrorNotReady) { rc = GPUHASH_EHIP; break; }
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(500))
            std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
    C.poll_exit(slot);
    // no control copy outlives the stage it was aimed at: the next upload reuses these bytes
    if ((drained || copying) && hipStreamSynchronize(d.ctl_stream) != hipSuccess) rc = GPUHASH_EHIP;
    return rc;
}

static int host_wait(Dev& d, const Stage& st) {
    if (d.wait_mode == kWaitStream) {
        HIPCHK(hipStreamSynchronize(d.stream));
        return GPUHASH_OK;
    }
    HIPCHK(hipEventRecord(d.done, d.stream));
    if (d.wait_mode == kWaitEvent) {
        HIPCHK(hipEventSynchronize(d.done));
        return GPUHASH_OK;
    }
    return poll_wait(d, st);
}

static int dev_init(Dev& d, int ord, int shard, Control* ctl) {
    d.ord = ord;
    d.shard = shard;
    d.ctl = ctl;
    DeviceGuard guard;
    HIPCHK(hipSetDevice(ord));
    HIPCHK(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
    hipDevice_t sd = -1;
    HIPCHK(hipStreamGetDevice(d.stream, &sd));
    if (sd != ord) return GPUHASH_EHIP;  // the stream must live on the device it serves
    d.stream_dev = sd;
    d.wait_mode = host_wait_mode();
    HIPCHK(hipEventCreateWithFlags(&d.done, hipEventBlockingSync | hipEventDisableTiming));
    if (hipMalloc(&d.d_thresh, sizeof(unsigned long long)) != hipSuccess) return GPUHASH_ENOMEM;
    if (hipMalloc(&d.d_ncand, sizeof(unsigned int)) != hipSuccess) return GPUHASH_ENOMEM;
    if (hipMalloc(&d.d_best, sizeof(Cand)) != hipSuccess) return GPUHASH_ENOMEM;
    if (hipHostMalloc(&d.h_best, sizeof(Cand), hipHostMallocDefault) != hipSuccess) return GPUHASH_ENOMEM;
    if (hipHostMalloc(&d.h_nhit, sizeof(unsigned int), hipHostMallocDefault) != hipSuccess) return GPUHASH_ENOMEM;
    HIPCHK(hipMemset(d.d_ncand, 0, sizeof(unsigned int)));
    // The control stream takes the highest stream priority: the runtime maps the streams of one
    // priority onto a few hardware queues that they share, and a copy on a stream that shares its
    // queue with a stream whose grid is resident (this context's, or another's in the process)
    // waits for that grid.  No kernel ever runs at this priority, so no such queue holds one.
    int least = 0, greatest = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHK(hipStreamCreateWithPriority(&d.ctl_stream, hipStreamNonBlocking, greatest));
    HIPCHK(hipEventCreateWithFlags(&d.uploaded, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&d.prog_done, hipEventDisableTiming));
    if (hipHostMalloc(&d.h_prog, kControlCopyBytes, hipHostMallocDefault) != hipSuccess) return GPUHASH_ENOMEM;
    return GPUHASH_OK;
}

static void dev_free(Dev& d) {
    if (d.ord < 0) return;
    DeviceGuard guard;
    hipSetDevice(d.ord);
    if (d.stream) hipStreamSynchronize(d.stream);
    if (d.ctl_stream) hipStreamSynchronize(d.ctl_stream);
    for (auto e : d.ev) hipEventDestroy(e);
    d.ev.clear();
    if (d.done) hipEventDestroy(d.done);
    if (d.uploaded) hipEventDestroy(d.uploaded);
    if (d.prog_done) hipEventDestroy(d.prog_done);
    if (d.h_prog) hipHostFree(d.h_prog);
    if (d.ctl_stream) hipStreamDestroy(d.ctl_stream);
    if (d.d_thresh) hipFree(d.d_thresh);
    if (d.d_ncand) hipFree(d.d_ncand);
    if (d.d_best) hipFree(d.d_best);
    if (d.d_cands) hipFree(d.d_cands);
    if (d.d_hits) hipFree(d.d_hits);
    if (d.d_blist) hipFree(d.d_blist);
    if (d.h_best) hipHostFree(d.h_best);
    if (d.h_nhit) hipHostFree(d.h_nhit);
    if (d.d_meta) hipFree(d.d_meta);
    if (d.d_ktab) hipFree(d.d_ktab);
    if (d.h_clk) hipHostFree(d.h_clk);
    if (d.h_meta) hipHostFree(d.h_meta);
    if (d.stream) hipStreamDestroy(d.stream);
    d = Dev{};
}

// An entry's buffers only grow: room for n elements, on the device or pinned on the host.
template <class T>
static int grow(T*& p, size_t& cap, size_t n, bool pinned = false) {
    if (n <= cap) return GPUHASH_OK;
    if (p) pinned ? hipHostFree(p) : hipFree(p);
    p = nullptr;
    cap = 0;
    if ((pinned ? hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, n * sizeof(T))) != hipSuccess)
        return GPUHASH_ENOMEM;
    cap = n;
    return GPUHASH_OK;
}

// What one device run is asked for.
struct ScanJob {
    ScanMode mode = kScanMin;
    uint64_t target = 0;                   // kScanFirst, kScanCollect: hashes <= target qualify
    uint32_t collect_cap = 0;              // kScanCollect: hit-list entries asked for (0: count only)
    unsigned long long* d_dump = nullptr;  // kScanDump: device array for the range's hashes
};

// How a mode uses the words the kernels share: the one statement of it on the host (kernels.h's
// ScanArgs and the phases of dev_run refer here).  Unless a flag says otherwise, d_thresh is a
// bound that only falls, armed to all ones (kScanMin: the pruning threshold); d_ncand is the
// append counter of d_cands, armed to 0; dump_lo is the range's first nonce (kScanDump: the
// nonce of dump[0]); and d_best comes back in h_best.
struct ModeWiring {
    // d_thresh is the 64-bit hit counter, armed to 0, and comes back in h_best->hash, instead
    // of d_best.  d_ncand is the list's capacity (collect_cap; 0: count only), which the
    // kernels only read.  cands is d_hits; after the wait its `count` entries are copied if
    // they all fitted (count <= collect_cap): a list that overflowed is merely some of the
    // hits, which the collector discards (collect.h).
    bool collects;
    bool takes_target;  // dump_lo is the target
    // d_thresh is the lowest qualifying nonce found so far.  The workgroups append only real
    // hits, nonce and hash swapped, so the same reduce picks the lowest nonce, and d_best comes
    // back swapped.  The append counter, copied to h_nhit before the reduce, is the found flag.
    bool first_hit;
    bool reduces;  // k_reduce folds d_cands into d_best
    // The mode's words live in the metadata buffer, where the stage's fill() arms them (stage.h):
    // thresh is the array of per-job pruning words, cands the result list (BatchEntry) and ncand
    // the list's head, whose append counter comes back in h_nhit.  After the wait that many
    // entries are copied and folded per job by the (hash, nonce) key.  d_thresh, d_cands, d_ncand
    // and d_best are not used.
    bool batch;
    // A batch whose per-job words are pairs, {the lowest qualifying nonce found so far, the job's
    // target}, in a stage whose launches ascend in digits (stage.h, Stage::by_digits).  The list
    // holds real hits only and is folded per job by the LOWEST NONCE; a job without an entry has
    // no hit.
    bool batch_first;
    // A batch whose per-job words are triples, {the job's exact hit counter, armed to 0; its
    // target; whether it lists}, in a job-major stage (stage.h, Stage::collects).  cands is the
    // entry's d_blist, one list for all listing jobs, and the head's append counter is 64 bits
    // wide: it comes back in h_best->hash.  After the wait the per-job words and the first
    // min(appended, capacity) entries are copied; collect.h's fold_collect_batch makes every
    // job's answer of them.
    bool batch_collect;
};
// The packed group of a batch stage (stage.h, C2 = 4) is no mode of its own: k_pack reads the same
// per-job words, list and list head as the scan kernels of the stage's mode, kScanBatch or
// kScanCollectBatch, and everything after the launch is that mode's.  Likewise k_pack_first under
// kScanFirstBatch (a round of gpuhash_first_below_batch_early).
constexpr ModeWiring kWiring[] = {
    /* kScanMin     */ {false, false, false, true},
    /* kScanDump    */ {false, false, false, false},
    /* kScanFirst   */ {false, true, true, true},
    /* kScanCollect */ {true, true, false, false},
    /* kScanBatch   */ {false, false, false, false, true},
    /* kScanFirstBatch */ {false, false, false, false, true, true},
    /* kScanCollectBatch */ {false, false, false, false, true, false, true},
};

// dev_run, phase 1: reserves the entry's buffers, writes and uploads the launch metadata in one
// copy, and has the device build the tables.  grids[g] = workgroups of group g.
static int stage_upload(Dev& d, const Stage& st, const ScanJob& job, std::vector<unsigned int>& grids) {
    // both metadata buffers hold kControlCopyBytes at least: a drain copies that much (poll_wait)
    const size_t ng = st.groups.size(), meta = std::max<size_t>(st.bytes, kControlCopyBytes);
    int rc;
    const size_t host_meta = std::max<size_t>(st.upload_bytes, kControlCopyBytes);  // a batch's list is the device's alone
    if ((rc = grow(d.d_meta, d.meta_cap, meta)) || (rc = grow(d.h_meta, d.h_meta_cap, host_meta, true))) return rc;
    st.fill(d.h_meta);
    size_t sumgrid = 0;
    grids.reserve(ng);
    for (const StageGroup& g : st.groups) {
        const unsigned int resident = g.C2 != 4                      ? grid_for(g.J, g.C2, g.EX, job.mode, d.ord)
                                      : job.mode == kScanFirstBatch ? pack_first_grid_for(d.ord)
                                                                    : pack_grid_for(job.mode, d.ord);
        if (resident == 0) return GPUHASH_EHIP;
        // a batch stage's list bound assumes at most kBatchMaxGrid workgroups (stage.h)
        grids.push_back(Stage::grid(g, st.njobs ? std::min<unsigned int>(resident, kBatchMaxGrid) : resident));
        sumgrid += grids.back();
    }
    // every workgroup of every group may append one candidate before the single reduce
    if ((rc = grow(d.d_cands, d.cands_cap, std::max<size_t>(sumgrid, 1))) ||
        (rc = grow(d.d_ktab, d.ktab_cap, st.tab_words)) || (rc = grow(d.d_hits, d.hits_cap, job.collect_cap)) ||
        (rc = grow(d.h_clk, d.clk_cap, kCounterBytes / 8 * std::max<size_t>(ng, 8), true)))
        return rc;
    if (st.collects && std::any_of(st.lists.begin(), st.lists.end(), [](uint8_t l) { return l != 0; }))
        if ((rc = grow(d.d_blist, d.blist_cap, st.list_cap))) return rc;
    while (d.ev.size() < 2 * ng) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        d.ev.push_back(e);
    }
    HIPCHK(hipMemcpyAsync(d.d_meta, d.h_meta, st.upload_bytes, hipMemcpyHostToDevice, d.stream));
    HIPCHK(hipEventRecord(d.uploaded, d.stream));  // the counters are zeroed: a drain may follow (poll_wait)
    for (const StageTab& t : st.tabs)
        HIPCHK(launch_ktab(reinterpret_cast<const LaunchDesc*>(d.d_meta + t.desc_byte), d.d_ktab + t.off,
                           t.R, d.stream));
    // lane-table groups: their launches' p-tables, one device thread per block B-1 value
    // (on the host these compressions cost ~0.16 us each, ~7% of a search whose loop
    // values cover only 10^5 lane values each)
    for (const StageGroup& g : st.groups)
        if (g.C2 == 3)
            HIPCHK(launch_ptab(reinterpret_cast<const LaunchDesc*>(d.d_meta + g.desc_at), (int)g.idx.size(),
                               reinterpret_cast<uint32_t*>(d.d_meta + g.ptab_at), d.stream));
    return GPUHASH_OK;
}

// dev_run, phase 2: arms the shared words as kWiring says and launches the groups.
// Groups run back to back on the device's stream (each launch's HIP events then time
// that kernel alone, which bench.py's roofline relies on).  Running the small groups
// on a second stream was measured: a persistent grid launched beside another is not
// fully dispatched until the other drains, so its events span the whole call, for
// <= 0.3% less wall time.  All groups append to one candidate list (atomic counter,
// shared pruning threshold); one reduce at the end folds it.
static int arm_and_launch(Dev& d, const Stage& st, const ScanJob& job, uint64_t lo,
                          const std::vector<unsigned int>& grids) {
    const ModeWiring w = kWiring[job.mode];
    if (!w.batch) {
        HIPCHK(hipMemsetAsync(d.d_thresh, w.collects ? 0 : 0xFF, sizeof(unsigned long long), d.stream));
        HIPCHK(hipMemsetAsync(d.d_best, 0xFF, sizeof(Cand), d.stream));
        if (w.collects)  // every call sets the capacity anew
            HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d.d_ncand), (int)job.collect_cap, 1, d.stream));
        else
            HIPCHK(hipMemsetAsync(d.d_ncand, 0, sizeof(unsigned int), d.stream));
    }
    for (size_t g = 0; g < st.groups.size(); g++) {
        const StageGroup& G = st.groups[g];
        ScanArgs a{};
        a.stream = d.stream;
        a.descs = reinterpret_cast<const LaunchDesc*>(d.d_meta + G.desc_at);
        a.offs = reinterpret_cast<const unsigned long long*>(d.d_meta + G.offs_at);
        a.ndesc = (int)G.idx.size();
        a.work = reinterpret_cast<unsigned long long*>(d.d_meta + G.work_at);
        a.gmin = st.gmin;
        a.gmax = st.gmax;
        a.thresh = d.d_thresh;
        a.cands = w.collects ? d.d_hits : d.d_cands;
        a.ncand = d.d_ncand;
        if (w.batch) {
            a.thresh = reinterpret_cast<unsigned long long*>(d.d_meta + st.thresh_at);
            a.cands = reinterpret_cast<Cand*>(d.d_meta + st.list_at + kBatchListHead);
            a.ncand = reinterpret_cast<unsigned int*>(d.d_meta + st.list_at);
            if (w.batch_collect) a.cands = reinterpret_cast<Cand*>(d.d_blist);  // null: no job lists
        }
        a.dump = job.d_dump;
        a.dump_lo = w.takes_target ? job.target : lo;
        a.ktab = G.C2 == 3 ? reinterpret_cast<const uint32_t*>(d.d_meta + G.ptab_at) : d.d_ktab;
        a.grid = grids[g];
        HIPCHK(hipEventRecord(d.ev[2 * g], a.stream));
        if (G.C2 == 4) {  // the packed group: its tables instead of descriptors (pack.h)
            const PackArgs p{d.stream, d.d_meta + st.pack_recs_at, d.d_meta + st.pack_segs_at, d.d_meta + st.pack_tiles_at,
                             G.total, a.work, a.thresh, reinterpret_cast<BatchEntry*>(a.cands), a.ncand, a.grid};
            // a first-hit batch stage's packed group is a round of gpuhash_first_below_batch_early
            HIPCHK(job.mode == kScanFirstBatch ? launch_pack_first(p) : launch_pack(job.mode, p));
        } else {
            HIPCHK(launch_scan(G.J, G.C2, G.EX, job.mode, a));
        }
        HIPCHK(hipEventRecord(d.ev[2 * g + 1], a.stream));
    }
    return GPUHASH_OK;
}

// dev_run, phase 3: the reduce, the copies back, the call's one wait and the launch records.
static int read_back(Dev& d, const Stage& st, const ScanJob& job, uint64_t lo, uint64_t hi) {
    const ModeWiring w = kWiring[job.mode];
    if (w.first_hit)
        HIPCHK(hipMemcpyAsync(d.h_nhit, d.d_ncand, sizeof(unsigned int), hipMemcpyDeviceToHost, d.stream));
    if (w.batch_collect)  // the 64-bit append counter, into the pinned h_best->hash
        HIPCHK(hipMemcpyAsync(d.h_best, d.d_meta + st.list_at, sizeof(unsigned long long), hipMemcpyDeviceToHost, d.stream));
    else if (w.batch)
        HIPCHK(hipMemcpyAsync(d.h_nhit, d.d_meta + st.list_at, sizeof(unsigned int), hipMemcpyDeviceToHost, d.stream));
    if (w.reduces) HIPCHK(launch_reduce(d.d_cands, d.d_ncand, d.d_best, d.stream));
    // d_best, or the hit counter alone, which lands in the pinned h_best->hash
    const void* result = w.collects ? (const void*)d.d_thresh : d.d_best;
    const size_t result_bytes = w.collects ? sizeof(unsigned long long) : sizeof(Cand);
    if (!w.batch) HIPCHK(hipMemcpyAsync(d.h_best, result, result_bytes, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(hipMemcpyAsync(d.h_clk, d.d_meta, kCounterBytes * st.groups.size(), hipMemcpyDeviceToHost, d.stream));
    if (int rc = host_wait(d, st)) return rc;
    // whatever the wait brought back is discarded once the call has seen the latch
    if (d.ctl->observe()) return GPUHASH_ECANCELED;
    uint64_t stage_nonces = 0;
    for (const StageGroup& G : st.groups) stage_nonces = sat_add(stage_nonces, G.nonces);
    d.ctl->stage_done((size_t)d.shard, stage_nonces);
    for (size_t g = 0; g < st.groups.size(); g++) {
        const StageGroup& G = st.groups[g];
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, d.ev[2 * g], d.ev[2 * g + 1]));
        d.kernel_ms += ms;
        const unsigned long long* c = d.h_clk + (kCounterBytes / 8) * g + 1;
        const double ticks = (double)(c[2] - c[0]), rt = (double)(c[3] - c[1]);
        const double sclk = rt > 0 ? ticks / rt * 100.0 : 0.0;  // s_memrealtime runs at 100 MHz
        d.recs.push_back(gpuhash_launch_record{d.ord, G.J, G.C2, G.EX, G.d, G.c, d.shard, d.stream_dev, lo, hi,
                                               G.nonces, (double)ms, sclk});
    }
    d.launches += (uint32_t)st.groups.size();  // an entry may run several stages between two resets
    return GPUHASH_OK;
}

// dev_run, phase 4: the entry's results from what came back.
static int decode(Dev& d, const ScanJob& job, const Stage& st) {
    if (kWiring[job.mode].batch_collect) {
        // the entries past the list's end were counted, not stored; a run without a listing job
        // has no list at all (and appended nothing)
        const size_t n = d.d_blist ? (size_t)std::min<uint64_t>(d.h_best->hash, st.list_cap) : 0;
        std::vector<uint64_t> words(kCollectJobWords * st.njobs);
        d.bat_list.resize(n);
        if (n)
            HIPCHK(hipMemcpyAsync(d.bat_list.data(), d.d_blist, n * sizeof(BatchEntry), hipMemcpyDeviceToHost, d.stream));
        HIPCHK(hipMemcpyAsync(words.data(), d.d_meta + st.thresh_at, words.size() * sizeof(uint64_t),
                              hipMemcpyDeviceToHost, d.stream));
        HIPCHK(hipStreamSynchronize(d.stream));
        d.bat_counts.resize(st.njobs);
        for (size_t k = 0; k < st.njobs; k++) d.bat_counts[k] = words[kCollectJobWords * k];
        return GPUHASH_OK;
    }
    if (kWiring[job.mode].batch) {
        const size_t n = *d.h_nhit;
        if (n > st.list_cap) return GPUHASH_EHIP;  // the bound is proved (stage.h): not reached
        d.bat_list.resize(n);
        if (n) {
            HIPCHK(hipMemcpyAsync(d.bat_list.data(), d.d_meta + st.list_at + kBatchListHead, n * sizeof(BatchEntry),
                                  hipMemcpyDeviceToHost, d.stream));
            HIPCHK(hipStreamSynchronize(d.stream));
        }
        d.bat_h.assign(st.njobs, ~0ull);
        d.bat_n.assign(st.njobs, ~0ull);
        d.bat_found.assign(st.njobs, 0);
        const bool first = kWiring[job.mode].batch_first;
        for (const BatchEntry& e : d.bat_list) {
            if (e.job >= st.njobs) return GPUHASH_EHIP;
            uint64_t &h = d.bat_h[e.job], &x = d.bat_n[e.job];
            if (first) {  // the lowest nonce; 2^64-1 is a legal one, so the flag says "any"
                if (!d.bat_found[e.job] || e.nonce < x) { h = e.hash; x = e.nonce; }
                d.bat_found[e.job] = 1;
            } else if (e.hash < h || (e.hash == h && e.nonce < x)) {
                h = e.hash;
                x = e.nonce;
            }
        }
        return GPUHASH_OK;
    }
    if (kWiring[job.mode].collects) {
        d.hit_count = d.h_best->hash;
        const size_t n = d.hit_count <= job.collect_cap ? (size_t)d.hit_count : 0;
        if (n) {
            d.hits.resize(n);
            HIPCHK(hipMemcpyAsync(d.hits.data(), d.d_hits, n * sizeof(Cand), hipMemcpyDeviceToHost, d.stream));
            HIPCHK(hipStreamSynchronize(d.stream));
        }
        return GPUHASH_OK;
    }
    d.best_h = d.h_best->hash;
    d.best_n = d.h_best->nonce;
    if (kWiring[job.mode].first_hit) {
        d.found = *d.h_nhit > 0;
        std::swap(d.best_h, d.best_n);
    }
    return GPUHASH_OK;
}

// Runs one device's shard [lo, hi] of a job.  The stage groups the planned launches by kernel
// variant; each group is ONE persistent launch over all its descriptors (scan_kernel.h).
static int dev_run(Dev& d, const uint8_t* msg, size_t len, uint64_t lo, uint64_t hi, uint32_t rchunk,
                   int policy, const ScanJob& job) {
    d.used = true;
    DeviceGuard guard;
    HIPCHK(hipSetDevice(d.ord));
    const Stage st(msg, len, lo, hi, rchunk, policy);
    std::vector<unsigned int> grids;
    int rc = stage_upload(d, st, job, grids);
    if (!rc) rc = arm_and_launch(d, st, job, lo, grids);
    if (!rc) rc = read_back(d, st, job, lo, hi);
    return rc ? rc : decode(d, job, st);
}

// Runs one entry's run of a sub-batch: the jobs [first, end) of `jobs`, whose plans are moved
// into the stage; index0 is the batch index of jobs[0], for the launch records.
// target: null for gpuhash_min_batch, else the targets of jobs[0..) for gpuhash_first_below_batch
// and, with lists (whether each of jobs[0..) lists) and the entry's list capacity `buffer`, for
// gpuhash_collect_below_batch.  index_of: null, or the batch index of every position index0 + k
// where the jobs are a selection of the batch's (gpuhash_first_below_batch_early): the launch
// records then carry the batch indices of the run's first and last job.
static int dev_run_batch(Dev& d, std::vector<PlannedJob>& jobs, size_t first, size_t end, size_t index0,
                         uint32_t rchunk, const uint64_t* target = nullptr, const uint8_t* lists = nullptr,
                         uint64_t buffer = 0, const size_t* index_of = nullptr) {
    d.used = true;
    DeviceGuard guard;
    HIPCHK(hipSetDevice(d.ord));
    StageJobs sj(jobs, first, end);
    std::vector<std::vector<Launch>>& plans = sj.plans;
    const Stage st = lists    ? Stage(plans, target + first, lists + first, buffer, rchunk, sj.which())
                     : target ? Stage(plans, target + first, rchunk, sj.which())
                              : Stage(plans, rchunk, sj.which());
    const ScanJob job{lists ? kScanCollectBatch : target ? kScanFirstBatch : kScanBatch};
    std::vector<unsigned int> grids;
    int rc = stage_upload(d, st, job, grids);
    if (!rc) rc = arm_and_launch(d, st, job, 0, grids);
    const size_t lo = index0 + first, hi = index0 + end - 1;
    if (!rc) rc = read_back(d, st, job, index_of ? index_of[lo] : lo, index_of ? index_of[hi] : hi);
    return rc ? rc : decode(d, job, st);
}

// One ABI call: its device runs, batch by batch, and its statistics and launch records, which
// finish() publishes.  A batch: sub-ranges that run concurrently, each on its own context entry.
struct Call {
    gpuhash_ctx* ctx;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    gpuhash_stats st{};

    // total: the call's nonce count, saturating (gpuhash_progress)
    Call(gpuhash_ctx* c, uint64_t total) : ctx(c) {
        ctx->recs.clear();
        ctx->ctl->begin_call(total);
    }
    ~Call() { ctx->ctl->end_call(); }
    Call(const Call&) = delete;
    Call& operator=(const Call&) = delete;

    // The cancel latch, read at call entry and before every run of the entries (run_each): every
    // slice, sub-batch and collector re-run.
    bool cancelled() { return ctx->ctl->observe(); }

    // Runs `job` over the batch: on the caller's thread when it is one sub-range, else each on a
    // host thread of its own.  Takes the entries' records and times; returns the first failure.
    int run(const uint8_t* msg, size_t msg_len, uint32_t rchunk, const std::vector<SubRange>& batch,
            const ScanJob& job) {
        return run_each(batch.size(), [&](size_t k) {  // nothing may escape a std::thread (std::terminate)
            const SubRange& s = batch[k];
            Dev& d = ctx->devs[(size_t)s.shard];
            d.rc = guarded([&] { return dev_run(d, msg, msg_len, s.lo, s.hi, rchunk, ctx->policy, job); });
        });
    }

    // Runs one(k) for k < n, each a device run on a context entry of its own that leaves its
    // return code in that entry's rc: on the caller's thread when n is 1, else each on a host
    // thread of its own.
    template <class F>
    int run_each(size_t n, F&& one) {
        if (cancelled()) return GPUHASH_ECANCELED;
        for (auto& d : ctx->devs) d.reset();
        if (n == 1) {
            one((size_t)0);
        } else {
            std::vector<std::thread> th;
            th.reserve(n);
            // Thread creation can fail (std::system_error): the shards already started are
            // joined before the error is returned, so no joinable std::thread is destroyed.
            int spawn_rc = GPUHASH_OK;
            for (size_t k = 0; k < n && spawn_rc == GPUHASH_OK; k++)
                spawn_rc = guarded([&] {
                    th.emplace_back([&, k] { one(k); });
                    return GPUHASH_OK;
                });
            for (auto& t : th) t.join();
            if (spawn_rc) return spawn_rc;
        }
        double batch_max = 0;
        uint32_t used = 0;
        for (auto& d : ctx->devs) {
            if (!d.used) continue;
            if (d.rc) return d.rc;
            ctx->recs.insert(ctx->recs.end(), d.recs.begin(), d.recs.end());
            st.launches += d.launches;
            st.kernel_ms += d.kernel_ms;
            batch_max = std::max(batch_max, d.kernel_ms);
            used++;
        }
        st.max_dev_kernel_ms += batch_max;  // the entries of a batch run concurrently
        st.ndevices = std::max(st.ndevices, used);
        return GPUHASH_OK;
    }

    // The call examined the nonces [first, last].
    void finish(uint64_t first, uint64_t last) {
        const uint64_t span = last - first;
        finish_nonces(span == ~0ull ? ~0ull : span + 1);
    }

    void finish_nonces(uint64_t nonces) {
        st.nonces = nonces;
        st.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        ctx->last = st;
    }
};

extern "C" {

static int open_impl(const int* devices, int ndevices, gpuhash_ctx** out);

int gpuhash_open(const int* devices, int ndevices, gpuhash_ctx** out) {
    if (!out || ndevices < 0 || (ndevices > 0 && !devices)) return GPUHASH_EINVAL;
    *out = nullptr;
    return guarded([&] { return open_impl(devices, ndevices, out); });
}

static int open_impl(const int* devices, int ndevices, gpuhash_ctx** out) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return GPUHASH_ENODEV;
    std::vector<int> ords;
    if (ndevices == 0) {
        for (int i = 0; i < count; i++) ords.push_back(i);
    } else {
        // A device may be listed more than once: each entry gets its own stream and
        // buffers and takes its own shard (rehearses the multi-device path on one GPU).
        for (int i = 0; i < ndevices; i++) {
            if (devices[i] < 0 || devices[i] >= count) return GPUHASH_EINVAL;
            ords.push_back(devices[i]);
        }
    }
    for (int o : ords) {  // the code object is gfx950-only
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, o) != hipSuccess) return GPUHASH_ENODEV;
        if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0) return GPUHASH_ENODEV;
    }
    auto* raw = new (std::nothrow) gpuhash_ctx();
    if (!raw) return GPUHASH_ENOMEM;
    // frees whatever was set up if a device fails to initialise or an allocation throws
    std::unique_ptr<gpuhash_ctx, void (*)(gpuhash_ctx*)> ctx(raw, [](gpuhash_ctx* c) {
        for (auto& d : c->devs) dev_free(d);
        delete c;
    });
    ctx->devs.resize(ords.size());
    ctx->ctl.reset(new Control(ords.size()));
    for (size_t i = 0; i < ords.size(); i++) {
        int rc = dev_init(ctx->devs[i], ords[i], (int)i, ctx->ctl.get());
        if (rc) return rc;
    }
    *out = ctx.release();
    return GPUHASH_OK;
}

int gpuhash_ndevices(const gpuhash_ctx* ctx) { return ctx ? (int)ctx->devs.size() : 0; }

int gpuhash_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 0) return 0;
    return count;
}

static bool valid_policy(int policy) {
    const int base = policy & 15, flags = policy & ~15;
    return base >= GPUHASH_LAYOUT_AUTO && base <= GPUHASH_LAYOUT_LANETABLE &&
           !(flags & ~(GPUHASH_LAYOUT_TAIL_ALWAYS | GPUHASH_LAYOUT_TAIL_NEVER | GPUHASH_LAYOUT_PACKED_ALWAYS)) &&
           (flags & ~GPUHASH_LAYOUT_PACKED_ALWAYS) != (GPUHASH_LAYOUT_TAIL_ALWAYS | GPUHASH_LAYOUT_TAIL_NEVER);
}

int gpuhash_shard_range(size_t msg_len, uint64_t lower, uint64_t upper, int nshards,
                        uint64_t* out_lower, uint64_t* out_upper) {
    return gpuhash_shard_range_policy(msg_len, lower, upper, nshards, GPUHASH_LAYOUT_AUTO, out_lower, out_upper);
}

int gpuhash_shard_range_policy(size_t msg_len, uint64_t lower, uint64_t upper, int nshards, int policy,
                               uint64_t* out_lower, uint64_t* out_upper) {
    if (nshards < 1 || !out_lower || !out_upper || lower > upper || !valid_policy(policy)) return GPUHASH_EINVAL;
    if (msg_len > GPUHASH_MAX_MSG) return GPUHASH_ETOOLONG;
    return guarded([&] {
        // the same cost model and cut points as gpuhash_min's in-process shards under the
        // same layout policy (the cuts depend on it)
        const std::vector<Shard> sh = shard_range(msg_len, lower, upper, nshards, policy);
        int used = 0;
        for (int k = 0; k < nshards; k++) {
            const Shard& s = sh[(size_t)k];
            out_lower[k] = s.empty ? 1 : s.lo;
            out_upper[k] = s.empty ? 0 : s.hi;
            used += s.empty ? 0 : 1;
        }
        return used;
    });
}

int gpuhash_set_layout_policy(gpuhash_ctx* ctx, int policy) {
    if (!ctx || !valid_policy(policy)) return GPUHASH_EINVAL;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->policy = policy;
    return GPUHASH_OK;
}

// The nonces of the inclusive [lower, upper], saturating.
static uint64_t span_of(uint64_t lower, uint64_t upper) {
    const uint64_t s = upper - lower;
    return s == ~0ull ? ~0ull : s + 1;
}

// The sum of a batch's spans, saturating.
static uint64_t spans_of(size_t njobs, const uint64_t* lower, const uint64_t* upper) {
    uint64_t n = 0;
    for (size_t k = 0; k < njobs; k++) n = sat_add(n, upper[k] - lower[k] + 1);  // <= GPUHASH_BATCH_MAX_SPAN each
    return n;
}

// The slice loop of gpuhash_min_ex and gpuhash_first_below_ex (kScanFirst, where out_found is
// set and the loop stops after the first slice that has a hit).  Searches longer than a slice
// (stage.h, slice_width) run as consecutive slices, each sharded over the context's devices,
// with a host argmin over the per-device 16-byte results.
static int search(gpuhash_ctx* ctx, const uint8_t* msg, size_t msg_len, uint64_t lower, uint64_t upper,
                  uint32_t rchunk, const ScanJob& job, uint64_t* out_hash, uint64_t* out_nonce,
                  int* out_found) {
    std::lock_guard<std::mutex> lock(ctx->mu);
    Call call(ctx, span_of(lower, upper));
    if (call.cancelled()) return GPUHASH_ECANCELED;
    const uint64_t slice = slice_width(ctx->devs.size());
    const bool first = job.mode == kScanFirst;
    uint64_t bh = ~0ull, bn = ~0ull;
    bool any = false;  // first hit: a hit exists
    std::vector<SubRange> batch;
    for (uint64_t lo = lower;;) {
        const uint64_t hi = upper - lo < slice ? upper : lo + (slice - 1);
        batch.clear();
        split_slice(msg_len, lo, hi, (int)ctx->devs.size(), ctx->policy, batch);
        if (int rc = call.run(msg, msg_len, rchunk, batch, job)) return rc;
        for (const Dev& d : ctx->devs) {
            if (!d.used || (first && !d.found)) continue;
            // first hit: the lowest nonce wins; else the lowest (hash, nonce)
            const bool less = first ? d.best_n < bn : d.best_h < bh || (d.best_h == bh && d.best_n < bn);
            if (!any || less) { bh = d.best_h; bn = d.best_n; }
            any = true;
        }
        if (hi == upper || (first && any)) break;
        lo = hi + 1;
    }
    // first hit: what an ascending scan would have examined
    call.finish(lower, first && any ? bn : upper);
    if (first) {
        *out_found = any ? 1 : 0;
        if (!any) return GPUHASH_OK;  // outputs untouched
    }
    *out_hash = bh;
    *out_nonce = bn;
    return GPUHASH_OK;
}

int gpuhash_min_ex(gpuhash_ctx* ctx, const uint8_t* msg, size_t msg_len, uint64_t lower,
                   uint64_t upper, uint32_t rchunk, uint64_t* out_hash, uint64_t* out_nonce) {
    if (!ctx || !out_hash || !out_nonce || (msg_len && !msg)) return GPUHASH_EINVAL;
    if (lower > upper) return GPUHASH_EINVAL;
    if (msg_len > GPUHASH_MAX_MSG) return GPUHASH_ETOOLONG;
    return guarded([&] { return search(ctx, msg, msg_len, lower, upper, rchunk, ScanJob{}, out_hash, out_nonce, nullptr); });
}

int gpuhash_first_below_ex(gpuhash_ctx* ctx, const uint8_t* msg, size_t msg_len, uint64_t lower,
                           uint64_t upper, uint64_t target, uint32_t rchunk, uint64_t* out_hash,
                           uint64_t* out_nonce, int* out_found) {
    if (!ctx || !out_hash || !out_nonce || !out_found || (msg_len && !msg)) return GPUHASH_EINVAL;
    if (lower > upper) return GPUHASH_EINVAL;
    if (msg_len > GPUHASH_MAX_MSG) return GPUHASH_ETOOLONG;
    return guarded([&] {
        return search(ctx, msg, msg_len, lower, upper, rchunk, ScanJob{kScanFirst, target}, out_hash, out_nonce, out_found);
    });
}

int gpuhash_first_below(gpuhash_ctx* ctx, const uint8_t* msg, size_t msg_len, uint64_t lower,
                        uint64_t upper, uint64_t target, uint64_t* out_hash, uint64_t* out_nonce,
                        int* out_found) {
    return gpuhash_first_below_ex(ctx, msg, msg_len, lower, upper, target, 0, out_hash, out_nonce, out_found);
}

// The list capacity of collecting calls: GPUHASH_COLLECT_BUFFER overrides the device list's
// entries (tests use it to reach the overflow paths on oracle-sized ranges).
static uint32_t collect_buffer() {
    const uint64_t env = env_u64("GPUHASH_COLLECT_BUFFER");
    return env ? (uint32_t)std::min<uint64_t>(env, GPUHASH_COLLECT_MAX) : GPUHASH_COLLECT_MAX;
}

// gpuhash_collect_below_ex: search()'s slices and shards, with collect.h's collector between
// the device runs and the outputs.  A slice's shards run concurrently, one per context entry;
// a re-run of an overflowed sub-range runs alone, on its shard's entry.
static int collect(gpuhash_ctx* ctx, const uint8_t* msg, size_t msg_len, uint64_t lower, uint64_t upper,
                   uint64_t target, uint32_t rchunk, uint64_t* out_nonces, uint64_t* out_hashes, size_t cap,
                   uint64_t* out_total) {
    std::lock_guard<std::mutex> lock(ctx->mu);
    Call call(ctx, span_of(lower, upper));
    if (call.cancelled()) return GPUHASH_ECANCELED;
    const uint32_t buffer = collect_buffer();
    auto split = [&](uint64_t lo, uint64_t hi, std::vector<SubRange>& batch) {
        split_slice(msg_len, lo, hi, (int)ctx->devs.size(), ctx->policy, batch);
    };
    auto run = [&](const std::vector<SubRange>& batch, bool want_list, std::vector<SubResult>& res) -> int {
        const ScanJob job{kScanCollect, target, want_list ? buffer : 0u};
        if (int rc = call.run(msg, msg_len, rchunk, batch, job)) return rc;
        for (size_t k = 0; k < batch.size(); k++) {
            Dev& d = ctx->devs[(size_t)batch[k].shard];
            res[k].count = d.hit_count;
            res[k].hits = std::move(d.hits);
            d.hits.clear();
        }
        return GPUHASH_OK;
    };
    Collector<decltype(run), decltype(split)> c(buffer, cap, run, split);
    if (int rc = c.collect(lower, upper, slice_width(ctx->devs.size()))) return rc;
    call.finish(lower, upper);  // every nonce is hashed: no early exit
    for (size_t i = 0; i < c.held.size(); i++) {
        out_nonces[i] = c.held[i].nonce;
        out_hashes[i] = c.held[i].hash;
    }
    *out_total = c.total;
    return GPUHASH_OK;
}

int gpuhash_collect_below_ex(gpuhash_ctx* ctx, const uint8_t* msg, size_t msg_len, uint64_t lower,
                             uint64_t upper, uint64_t target, uint32_t rchunk, uint64_t* out_nonces,
                             uint64_t* out_hashes, size_t cap, uint64_t* out_total) {
    if (!ctx || !out_total || (msg_len && !msg)) return GPUHASH_EINVAL;
    if (cap > GPUHASH_COLLECT_MAX || (cap > 0 && (!out_nonces || !out_hashes))) return GPUHASH_EINVAL;
    if (lower > upper) return GPUHASH_EINVAL;
    if (msg_len > GPUHASH_MAX_MSG) return GPUHASH_ETOOLONG;
    return guarded([&] {
        return collect(ctx, msg, msg_len, lower, upper, target, rchunk, out_nonces, out_hashes, cap, out_total);
    });
}

int gpuhash_collect_below(gpuhash_ctx* ctx, const uint8_t* msg, size_t msg_len, uint64_t lower,
                          uint64_t upper, uint64_t target, uint64_t* out_nonces, uint64_t* out_hashes,
                          size_t cap, uint64_t* out_total) {
    return gpuhash_collect_below_ex(ctx, msg, msg_len, lower, upper, target, 0, out_nonces, out_hashes, cap,
                                    out_total);
}

// gpuhash_min_batch_ex, its arguments checked: the sub-batches (stage.h, for_each_sub_batch),
// each cut into one run per context entry, which run concurrently.
static int min_batch(gpuhash_ctx* ctx, const uint8_t* msgs, const size_t* msg_off, size_t njobs,
                     const uint64_t* lower, const uint64_t* upper, uint32_t rchunk, uint64_t* out_hashes,
                     uint64_t* out_nonces) {
    std::lock_guard<std::mutex> lock(ctx->mu);
    Call call(ctx, spans_of(njobs, lower, upper));
    if (call.cancelled()) return GPUHASH_ECANCELED;
    std::vector<uint64_t> rh(njobs), rn(njobs);  // the outputs are written only when all ran
    const int policy = ctx->policy;
    auto plan = [&](size_t k) {
        const size_t len = msg_off[k + 1] - msg_off[k];
        const BatchJob j{len ? msgs + msg_off[k] : nullptr, len, lower[k], upper[k]};
        return packs(policy, j.lo, j.hi) ? plan_packed_job(j) : plan_job(j, rchunk, policy);
    };
    auto run = [&](size_t first, std::vector<PlannedJob>& jobs) -> int {
        const std::vector<std::pair<size_t, size_t>> runs = batch_runs(jobs, ctx->devs.size());
        const int rc = call.run_each(runs.size(), [&](size_t r) {
            Dev& d = ctx->devs[r];
            d.rc = guarded([&] { return dev_run_batch(d, jobs, runs[r].first, runs[r].second, first, rchunk); });
        });
        if (rc) return rc;
        for (size_t r = 0; r < runs.size(); r++) {
            const Dev& d = ctx->devs[r];
            for (size_t k = runs[r].first; k < runs[r].second; k++) {
                rh[first + k] = d.bat_h[k - runs[r].first];
                rn[first + k] = d.bat_n[k - runs[r].first];
            }
        }
        return GPUHASH_OK;
    };
    if (int rc = for_each_sub_batch(njobs, batch_bytes_bound(), plan, run)) return rc;
    uint64_t nonces = 0;
    for (size_t k = 0; k < njobs; k++) {
        const uint64_t n = upper[k] - lower[k] + 1;  // <= GPUHASH_BATCH_MAX_SPAN
        nonces = nonces + n < nonces ? ~0ull : nonces + n;
    }
    call.finish_nonces(nonces);
    std::copy(rh.begin(), rh.end(), out_hashes);
    std::copy(rn.begin(), rn.end(), out_nonces);
    return GPUHASH_OK;
}

int gpuhash_min_batch_ex(gpuhash_ctx* ctx, const uint8_t* msgs, const size_t* msg_off, size_t njobs,
                         const uint64_t* lower, const uint64_t* upper, uint32_t rchunk, uint64_t* out_hashes,
                         uint64_t* out_nonces) {
    if (!ctx || !msg_off || !lower || !upper || !out_hashes || !out_nonces) return GPUHASH_EINVAL;
    if (njobs == 0 || njobs > GPUHASH_BATCH_MAX_JOBS) return GPUHASH_EINVAL;
    bool too_long = false;
    for (size_t k = 0; k < njobs; k++) {
        if (msg_off[k + 1] < msg_off[k] || lower[k] > upper[k]) return GPUHASH_EINVAL;
        if (upper[k] - lower[k] >= GPUHASH_BATCH_MAX_SPAN) return GPUHASH_EINVAL;
        too_long = too_long || msg_off[k + 1] - msg_off[k] > GPUHASH_MAX_MSG;
    }
    if (!msgs && msg_off[njobs] != msg_off[0]) return GPUHASH_EINVAL;
    if (too_long) return GPUHASH_ETOOLONG;
    return guarded([&] { return min_batch(ctx, msgs, msg_off, njobs, lower, upper, rchunk, out_hashes, out_nonces); });
}

int gpuhash_min_batch(gpuhash_ctx* ctx, const uint8_t* msgs, const size_t* msg_off, size_t njobs,
                      const uint64_t* lower, const uint64_t* upper, uint64_t* out_hashes, uint64_t* out_nonces) {
    return gpuhash_min_batch_ex(ctx, msgs, msg_off, njobs, lower, upper, 0, out_hashes, out_nonces);
}

// The body gpuhash_first_below_batch_ex and the remainder of gpuhash_first_below_batch_early
// share: the first-hit searches of n jobs over [lower[i], upper[i]] with target[i], as min_batch's
// sub-batches and runs, each run one first-hit batch stage (stage.h, Stage::by_digits) and one
// launch per group of it.  Job i is job sel[i] of the call's batch (sel null: job i), which names
// its message and, in the launch records, its index.  rh, rn and rf take the results, by i.
static int first_batch_runs(Call& call, const uint8_t* msgs, const size_t* msg_off, const size_t* sel, size_t n,
                            const uint64_t* lower, const uint64_t* upper, const uint64_t* target, uint32_t rchunk,
                            uint64_t* rh, uint64_t* rn, uint8_t* rf) {
    gpuhash_ctx* const ctx = call.ctx;
    const int policy = ctx->policy;
    auto plan = [&](size_t i) {
        const size_t k = sel ? sel[i] : i, len = msg_off[k + 1] - msg_off[k];
        return plan_job(BatchJob{len ? msgs + msg_off[k] : nullptr, len, lower[i], upper[i]}, rchunk, policy,
                        /*host_ptab=*/false, /*pair=*/true);
    };
    auto run = [&](size_t first, std::vector<PlannedJob>& jobs) -> int {
        const std::vector<std::pair<size_t, size_t>> runs = batch_runs(jobs, ctx->devs.size());
        const int rc = call.run_each(runs.size(), [&](size_t r) {
            Dev& d = ctx->devs[r];
            d.rc = guarded([&] {
                return dev_run_batch(d, jobs, runs[r].first, runs[r].second, first, rchunk, target + first, nullptr, 0,
                                     sel);
            });
        });
        if (rc) return rc;
        for (size_t r = 0; r < runs.size(); r++) {
            const Dev& d = ctx->devs[r];
            for (size_t k = runs[r].first; k < runs[r].second; k++) {
                rh[first + k] = d.bat_h[k - runs[r].first];
                rn[first + k] = d.bat_n[k - runs[r].first];
                rf[first + k] = d.bat_found[k - runs[r].first];
            }
        }
        return GPUHASH_OK;
    };
    return for_each_sub_batch(n, batch_bytes_bound(), plan, run);
}

// What an ascending scan of every job would have examined (gpuhash_last_stats().nonces of the
// first-hit batches), then the outputs: a job that is not found leaves its two untouched.
static void first_batch_finish(Call& call, size_t njobs, const uint64_t* lower, const uint64_t* upper,
                               const std::vector<uint64_t>& rh, const std::vector<uint64_t>& rn,
                               const std::vector<uint8_t>& rf, uint64_t* out_hashes, uint64_t* out_nonces,
                               int* out_found) {
    uint64_t nonces = 0;
    for (size_t k = 0; k < njobs; k++) {
        const uint64_t n = (rf[k] ? rn[k] : upper[k]) - lower[k] + 1;  // <= GPUHASH_BATCH_MAX_SPAN
        nonces = nonces + n < nonces ? ~0ull : nonces + n;
    }
    call.finish_nonces(nonces);
    for (size_t k = 0; k < njobs; k++) {
        out_found[k] = rf[k] ? 1 : 0;
        if (!rf[k]) continue;  // its outputs stay untouched
        out_hashes[k] = rh[k];
        out_nonces[k] = rn[k];
    }
}

// gpuhash_first_below_batch_ex, its arguments checked.
static int first_below_batch(gpuhash_ctx* ctx, const uint8_t* msgs, const size_t* msg_off, size_t njobs,
                             const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                             uint32_t rchunk, uint64_t* out_hashes, uint64_t* out_nonces, int* out_found) {
    std::lock_guard<std::mutex> lock(ctx->mu);
    Call call(ctx, spans_of(njobs, lower, upper));
    if (call.cancelled()) return GPUHASH_ECANCELED;
    std::vector<uint64_t> rh(njobs), rn(njobs);  // the outputs are written only when all ran
    std::vector<uint8_t> rf(njobs);
    if (int rc = first_batch_runs(call, msgs, msg_off, nullptr, njobs, lower, upper, target, rchunk, rh.data(),
                                  rn.data(), rf.data()))
        return rc;
    first_batch_finish(call, njobs, lower, upper, rh, rn, rf, out_hashes, out_nonces, out_found);
    return GPUHASH_OK;
}

// One context entry's packed phase of gpuhash_first_below_batch_early: the jobs `mine` (batch
// indices, ascending), which it alone reads and writes, in ascending rounds of doubling pieces
// (include/gpuhash.h).  A round is one first-hit batch stage per sub-batch that holds the packed
// group and nothing else; a job with an entry is answered by its lowest nonce and closed, every
// other job's front advances by its piece.  used[k] counts the nonces of job k handed out so far.
struct EarlyJobs {
    const uint8_t* msgs;
    const size_t* msg_off;
    const uint64_t *lower, *target;
    const uint64_t* limit;
    const PackJob* recs;  // by batch index: built once per call
    uint64_t *used, *rh, *rn;
    uint8_t* rf;
};

static int early_rounds(Dev& d, const EarlyJobs& J, const std::vector<size_t>& mine, uint64_t c0, uint32_t rchunk) {
    const uint64_t bound = batch_bytes_bound();
    std::vector<size_t> open;
    std::vector<BatchJob> piece;
    std::vector<uint64_t> tg;
    for (uint64_t c = c0;; c = early_next_chunk(c)) {
        open.clear();
        piece.clear();
        tg.clear();
        for (size_t k : mine) {
            if (J.rf[k] || J.used[k] >= J.limit[k]) continue;
            const uint64_t lo = J.lower[k] + J.used[k], len = J.msg_off[k + 1] - J.msg_off[k];
            open.push_back(k);
            piece.push_back(BatchJob{len ? J.msgs + J.msg_off[k] : nullptr, len, lo,
                                     lo + (std::min(c, J.limit[k] - J.used[k]) - 1), J.recs + k});
            tg.push_back(J.target[k]);
        }
        if (open.empty()) return GPUHASH_OK;
        auto plan = [&](size_t i) {
            PlannedJob p = plan_packed_job(piece[i]);
            p.bytes += 8;  // its per-job words are a pair
            return p;
        };
        auto run = [&](size_t first, std::vector<PlannedJob>& jobs) -> int {
            if (d.ctl->observe()) return GPUHASH_ECANCELED;  // before every round and every sub-batch
            if (int rc = dev_run_batch(d, jobs, 0, jobs.size(), first, rchunk, tg.data() + first, nullptr, 0, open.data()))
                return rc;
            for (size_t i = 0; i < jobs.size(); i++) {
                const size_t k = open[first + i];
                if (!d.bat_found[i]) continue;
                J.rf[k] = 1;
                J.rh[k] = d.bat_h[i];
                J.rn[k] = d.bat_n[i];
            }
            return GPUHASH_OK;
        };
        if (int rc = for_each_sub_batch(open.size(), bound, plan, run)) return rc;
        for (size_t i = 0; i < open.size(); i++) J.used[open[i]] += piece[i].hi - piece[i].lo + 1;
    }
}

// gpuhash_first_below_batch_early, its arguments checked: the packed rounds of every job's front,
// each context entry over a contiguous run of the jobs that have one, then first_batch_runs over
// what is left of the jobs still open.
static int first_below_batch_early(gpuhash_ctx* ctx, const uint8_t* msgs, const size_t* msg_off, size_t njobs,
                                   const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                                   uint64_t prefix, uint32_t rchunk, uint64_t* out_hashes, uint64_t* out_nonces,
                                   int* out_found) {
    std::lock_guard<std::mutex> lock(ctx->mu);
    Call call(ctx, spans_of(njobs, lower, upper));
    if (call.cancelled()) return GPUHASH_ECANCELED;
    std::vector<uint64_t> rh(njobs), rn(njobs), limit(njobs), used(njobs, 0);
    std::vector<uint8_t> rf(njobs);
    std::vector<size_t> fronts;
    for (size_t k = 0; k < njobs; k++) {
        limit[k] = early_limit(lower[k], upper[k], target[k], prefix);
        if (limit[k]) fronts.push_back(k);
    }
    if (!fronts.empty()) {
        std::vector<PackJob> recs(njobs);
        for (size_t k : fronts) {
            const size_t len = msg_off[k + 1] - msg_off[k];
            recs[k] = PackTables::record(len ? msgs + msg_off[k] : nullptr, len);
        }
        const EarlyJobs J{msgs, msg_off, lower, target, limit.data(), recs.data(), used.data(), rh.data(), rn.data(), rf.data()};
        const uint64_t c0 = early_first_chunk(fronts.size());
        const size_t nruns = std::min(ctx->devs.size(), fronts.size());
        std::vector<std::vector<size_t>> mine(nruns);
        for (size_t r = 0; r < nruns; r++)
            mine[r].assign(fronts.begin() + (long)(fronts.size() * r / nruns),
                           fronts.begin() + (long)(fronts.size() * (r + 1) / nruns));
        const int rc = call.run_each(nruns, [&](size_t r) {
            Dev& d = ctx->devs[r];
            d.rc = guarded([&] { return early_rounds(d, J, mine[r], c0, rchunk); });
        });
        if (rc) return rc;
    }
    std::vector<size_t> sel;
    std::vector<uint64_t> lo2, hi2, tg2;
    for (size_t k = 0; k < njobs; k++) {
        if (rf[k] || used[k] > upper[k] - lower[k]) continue;  // answered, or its front was all of it
        sel.push_back(k);
        lo2.push_back(lower[k] + used[k]);
        hi2.push_back(upper[k]);
        tg2.push_back(target[k]);
    }
    if (!sel.empty()) {
        std::vector<uint64_t> h2(sel.size()), n2(sel.size());
        std::vector<uint8_t> f2(sel.size());
        if (int rc = first_batch_runs(call, msgs, msg_off, sel.data(), sel.size(), lo2.data(), hi2.data(), tg2.data(),
                                      rchunk, h2.data(), n2.data(), f2.data()))
            return rc;
        for (size_t i = 0; i < sel.size(); i++) {
            rf[sel[i]] = f2[i];
            rh[sel[i]] = h2[i];
            rn[sel[i]] = n2[i];
        }
    }
    first_batch_finish(call, njobs, lower, upper, rh, rn, rf, out_hashes, out_nonces, out_found);
    return GPUHASH_OK;
}

// The whole-call argument errors of the first-hit batches: 0, or the error.
static int first_batch_args(const gpuhash_ctx* ctx, const uint8_t* msgs, const size_t* msg_off, size_t njobs,
                            const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                            const uint64_t* out_hashes, const uint64_t* out_nonces, const int* out_found) {
    if (!ctx || !msg_off || !lower || !upper || !target || !out_hashes || !out_nonces || !out_found)
        return GPUHASH_EINVAL;
    if (njobs == 0 || njobs > GPUHASH_BATCH_MAX_JOBS) return GPUHASH_EINVAL;
    bool too_long = false;
    for (size_t k = 0; k < njobs; k++) {
        if (msg_off[k + 1] < msg_off[k] || lower[k] > upper[k]) return GPUHASH_EINVAL;
        if (upper[k] - lower[k] >= GPUHASH_BATCH_MAX_SPAN) return GPUHASH_EINVAL;
        too_long = too_long || msg_off[k + 1] - msg_off[k] > GPUHASH_MAX_MSG;
    }
    if (!msgs && msg_off[njobs] != msg_off[0]) return GPUHASH_EINVAL;
    return too_long ? GPUHASH_ETOOLONG : GPUHASH_OK;
}

int gpuhash_first_below_batch_ex(gpuhash_ctx* ctx, const uint8_t* msgs, const size_t* msg_off, size_t njobs,
                                 const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                                 uint32_t rchunk, uint64_t* out_hashes, uint64_t* out_nonces, int* out_found) {
    if (int rc = first_batch_args(ctx, msgs, msg_off, njobs, lower, upper, target, out_hashes, out_nonces, out_found))
        return rc;
    return guarded([&] {
        return first_below_batch(ctx, msgs, msg_off, njobs, lower, upper, target, rchunk, out_hashes, out_nonces,
                                 out_found);
    });
}

int gpuhash_first_below_batch_early(gpuhash_ctx* ctx, const uint8_t* msgs, const size_t* msg_off, size_t njobs,
                                    const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                                    uint64_t prefix, uint32_t rchunk, uint64_t* out_hashes, uint64_t* out_nonces,
                                    int* out_found) {
    if (prefix > GPUHASH_BATCH_MAX_SPAN) return GPUHASH_EINVAL;
    if (int rc = first_batch_args(ctx, msgs, msg_off, njobs, lower, upper, target, out_hashes, out_nonces, out_found))
        return rc;
    return guarded([&] {
        return first_below_batch_early(ctx, msgs, msg_off, njobs, lower, upper, target, prefix, rchunk, out_hashes,
                                       out_nonces, out_found);
    });
}

int gpuhash_first_below_batch(gpuhash_ctx* ctx, const uint8_t* msgs, const size_t* msg_off, size_t njobs,
                              const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                              uint64_t* out_hashes, uint64_t* out_nonces, int* out_found) {
    return gpuhash_first_below_batch_ex(ctx, msgs, msg_off, njobs, lower, upper, target, 0, out_hashes, out_nonces,
                                        out_found);
}

// A re-run of one job of a collect batch: the job alone on context entry `shard`, through the
// path gpuhash_collect_below takes (the Collector over [lo, hi], one shard, cap), which splits a
// range that alone overflows the list.  Every launch record of it carries lo == hi == index.
static int collect_alone(Call& call, int shard, size_t index, const uint8_t* msg, size_t msg_len, uint64_t lo,
                         uint64_t hi, uint64_t target, uint32_t rchunk, uint32_t buffer, size_t cap, JobHits& out) {
    gpuhash_ctx* const ctx = call.ctx;
    const size_t recs0 = ctx->recs.size();
    auto split = [&](uint64_t a, uint64_t b, std::vector<SubRange>& batch) { batch.push_back(SubRange{a, b, shard}); };
    auto run = [&](const std::vector<SubRange>& batch, bool want_list, std::vector<SubResult>& res) -> int {
        const ScanJob job{kScanCollect, target, want_list ? buffer : 0u};
        if (int rc = call.run(msg, msg_len, rchunk, batch, job)) return rc;
        for (size_t k = 0; k < batch.size(); k++) {
            Dev& d = ctx->devs[(size_t)batch[k].shard];
            res[k].count = d.hit_count;
            res[k].hits = std::move(d.hits);
            d.hits.clear();
        }
        return GPUHASH_OK;
    };
    Collector<decltype(run), decltype(split)> c(buffer, cap, run, split);
    const int rc = c.collect(lo, hi, slice_width(1));
    for (size_t i = recs0; i < ctx->recs.size(); i++) ctx->recs[i].lo = ctx->recs[i].hi = index;
    out.total = c.total;
    out.held = std::move(c.held);
    return rc;
}

// gpuhash_collect_below_batch_ex, its arguments checked: min_batch's sub-batches and runs, each run
// one collect batch stage (stage.h, Stage::collects) and one launch per group of it; then
// collect.h's fold_collect_batch per run, whose re-runs follow the sub-batch on the run's entry.
static int collect_below_batch(gpuhash_ctx* ctx, const uint8_t* msgs, const size_t* msg_off, size_t njobs,
                               const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                               uint32_t rchunk, const size_t* out_off, uint64_t* out_nonces, uint64_t* out_hashes,
                               uint64_t* out_totals) {
    std::lock_guard<std::mutex> lock(ctx->mu);
    Call call(ctx, spans_of(njobs, lower, upper));
    if (call.cancelled()) return GPUHASH_ECANCELED;
    const uint32_t buffer = collect_buffer();
    std::vector<JobHits> res(njobs);  // the outputs are written only when all ran
    std::vector<size_t> caps(njobs, 0);
    std::vector<uint8_t> lists(njobs, 0);
    for (size_t k = 0; out_off && k < njobs; k++) {
        caps[k] = out_off[k + 1] - out_off[k];
        lists[k] = caps[k] ? 1 : 0;
    }
    const int policy = ctx->policy;
    auto message = [&](size_t k, size_t& len) {
        len = msg_off[k + 1] - msg_off[k];
        return len ? msgs + msg_off[k] : nullptr;
    };
    auto plan = [&](size_t k) {
        size_t len;
        const uint8_t* const m = message(k, len);
        const BatchJob j{m, len, lower[k], upper[k]};
        if (packs(policy, j.lo, j.hi)) return plan_packed_job(j, /*collects=*/true);
        return plan_job(j, rchunk, policy, /*host_ptab=*/false, /*pair=*/false, /*collects=*/true);
    };
    auto run = [&](size_t first, std::vector<PlannedJob>& jobs) -> int {
        const std::vector<std::pair<size_t, size_t>> runs = batch_runs(jobs, ctx->devs.size());
        const int rc = call.run_each(runs.size(), [&](size_t r) {
            Dev& d = ctx->devs[r];
            d.rc = guarded([&] {
                return dev_run_batch(d, jobs, runs[r].first, runs[r].second, first, rchunk, target + first,
                                     lists.data() + first, buffer);
            });
        });
        if (rc) return rc;
        // a re-run resets every entry: take what the runs brought back first
        std::vector<std::vector<BatchEntry>> list(runs.size());
        std::vector<std::vector<uint64_t>> counts(runs.size());
        for (size_t r = 0; r < runs.size(); r++) {
            list[r] = std::move(ctx->devs[r].bat_list);
            counts[r] = std::move(ctx->devs[r].bat_counts);
            ctx->devs[r].bat_list.clear();
            ctx->devs[r].bat_counts.clear();
        }
        for (size_t r = 0; r < runs.size(); r++) {
            const size_t k0 = first + runs[r].first, n = runs[r].second - runs[r].first;
            if (counts[r].size() != n) return GPUHASH_EHIP;
            auto rerun = [&](size_t j, size_t cap, JobHits& out) {
                const size_t k = k0 + j;
                size_t len;
                const uint8_t* const m = message(k, len);
                return collect_alone(call, (int)r, k, m, len, lower[k], upper[k], target[k], rchunk, buffer, cap, out);
            };
            if (int frc = fold_collect_batch(n, counts[r].data(), list[r].data(), list[r].size(), caps.data() + k0,
                                             GPUHASH_EHIP, rerun, res.data() + k0))
                return frc;
        }
        return GPUHASH_OK;
    };
    if (int rc = for_each_sub_batch(njobs, batch_bytes_bound(), plan, run)) return rc;
    uint64_t nonces = 0;  // every nonce is hashed: no early exit
    for (size_t k = 0; k < njobs; k++) {
        const uint64_t n = upper[k] - lower[k] + 1;  // <= GPUHASH_BATCH_MAX_SPAN
        nonces = nonces + n < nonces ? ~0ull : nonces + n;
    }
    call.finish_nonces(nonces);
    for (size_t k = 0; k < njobs; k++) {
        out_totals[k] = res[k].total;
        for (size_t i = 0; i < res[k].held.size(); i++) {
            out_nonces[out_off[k] + i] = res[k].held[i].nonce;
            out_hashes[out_off[k] + i] = res[k].held[i].hash;
        }
    }
    return GPUHASH_OK;
}

int gpuhash_collect_below_batch_ex(gpuhash_ctx* ctx, const uint8_t* msgs, const size_t* msg_off, size_t njobs,
                                   const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                                   uint32_t rchunk, const size_t* out_off, uint64_t* out_nonces,
                                   uint64_t* out_hashes, uint64_t* out_totals) {
    if (!ctx || !msg_off || !lower || !upper || !target || !out_totals) return GPUHASH_EINVAL;
    if (njobs == 0 || njobs > GPUHASH_BATCH_MAX_JOBS) return GPUHASH_EINVAL;
    bool too_long = false;
    for (size_t k = 0; k < njobs; k++) {
        if (msg_off[k + 1] < msg_off[k] || lower[k] > upper[k]) return GPUHASH_EINVAL;
        if (upper[k] - lower[k] >= GPUHASH_BATCH_MAX_SPAN) return GPUHASH_EINVAL;
        if (out_off && (out_off[k + 1] < out_off[k] || out_off[k + 1] - out_off[k] > GPUHASH_COLLECT_MAX))
            return GPUHASH_EINVAL;
        too_long = too_long || msg_off[k + 1] - msg_off[k] > GPUHASH_MAX_MSG;
    }
    if (!msgs && msg_off[njobs] != msg_off[0]) return GPUHASH_EINVAL;
    if (out_off && out_off[njobs] > 0 && (!out_nonces || !out_hashes)) return GPUHASH_EINVAL;
    if (too_long) return GPUHASH_ETOOLONG;
    return guarded([&] {
        return collect_below_batch(ctx, msgs, msg_off, njobs, lower, upper, target, rchunk, out_off, out_nonces,
                                   out_hashes, out_totals);
    });
}

int gpuhash_collect_below_batch(gpuhash_ctx* ctx, const uint8_t* msgs, const size_t* msg_off, size_t njobs,
                                const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                                const size_t* out_off, uint64_t* out_nonces, uint64_t* out_hashes,
                                uint64_t* out_totals) {
    return gpuhash_collect_below_batch_ex(ctx, msgs, msg_off, njobs, lower, upper, target, 0, out_off, out_nonces,
                                          out_hashes, out_totals);
}

int gpuhash_min(gpuhash_ctx* ctx, const uint8_t* msg, size_t msg_len, uint64_t lower,
                uint64_t upper, uint64_t* out_hash, uint64_t* out_nonce) {
    return gpuhash_min_ex(ctx, msg, msg_len, lower, upper, 0, out_hash, out_nonce);
}

int gpuhash_hash_range(gpuhash_ctx* ctx, const uint8_t* msg, size_t msg_len, uint64_t lower,
                       uint64_t count, uint64_t* out) {
    if (!ctx || !out || (msg_len && !msg) || ctx->devs.empty()) return GPUHASH_EINVAL;
    if (count == 0) return GPUHASH_OK;
    if (count > (1ull << 26) || lower + (count - 1) < lower) return GPUHASH_EINVAL;
    if (msg_len > GPUHASH_MAX_MSG) return GPUHASH_ETOOLONG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    Call call(ctx, count);
    if (call.cancelled()) return GPUHASH_ECANCELED;
    DeviceGuard guard;
    HIPCHK(hipSetDevice(ctx->devs[0].ord));
    ScanJob job{kScanDump};
    if (hipMalloc(&job.d_dump, count * sizeof(uint64_t)) != hipSuccess) return GPUHASH_ENOMEM;
    const uint64_t last = lower + (count - 1);
    int rc = guarded([&] { return call.run(msg, msg_len, 0, {SubRange{lower, last, 0}}, job); });
    if (!rc && hipMemcpy(out, job.d_dump, count * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
        rc = GPUHASH_EHIP;
    hipFree(job.d_dump);
    if (!rc) call.finish(lower, last);
    return rc;
}

uint64_t gpuhash_hash_cpu(const uint8_t* msg, size_t msg_len, uint64_t nonce) {
    return hash_host(msg, msg_len, nonce);
}

int gpuhash_last_stats(const gpuhash_ctx* ctx, gpuhash_stats* out) {
    if (!ctx || !out) return GPUHASH_EINVAL;
    std::lock_guard<std::mutex> lock(const_cast<gpuhash_ctx*>(ctx)->mu);
    *out = ctx->last;
    return GPUHASH_OK;
}

int gpuhash_last_launches(const gpuhash_ctx* ctx, gpuhash_launch_record* out, int cap) {
    if (!ctx || cap < 0 || (cap > 0 && !out)) return GPUHASH_EINVAL;
    std::lock_guard<std::mutex> lock(const_cast<gpuhash_ctx*>(ctx)->mu);
    const int n = (int)ctx->recs.size();
    for (int i = 0; i < n && i < cap; i++) out[i] = ctx->recs[(size_t)i];
    return n;
}

int gpuhash_cancel(gpuhash_ctx* ctx) {
    if (!ctx) return GPUHASH_EINVAL;
    ctx->ctl->cancel();  // one lock-free atomic store: async-signal-safe
    return GPUHASH_OK;
}

int gpuhash_resume(gpuhash_ctx* ctx) {
    if (!ctx) return GPUHASH_EINVAL;
    ctx->ctl->resume();
    return GPUHASH_OK;
}

int gpuhash_progress(gpuhash_ctx* ctx, uint64_t* out_done, uint64_t* out_total) {
    if (!ctx || !out_done || !out_total) return GPUHASH_EINVAL;
    ctx->ctl->progress(out_done, out_total);  // no HIP call, no ctx->mu: the call's waiting threads answer
    return GPUHASH_OK;
}

void gpuhash_close(gpuhash_ctx* ctx) {
    if (!ctx) return;
    for (auto& d : ctx->devs) dev_free(d);
    delete ctx;
}

const char* gpuhash_strerror(int rc) {
    switch (rc) {
        case GPUHASH_OK: return "ok";
        case GPUHASH_EINVAL: return "invalid argument (null pointer, lower > upper, or bad device list)";
        case GPUHASH_ENODEV: return "no usable gfx950 (MI355X) device";
        case GPUHASH_EHIP: return "HIP runtime error or kernel launch failure";
        case GPUHASH_ETOOLONG: return "message longer than GPUHASH_MAX_MSG";
        case GPUHASH_ENOMEM: return "out of device or host memory";
        case GPUHASH_ECANCELED: return "search cancelled (gpuhash_cancel; gpuhash_resume clears it)";
        default: return "unknown gpuhash error";
    }
}

#ifndef GPUHASH_BUILD_ID
#define GPUHASH_BUILD_ID "unknown"
#endif

const char* gpuhash_version(void) {
#ifdef GPUHASH_TIE_TEST_BITS
    return "gpuhash 0.9 gfx950 build=" GPUHASH_BUILD_ID " TIE-TEST (truncated keys; test build only)";
#else
    return "gpuhash 0.9 gfx950 build=" GPUHASH_BUILD_ID;
#endif
}

}  // extern "C"
