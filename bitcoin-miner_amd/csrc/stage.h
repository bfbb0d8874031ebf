// stage.h -- everything a device run decides before it touches the device: the plan, its
// kernel-variant groups, the launch metadata buffer and its bytes, the K+W tables, the piece
// rule and the slice width.  Shared by the host library (gpuhash.cpp, dev_run) and the CPU
// replay (hostcheck.cpp), which cuts its pieces from the buffer that fill() wrote, as the
// kernels do from its device copy; plain C++, no HIP.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "collect.h"
#include "pack.h"
#include "plan.h"

namespace gpuhash {

// Per group at the head of the metadata buffer: the work counter, then the 4 clock words the
// scan kernel writes (start/end s_memtime and s_memrealtime of workgroup 0).
constexpr size_t kCounterBytes = 40;

// The piece rule.  A group's work is its launches' rows x loop values ("row-iterations"),
// which the workgroups grab in pieces of clamp(remaining / (2 * grid), min, max)
// (scan_kernel.h); there are no more workgroups than minimum-size pieces.
constexpr uint32_t kMinPiece = 10;
constexpr uint32_t kDefaultMaxPiece = 400;  // unless the call's rchunk says otherwise

// The value of a numeric environment override, 0 when unset.
inline uint64_t env_u64(const char* name) {
    const char* e = std::getenv(name);
    return e ? std::strtoull(e, nullptr, 10) : 0;
}

// Nonces in one slice of a search over `entries` context entries, saturating.  Per device
// 2^38, ~8 s of work on one MI355X at config-2 rates: every launch descriptor covers <=
// 10^10-10^12 nonces (plan.h), so a slice's plan stays a few hundred descriptors whatever the
// span (a 2^64 range would otherwise plan ~10^9), and the per-slice sync and merge cost nothing
// measurable.  GPUHASH_SLICE_NONCES overrides it (tests use it to exercise the slice loop,
// including its end at 2^64-1, on oracle-sized ranges), and a caller's per_device both.
inline uint64_t slice_width(uint64_t entries, uint64_t per_device = 0) {
    if (!per_device) per_device = env_u64("GPUHASH_SLICE_NONCES");
    if (!per_device) per_device = 1ull << 38;
    return per_device > ~0ull / entries ? ~0ull : per_device * entries;
}

// The non-empty shards of the slice [lo, hi] over n context entries, ascending (the
// collector's `split`, collect.h).
inline void split_slice(uint64_t msg_len, uint64_t lo, uint64_t hi, int n, int policy, std::vector<SubRange>& batch) {
    if (n == 1) return batch.push_back(SubRange{lo, hi, 0});
    const std::vector<Shard> sh = shard_range(msg_len, lo, hi, n, policy);
    for (int i = 0; i < n; i++)
        if (!sh[(size_t)i].empty) batch.push_back(SubRange{sh[(size_t)i].lo, sh[(size_t)i].hi, i});
}

// Rows (256 consecutive lane values each) x loop values of one descriptor.
inline uint64_t row_iterations(const LaunchDesc& D) {
    return (uint64_t)((D.p_last - D.p_first) / (uint32_t)kBlock + 1u) * D.R;
}

// The launches of one kernel variant: ONE persistent launch over all their descriptors.
struct StageGroup {
    int J, C2, EX;
    std::vector<size_t> idx;  // its launches in Stage::plan, in plan order
    uint64_t total = 0;       // row-iterations (offs[n])
    uint64_t nonces = 0;      // of all its launches
    int d = 0, c = 0;         // digits and digit blocks of its largest launch (the first such);
                              // a first-hit batch stage: the digit count of all of them
    // byte positions in the metadata buffer, each 16-byte aligned: the counter block, the
    // n + 1 prefix offsets (8 B each), the n descriptors, and for C2 = 3 the launches' p-tables
    size_t work_at = 0, offs_at = 0, desc_at = 0, ptab_at = 0, ptab_bytes = 0;
};

// A uniform K+W table of C2 = 1 / J = 0 descriptors: block B's words depend only on the digit
// count d, so one table of 64 x R words per d serves all of them; k_ktab builds it from the
// device copy of the first such descriptor, at desc_byte.  (A batch stage has many messages:
// there a table serves the descriptors whose block B words U and R equal that descriptor's.)
struct StageTab {
    int d;
    uint32_t off, R;  // words
    size_t desc_byte;
    size_t launch = 0;  // that descriptor's launch in Stage::plan
};

// One search of a batch (gpuhash_min_batch, gpuhash_first_below_batch).
struct BatchJob {
    const uint8_t* msg;
    uint64_t len, lo, hi;
    const PackJob* rec = nullptr;  // a packed job's record where the caller built it before (pack.h)
};

// the list's head: its append counter and its capacity in entries (a uint32 each), padding
constexpr size_t kBatchListHead = 16;

// A batch launch never has more workgroups than this, whatever the device holds resident
// (an MI355X holds 2048 of the plain kernels'), so the list bound below needs no device.
constexpr uint32_t kBatchMaxGrid = 4096;

// The most entries the workgroups of a launch of <= grid workgroups can append for a job whose
// descriptors cover `span` consecutive row-iterations.  A workgroup's grabs return ascending
// positions (the work counter only rises) and a group's jobs lie in ascending order of
// position, so a workgroup meets each job in one unbroken run of its parts and leaves it once:
// at most one entry per workgroup that took a piece overlapping the job.  Pieces are disjoint
// and consecutive, each at least gmin long except the last of the group, so at most
// ceil(span / gmin) + 1 of them overlap `span` positions.
inline uint64_t batch_job_entries(uint64_t span, uint32_t gmin, uint64_t grid) {
    return std::min<uint64_t>(grid, (span + gmin - 1) / gmin + 1);
}

// A PACKED job's entries are bounded per segment instead, with no grid or piece in the argument:
// one entry at most per 64-item wave window of its class's space that the segment meets,
// floor((c + 62) / 64) + 1 for c items (pack.h, pack_seg_entries, where the argument is stated);
// Stage adds their sum, PackTables::entries, to list_cap.

// The metadata bytes a job adds to a batch stage, at most (every alignment gap at its widest):
// what the sub-batch cut (gpuhash.h) sums, with the K+W tables the job adds (BatchTables).
// A first-hit batch (pair) has two words per job, and may put every launch in a group of its own:
// the group's second prefix offset then takes 8 of the 64 bytes priced for the gaps, which are
// at most 15 wide there (the offsets and the descriptors end 16-byte aligned).
// A collect batch (collects) has three words per job and no list in the buffer: its list is the
// entry's fixed device buffer (Stage::collects), which the bound does not count.
inline uint64_t batch_job_bytes(const std::vector<Launch>& plan, uint32_t gmin, bool pair = false,
                                bool collects = false) {
    // its pruning word (pair: bound and target; collects: counter, target, list flag); its share of the list head
    uint64_t b = (collects ? 24 : pair ? 16 : 8) + 16;
    for (const Launch& l : plan) {
        b += sizeof(LaunchDesc) + 8 + kCounterBytes + 4 * 16;
        b += sizeof(uint32_t) * l.nptab;
        if (!collects) b += sizeof(BatchEntry) * batch_job_entries(row_iterations(l.desc), gmin, kBatchMaxGrid);
    }
    return b;
}

// The K+W tables of the jobs taken into a sub-batch so far, by what a table is computed from
// (block B's uniform words and R, as Stage shares them).
struct BatchTables {
    std::vector<const LaunchDesc*> keys;

    static bool same(const LaunchDesc& a, const LaunchDesc& b) {
        return a.R == b.R && !std::memcmp(a.U, b.U, sizeof a.U);
    }
    // Bytes of the tables `plan` needs that are not held yet; take = true holds them.  The
    // descriptors must stay where they are while the sub-batch is being cut.
    uint64_t add(const std::vector<Launch>& plan, bool take) {
        uint64_t bytes = 0;
        const size_t held = keys.size();
        for (const Launch& l : plan) {
            if (l.C2 != 1 || l.J != 0) continue;
            if (std::any_of(keys.begin(), keys.end(), [&](const LaunchDesc* k) { return same(*k, l.desc); })) continue;
            keys.push_back(&l.desc);
            bytes += 4 * 64ull * l.desc.R;
        }
        if (!take) keys.resize(held);
        return bytes;
    }
};

// A job of a batch, planned: its launches, batch_job_bytes of them and their plan_cost.  A packed
// job (pack.h) has no launches: `src` is the job itself, for the stage's packed tables, `bytes` its
// pack_job_bytes and `cost` its nonces at kPackCost.
struct PlannedJob {
    std::vector<Launch> plan;
    uint64_t bytes;
    double cost;
    bool packed = false;
    BatchJob src{};
};

// Whether a job of gpuhash_min_batch or gpuhash_collect_below_batch runs packed under `policy`
// (include/gpuhash.h, GPUHASH_LAYOUT_PACKED_ALWAYS).
inline bool packs(int policy, uint64_t lo, uint64_t hi) {
    return (policy & GPUHASH_LAYOUT_PACKED_ALWAYS) && hi - lo < kPackMaxSpan;
}

// gpuhash_first_below_batch_early (include/gpuhash.h, where the rule is stated): how many leading
// nonces of the job [lo, hi] with `target` run in packed rounds.  prefix != 0 forces min(span,
// prefix); else 4 * E, E = ceil(2^64 / (target + 1)) = floor((2^64 - 1) / (target + 1)) + 1, while
// that is at most GPUHASH_EARLY_MAX_PREFIX, and 0 beyond it.
inline uint64_t early_limit(uint64_t lo, uint64_t hi, uint64_t target, uint64_t prefix) {
    const uint64_t span = hi - lo + 1;  // <= GPUHASH_BATCH_MAX_SPAN
    if (prefix) return std::min(span, prefix);
    if (target == ~0ull) return std::min<uint64_t>(span, 4);
    const uint64_t q = ~0ull / (target + 1);  // E - 1
    if (q >= GPUHASH_EARLY_MAX_PREFIX / 4) return 0;
    return std::min(span, 4 * (q + 1));
}

// The items a round of it gives every job at most: the first round's, for `fronts` jobs with a
// packed front, and the next round's after one of c.
constexpr uint64_t kEarlyRoundItems = 1ull << 20;  // <= kPackMaxSpan: a piece is one packed job
inline uint64_t early_first_chunk(uint64_t fronts) {
    uint64_t c = 64;
    while (c < kEarlyRoundItems && c * fronts < kEarlyRoundItems) c *= 2;
    return c;
}
inline uint64_t early_next_chunk(uint64_t c) { return std::min(2 * c, kEarlyRoundItems); }

// A packed nonce against a nonce of a full row of the plain layouts (plan_cost's unit): it builds
// its whole block and schedule itself.  Only the balance of a batch's runs over entries reads it.
constexpr double kPackCost = 2.0;

inline PlannedJob plan_packed_job(const BatchJob& j, bool collects = false) {
    PlannedJob p;
    p.bytes = pack_job_bytes(j.lo, j.hi, collects);
    p.cost = kPackCost * (double)(j.hi - j.lo + 1);
    p.packed = true;
    p.src = j;
    return p;
}

// The jobs [first, end) of a sub-batch as a batch stage takes them: their plans, moved from, and
// which of them are packed (null when none is).
struct StageJobs {
    std::vector<std::vector<Launch>> plans;
    std::vector<const BatchJob*> packed;
    bool any = false;

    StageJobs(std::vector<PlannedJob>& jobs, size_t first, size_t end) : plans(end - first), packed(end - first) {
        for (size_t k = first; k < end; k++) {
            plans[k - first] = std::move(jobs[k].plan);
            packed[k - first] = jobs[k].packed ? &jobs[k].src : nullptr;
            any = any || jobs[k].packed;
        }
    }
    const std::vector<const BatchJob*>* which() const { return any ? &packed : nullptr; }
};

inline PlannedJob plan_job(const BatchJob& j, uint32_t rchunk, int policy, bool host_ptab = false,
                           bool pair = false, bool collects = false) {
    PlannedJob p;
    plan_range(j.msg, j.len, j.lo, j.hi, p.plan, rchunk, policy, host_ptab);
    const uint32_t gmax = rchunk ? rchunk : kDefaultMaxPiece;
    p.bytes = batch_job_bytes(p.plan, std::min(kMinPiece, gmax), pair, collects);
    p.cost = plan_cost(p.plan);
    return p;
}

// The bound on a sub-batch's metadata and table bytes (include/gpuhash.h, gpuhash_min_batch):
// GPUHASH_BATCH_BYTES, or `bytes`, overrides the default; at most 1 GiB, so that a list's
// entry count fits its 32-bit head.
inline uint64_t batch_bytes_bound(uint64_t bytes = 0) {
    if (!bytes) bytes = env_u64("GPUHASH_BATCH_BYTES");
    if (!bytes) bytes = GPUHASH_BATCH_BYTES_DEFAULT;
    return std::min<uint64_t>(bytes, 1ull << 30);
}

// Walks a batch of njobs jobs as consecutive sub-batches of whole jobs: jobs are planned one
// by one (plan(k) -> PlannedJob) and a sub-batch ends before the job that would take the sum
// of its jobs' batch_job_bytes and of their K+W tables, shared ones counted once, past `bound`; a sub-batch always holds at least one job.
// run(first, jobs) runs the sub-batch whose first job is `first`; a non-zero return ends the walk.
template <class Plan, class Run>
int for_each_sub_batch(size_t njobs, uint64_t bound, Plan&& plan, Run&& run) {
    std::vector<PlannedJob> jobs;
    PlannedJob held;
    bool holding = false;
    for (size_t first = 0, k = 0; first < njobs; first = k) {
        jobs.clear();
        jobs.reserve(njobs - first);  // the table keys point into the jobs' plans: no moves
        BatchTables tabs;
        uint64_t sum = 0;
        for (; k < njobs; k++) {
            PlannedJob p = holding ? std::move(held) : plan(k);
            holding = false;
            if (!jobs.empty() && sum + p.bytes + tabs.add(p.plan, false) > bound) {
                held = std::move(p);
                holding = true;
                break;
            }
            jobs.push_back(std::move(p));
            sum += jobs.back().bytes + tabs.add(jobs.back().plan, true);
        }
        if (int rc = run(first, jobs)) return rc;
    }
    return 0;
}

// A sub-batch's jobs as at most n contiguous runs of about equal plan_cost, one per context
// entry, [first, end) each; a job is never split.
inline std::vector<std::pair<size_t, size_t>> batch_runs(const std::vector<PlannedJob>& jobs, size_t n) {
    std::vector<std::pair<size_t, size_t>> runs;
    double total = 0, acc = 0;
    for (const PlannedJob& j : jobs) total += j.cost;
    size_t start = 0, r = 0;
    for (size_t k = 0; k < jobs.size(); k++) {
        acc += jobs[k].cost;
        const bool last = k + 1 == jobs.size();
        if (last || (runs.size() + 1 < n && acc >= total * (double)(r + 1) / (double)n)) {
            runs.push_back({start, k + 1});
            start = k + 1;
            r = std::max(r + 1, total > 0 ? (size_t)(acc * (double)n / total) : r + 1);
        }
    }
    return runs;
}

struct Stage {
    std::vector<Launch> plan;  // desc.tab_off set as the kernels read it
    std::vector<StageGroup> groups;  // in first-appearance order of (J, C2, EX)
    std::vector<StageTab> tabs;
    size_t tab_words = 0, bytes = 0;  // of all K+W tables; of the metadata buffer
    uint32_t gmax, gmin;              // piece size bounds
    // A batch stage (njobs > 0): desc.job of every launch is its job's index, a group's
    // launches are in ascending job order, and after the groups' regions the buffer holds
    // njobs pruning words (8 B each, armed to all ones) at thresh_at and the result list at
    // list_at: kBatchListHead bytes of append counter, then room for list_cap BatchEntry.
    // Only the first upload_bytes bytes are host-built (a single stage: all of them).
    size_t njobs = 0, thresh_at = 0, list_at = 0, list_cap = 0, upload_bytes = 0;
    // A first-hit batch stage (gpuhash_first_below_batch; by_digits): a batch stage whose groups
    // are keyed (d, J, C2, EX), d the launches' digit count, and ordered by d ascending, then by
    // first appearance.  The groups run back to back on one stream, so every nonce of up to d
    // digits of every job has been hashed, and its hit published in the job's bound word, before
    // any launch of more than d digits starts: A JOB WHOSE ANSWER HAS d DIGITS NEVER HASHES A
    // NONCE OF MORE THAN d DIGITS.  That is a property of this order alone, whatever the
    // workgroups' timing (the kernel's MODE 5 reads the bound at a job change and skips every part
    // whose nonces all lie above it).  The per-job region at thresh_at holds TWO 64-bit words per
    // job: the bound, the lowest qualifying nonce found so far (armed to all ones), then the job's
    // target.  The result list is a batch stage's.
    bool by_digits = false;
    std::vector<uint64_t> targets;  // by_digits, collects: one per job
    // A collect batch stage (gpuhash_collect_below_batch; collects): a batch stage in the job-major
    // order of the min_batch constructor (there is no early exit for an order to protect).  The
    // per-job region at thresh_at holds THREE 64-bit words per job: the job's exact hit counter
    // (armed to 0), its target, and whether the job lists at all (cap_k > 0).  The buffer ends with
    // the list's head at list_at: a 64-bit append counter (armed to 0), the capacity list_cap as a
    // uint32, padding.  The list itself is NOT in the buffer: it is the entry's own device array of
    // list_cap = buffer_entries BatchEntry, shared by all listing jobs.  That capacity is not a
    // proved bound (it depends on the hits): the host finds the jobs it cut short by their
    // counters and re-runs them (collect.h, fold_collect_batch).
    bool collects = false;
    std::vector<uint8_t> lists;  // collects: one per job, cap_k > 0
    // The packed jobs of a min or collect batch stage (pack.h; none unless the policy carries
    // GPUHASH_LAYOUT_PACKED_ALWAYS): ONE more group, the last, {J = -1, C2 = 4, EX = 0}, without
    // descriptors: its total is the tile count, its nonces the packed nonces, c the most tail
    // blocks of any segment.  Its counter block sits with the other groups', and its tables --
    // records, segments, tiles -- after the groups' regions and before the per-job region, inside
    // the upload.  The per-job region and the list are shared by packed and unpacked jobs; the
    // packed jobs add PackTables::entries to list_cap (pack.h, pack_seg_entries).
    PackTables pack;
    size_t pack_recs_at = 0, pack_segs_at = 0, pack_tiles_at = 0;

    Stage(const uint8_t* msg, uint64_t len, uint64_t lo, uint64_t hi, uint32_t rchunk, int policy,
          bool host_ptab = false) : gmax(rchunk ? rchunk : kDefaultMaxPiece), gmin(std::min(kMinPiece, gmax)) {
        plan_range(msg, len, lo, hi, plan, rchunk, policy, host_ptab);
        lay_out();
    }

    // The stage of a batch: plans[k] is job k's plan_range under the context's policy (moved
    // from).  All launches of all jobs are grouped by (J, C2, EX) in first-appearance order;
    // within a group each job's descriptors are contiguous, jobs ascending.
    // packed: null, or per job the job itself where it runs packed (its plan is then empty).
    Stage(std::vector<std::vector<Launch>>& plans, uint32_t rchunk,
          const std::vector<const BatchJob*>* packed = nullptr)
        : gmax(rchunk ? rchunk : kDefaultMaxPiece), gmin(std::min(kMinPiece, gmax)), njobs(plans.size()) {
        for (size_t k = 0; k < plans.size(); k++)
            for (Launch& l : plans[k]) {
                l.desc.job = (uint32_t)k;
                plan.push_back(std::move(l));
            }
        if (packed) take_packed(*packed);
        lay_out();
    }

    // The stage of a first-hit batch: plans[k] as above, target[k] job k's target.  See by_digits.
    // packed: null, or per job the job itself where it runs packed: a round of
    // gpuhash_first_below_batch_early, whose stage holds the packed group and nothing else.
    Stage(std::vector<std::vector<Launch>>& plans, const uint64_t* target, uint32_t rchunk,
          const std::vector<const BatchJob*>* packed = nullptr)
        : gmax(rchunk ? rchunk : kDefaultMaxPiece), gmin(std::min(kMinPiece, gmax)), njobs(plans.size()),
          by_digits(true), targets(target, target + plans.size()) {
        for (size_t k = 0; k < plans.size(); k++)
            for (Launch& l : plans[k]) {
                l.desc.job = (uint32_t)k;
                plan.push_back(std::move(l));
            }
        if (packed) take_packed(*packed);
        lay_out();
    }

    // The stage of a collect batch: plans[k] as above, target[k] job k's target, lists[k] whether
    // it lists, buffer_entries the capacity of the entry's list.  See collects.
    Stage(std::vector<std::vector<Launch>>& plans, const uint64_t* target, const uint8_t* lists_,
          uint64_t buffer_entries, uint32_t rchunk, const std::vector<const BatchJob*>* packed = nullptr)
        : gmax(rchunk ? rchunk : kDefaultMaxPiece), gmin(std::min(kMinPiece, gmax)), njobs(plans.size()),
          list_cap((size_t)std::min<uint64_t>(buffer_entries, 0xFFFFFFFFull)),
          targets(target, target + plans.size()), collects(true), lists(lists_, lists_ + plans.size()) {
        for (size_t k = 0; k < plans.size(); k++)
            for (Launch& l : plans[k]) {
                l.desc.job = (uint32_t)k;
                plan.push_back(std::move(l));
            }
        if (packed) take_packed(*packed);
        lay_out();
    }

    static size_t aligned(size_t b) { return (b + 15) & ~(size_t)15; }

    // Bytes of a job's words in the per-job region.
    size_t job_words_bytes() const { return collects ? 24 : by_digits ? 16 : 8; }

   private:
    void take_packed(const std::vector<const BatchJob*>& packed) {
        for (size_t k = 0; k < packed.size(); k++)
            if (const BatchJob* j = packed[k]) {
                if (j->rec) pack.add_job((uint32_t)k, *j->rec, j->lo, j->hi);
                else pack.add_job((uint32_t)k, j->msg, j->len, j->lo, j->hi);
            }
        pack.finish();
    }

    void lay_out() {
        for (size_t i = 0; i < plan.size(); i++) {
            const Launch& l = plan[i];
            auto it = std::find_if(groups.begin(), groups.end(), [&](const StageGroup& g) {
                return g.J == l.J && g.C2 == l.C2 && g.EX == l.EX && (!by_digits || g.d == l.d);
            });
            if (it == groups.end()) {
                it = groups.insert(it, StageGroup{l.J, l.C2, l.EX});
                it->d = l.d;
            }
            it->idx.push_back(i);
        }
        if (!pack.empty()) {
            groups.push_back(StageGroup{-1, 4, 0});
            groups.back().total = pack.tiles.size();
            groups.back().nonces = pack.nonces;
            groups.back().c = pack.blocks;
        }
        if (by_digits)
            std::stable_sort(groups.begin(), groups.end(),
                             [](const StageGroup& a, const StageGroup& b) { return a.d < b.d; });
        auto align = [&] { bytes = aligned(bytes); };
        bytes = kCounterBytes * groups.size();
        align();
        for (size_t gi = 0; gi < groups.size(); gi++) {
            StageGroup& g = groups[gi];
            g.work_at = kCounterBytes * gi;
            g.offs_at = bytes;
            bytes += 8 * (g.idx.size() + 1);
            align();
            g.desc_at = bytes;
            bytes += sizeof(LaunchDesc) * g.idx.size();
            align();
            g.ptab_at = bytes;
            uint64_t biggest = 0;
            for (size_t k = 0; k < g.idx.size(); k++) {
                Launch& l = plan[g.idx[k]];
                LaunchDesc& D = l.desc;
                g.total += row_iterations(D);
                const uint64_t n = (l.hi - l.lo) / l.stride + 1;
                g.nonces += n;
                if (!k || n > biggest) { biggest = n; g.d = l.d; g.c = l.c; }
                if (l.C2 == 3) {  // lane table: room for this launch's p-table (k_ptab fills it)
                    D.tab_off = (uint32_t)(g.ptab_bytes / sizeof(uint32_t));
                    g.ptab_bytes += sizeof(uint32_t) * l.nptab;
                }
                if (l.C2 == 1 && l.J == 0) {
                    // one message: block B's words follow from d.  A batch: the table is keyed
                    // by what it is computed from, block B's uniform words and R, so jobs that
                    // agree on those share it
                    auto it = std::find_if(tabs.begin(), tabs.end(), [&](const StageTab& t) {
                        if (!njobs) return t.d == l.d;
                        const LaunchDesc& T = plan[t.launch].desc;
                        return t.R == D.R && !std::memcmp(T.U, D.U, sizeof D.U);
                    });
                    if (it == tabs.end()) {
                        const size_t at = g.desc_at + k * sizeof(LaunchDesc);
                        it = tabs.insert(it, StageTab{l.d, (uint32_t)tab_words, D.R, at, g.idx[k]});
                        tab_words += 64ull * D.R;
                    }
                    D.tab_off = it->off;
                }
            }
            bytes += g.ptab_bytes;
            align();
        }
        if (!pack.empty()) {
            pack_recs_at = bytes;
            bytes += sizeof(PackJob) * pack.recs.size();
            align();
            pack_segs_at = bytes;
            bytes += sizeof(PackSeg) * pack.segs.size();
            align();
            pack_tiles_at = bytes;
            bytes += sizeof(PackTile) * pack.tiles.size();
            align();
        }
        upload_bytes = bytes;
        if (!njobs) return;
        thresh_at = bytes;
        bytes += job_words_bytes() * njobs;
        align();
        list_at = bytes;
        upload_bytes = list_at + kBatchListHead;
        if (collects) {  // the list is the entry's own array: the buffer ends with its head
            bytes = upload_bytes;
            align();
            return;
        }
        for (const StageGroup& g : groups) {
            const uint64_t grid = Stage::grid(g, kBatchMaxGrid);
            uint64_t span = 0;
            for (size_t k = 0; k < g.idx.size(); k++) {
                span += row_iterations(plan[g.idx[k]].desc);
                if (k + 1 == g.idx.size() || plan[g.idx[k + 1]].desc.job != plan[g.idx[k]].desc.job) {
                    list_cap += batch_job_entries(span, gmin, grid);
                    span = 0;
                }
            }
        }
        list_cap += pack.entries;  // none without packed jobs
        bytes = list_at + kBatchListHead + sizeof(BatchEntry) * list_cap;
        align();
    }

   public:
    // Writes the buffer's host-built bytes: zeroed counter blocks, and per group its prefix
    // offsets and descriptors.  The p-table room is the device's to fill.
    void fill(uint8_t* meta) const {
        std::memset(meta, 0, kCounterBytes * groups.size());
        for (const StageGroup& g : groups) {
            auto* offs = reinterpret_cast<unsigned long long*>(meta + g.offs_at);
            auto* descs = reinterpret_cast<LaunchDesc*>(meta + g.desc_at);
            unsigned long long acc = 0;  // meta may be pinned memory: written, never read back
            for (size_t k = 0; k < g.idx.size(); k++) {
                offs[k] = acc;
                descs[k] = plan[g.idx[k]].desc;
                acc += row_iterations(plan[g.idx[k]].desc);
            }
            offs[g.idx.size()] = acc;
        }
        if (!pack.empty()) {
            std::memcpy(meta + pack_recs_at, pack.recs.data(), sizeof(PackJob) * pack.recs.size());
            std::memcpy(meta + pack_segs_at, pack.segs.data(), sizeof(PackSeg) * pack.segs.size());
            std::memcpy(meta + pack_tiles_at, pack.tiles.data(), sizeof(PackTile) * pack.tiles.size());
        }
        if (collects) {
            for (size_t k = 0; k < njobs; k++) {  // {hit counter: 0, target, lists}
                const uint64_t words[3] = {0ull, targets[k], lists[k] ? 1ull : 0ull};
                std::memcpy(meta + thresh_at + sizeof words * k, words, sizeof words);
            }
            const uint32_t head[4] = {0u, 0u, (uint32_t)list_cap, 0u};  // appended (64 bits), capacity
            std::memcpy(meta + list_at, head, kBatchListHead);
        } else if (njobs) {
            std::memset(meta + thresh_at, 0xFF, job_words_bytes() * njobs);
            for (size_t k = 0; by_digits && k < njobs; k++)  // {bound: all ones, target}
                std::memcpy(meta + thresh_at + 16 * k + 8, &targets[k], 8);
            const uint32_t head[4] = {0u, (uint32_t)list_cap, 0u, 0u};  // appended, capacity
            std::memcpy(meta + list_at, head, kBatchListHead);
        }
    }

    // Workgroups of a group's launch, given the kernel's resident capacity on the device.
    static unsigned int grid(const StageGroup& g, unsigned int resident) {
        // the packed group (C2 = 4) hands out tiles, down to one per grab (pack.h)
        const uint64_t pieces = g.C2 == 4 ? g.total : (g.total + kMinPiece - 1) / kMinPiece;
        return (unsigned int)std::min<uint64_t>(resident, std::max<uint64_t>(pieces, 1));
    }
};

}  // namespace gpuhash
