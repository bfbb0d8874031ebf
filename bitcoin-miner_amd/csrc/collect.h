// collect.h -- the order-independent part of gpuhash_collect_below: from per-sub-range
// (count, unordered hit list) results to an exact total and the exact lowest `cap` hits.
//
// Shared by the host library (gpuhash.cpp, where a sub-range runs on a device) and the CPU
// replay (hostcheck.cpp, where it runs in plain C++ with a seeded append order); plain C++,
// no HIP.
//
// What one run of a sub-range gives (the scan kernel's MODE 3, scan_kernel.h): `count`, the
// exact number of qualifying nonces in it, whatever the list holds; and, when a list of B
// entries was asked for, the hits that found room in it, in the order the waves appended them.
// If count <= B the list is ALL the sub-range's hits, so sorting it by nonce gives them in
// ascending order.  If count > B the list is merely some B of them and is discarded (a run
// need not even return it).
//
// The collector walks the search's slices ascending and, within a slice, its shards
// ascending (a slice's shards are one batch: the host runs them concurrently, one per
// context entry).  Sub-ranges are disjoint and ascending, so:
//   total  adds every ORIGINAL sub-range's count once.  Counts of re-runs are never added:
//          they recount nonces already counted.
//   list   while fewer than cap hits are held, a sub-range with count <= B appends its
//          sorted hits (up to cap).  One that overflowed B is split in halves and each half
//          is re-run with a list, lower half first, recursively.  A single nonce holds at
//          most one hit and B >= 1, so the splitting ends.  Every hit appended is lower
//          than every hit of any later sub-range, and no hit of an earlier one was left out
//          while room remained: the held hits are always the lowest ones, ascending.
//          Once cap hits are held, every later sub-range runs without a list (capacity 0)
//          and only adds its count; it is never re-run.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <vector>

namespace gpuhash {

// One hit; the layout of the device list's entries (kernels.h, Cand).
struct Hit {
    uint64_t hash, nonce;
};

// One sub-range of a batch: an inclusive nonce range and the shard (context entry) it runs on.
struct SubRange {
    uint64_t lo, hi;
    int shard;
};

// What a run of one sub-range reports.
struct SubResult {
    uint64_t count = 0;
    std::vector<Hit> hits;  // all `count` hits when a list was asked for and count <= B;
                            // ignored otherwise
};

// run(batch, want_list, results) -> 0 or an error code, which ends the collection: runs every
// sub-range of `batch` (concurrently where it can) and fills results[i] for batch[i].
// split(lo, hi, batch): the non-empty shards of the slice [lo, hi], ascending.
template <class Run, class Split>
class Collector {
public:
    Collector(uint64_t buffer_entries, size_t cap, Run run, Split split)
        : B_(std::max<uint64_t>(buffer_entries, 1)), cap_(cap), run_(run), split_(split) {}

    uint64_t total = 0;     // saturates at 2^64-1
    std::vector<Hit> held;  // the lowest min(cap, total) hits, ascending by nonce

    // Collects over the inclusive [lower, upper] in slices of `slice` nonces.
    int collect(uint64_t lower, uint64_t upper, uint64_t slice) {
        std::vector<SubRange> batch;
        std::vector<SubResult> res;
        for (uint64_t lo = lower;;) {
            const uint64_t hi = upper - lo < slice ? upper : lo + (slice - 1);
            batch.clear();
            split_(lo, hi, batch);
            const bool want_list = held.size() < cap_;
            res.assign(batch.size(), SubResult{});
            if (int rc = run_(batch, want_list, res)) return rc;
            for (size_t i = 0; i < batch.size(); i++) {
                total = res[i].count > ~0ull - total ? ~0ull : total + res[i].count;
                if (held.size() < cap_)
                    if (int rc = take(batch[i], res[i])) return rc;
            }
            if (hi == upper) return 0;
            lo = hi + 1;
        }
    }

private:
    // Appends the lowest hits of `sub` while room remains.  `r` is a run of `sub` WITH a list.
    int take(const SubRange& sub, SubResult& r) {
        if (r.count <= B_) {
            std::sort(r.hits.begin(), r.hits.end(), [](const Hit& a, const Hit& b) { return a.nonce < b.nonce; });
            const size_t n = std::min(r.hits.size(), cap_ - held.size());
            held.insert(held.end(), r.hits.begin(), r.hits.begin() + (std::ptrdiff_t)n);
            return 0;
        }
        // overflowed: count > B >= 1 hits, so sub.lo < sub.hi and both halves are non-empty
        const uint64_t mid = sub.lo + (sub.hi - sub.lo) / 2;
        const SubRange halves[2] = {{sub.lo, mid, sub.shard}, {mid + 1, sub.hi, sub.shard}};
        for (const SubRange& h : halves) {
            if (held.size() >= cap_) break;
            std::vector<SubRange> one{h};
            std::vector<SubResult> res(1);
            if (int rc = run_(one, true, res)) return rc;
            if (int rc = take(h, res[0])) return rc;
        }
        return 0;
    }

    const uint64_t B_;
    const size_t cap_;
    Run run_;
    Split split_;
};

// ---- gpuhash_collect_below_batch: from one run of a batch to every job's exact answer ----
//
// What one run of n jobs gives (the scan kernel's MODE 6, scan_kernel.h): counts[k], job k's
// exact hit counter, whatever the list holds; and the first min(appended, B) entries of the ONE
// list the listing jobs share, each {hash, nonce, job}, in the order the waves appended them.
// A job that does not list (cap_k == 0) appends nothing.  For a job that lists, every hit was
// counted once and either stored once or not at all (its slot lay past the list's end), so with
// listed_k the number of entries tagged k:
//   total_k  is counts[k], always.  A re-run's count is never added: it recounts the same nonces.
//   list     listed_k == counts[k]: the list holds ALL of job k's hits; sorted by nonce, the
//            first cap_k are the lowest ones.  Otherwise the list filled up before job k was
//            complete, and what it holds of job k is merely some of its hits: they are dropped
//            and rerun(k, cap_k, out) runs job k alone, through the Collector above, which leaves
//            in out its own total and the lowest min(cap_k, total) hits.  That total must equal
//            counts[k] (both are exact counts of one range): anything else is `corrupt_rc`.
// Jobs are independent, so the order of the re-runs does not matter; they run after the batch.
struct JobHits {
    uint64_t total = 0;
    std::vector<Hit> held;  // the lowest min(cap, total) hits, ascending by nonce
};

// out[0..n): the jobs' answers.  *reruns, if given, counts the jobs that were re-run.
// rerun(k, cap, JobHits&) -> 0 or an error code, which ends the fold.
template <class Entry, class Rerun>
int fold_collect_batch(size_t n, const uint64_t* counts, const Entry* list, size_t nlist, const size_t* caps,
                       int corrupt_rc, Rerun&& rerun, JobHits* out, uint64_t* reruns = nullptr) {
    std::vector<size_t> at(n + 1, 0);  // entries tagged k: sorted[at[k] .. at[k + 1])
    for (size_t i = 0; i < nlist; i++) {
        if (list[i].job >= n) return corrupt_rc;
        at[(size_t)list[i].job + 1]++;
    }
    for (size_t k = 0; k < n; k++) at[k + 1] += at[k];
    std::vector<Hit> sorted(nlist);
    {
        std::vector<size_t> next(at.begin(), at.end() - 1);
        for (size_t i = 0; i < nlist; i++) sorted[next[list[i].job]++] = Hit{list[i].hash, list[i].nonce};
    }
    for (size_t k = 0; k < n; k++) {
        out[k].total = counts[k];
        out[k].held.clear();
        if (!caps[k]) continue;
        const size_t listed = at[k + 1] - at[k];
        if (listed == counts[k]) {
            const auto b = sorted.begin() + (std::ptrdiff_t)at[k], e = sorted.begin() + (std::ptrdiff_t)at[k + 1];
            std::sort(b, e, [](const Hit& x, const Hit& y) { return x.nonce < y.nonce; });
            out[k].held.assign(b, b + (std::ptrdiff_t)std::min(listed, caps[k]));
            continue;
        }
        if (listed > counts[k]) return corrupt_rc;  // more stored than counted
        JobHits again;
        if (reruns) ++*reruns;
        if (int rc = rerun(k, caps[k], again)) return rc;
        if (again.total != counts[k]) return corrupt_rc;
        out[k].held = std::move(again.held);
    }
    return 0;
}

}  // namespace gpuhash
