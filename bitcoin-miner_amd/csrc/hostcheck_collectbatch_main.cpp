// hostcheck_collectbatch_main.cpp -- TEST-ONLY stand-alone program over hostcheck_collect_below_batch,
// for a sanitizer build (lib/hostcheck_collectbatch_asan: plan.cpp + hostcheck.cpp + this file under
// -fsanitize=address,undefined; tests/test_collect_below_batch_cpu.py runs it).  It stages and
// replays collect batches on the CPU -- a few hundred jobs with every kind of target and room,
// lists of 1 to 2^20 entries, sub-batches, several context entries, the top of uint64 -- and
// checks every job against a plain ascending scan with hash_host.  Exit status 0 and "ok" when all
// agree; no GPU, no Python.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plan.h"

extern "C" int hostcheck_collect_below_batch(const uint8_t* msgs, const uint64_t* msg_off, uint64_t njobs,
                                             const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                                             uint32_t rchunk, int policy, uint64_t order_seed, uint64_t batch_bytes,
                                             int nshards, uint64_t buffer_entries, const uint64_t* out_off,
                                             uint64_t* out_nonces, uint64_t* out_hashes, uint64_t* out_totals,
                                             uint64_t* out_info);

namespace {

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
};

constexpr uint64_t kMark = 0xDEADBEEFull;

struct Batch {
    std::vector<uint8_t> msgs;
    std::vector<uint64_t> off{0}, lo, hi, target, out_off{0};
    void add(const std::vector<uint8_t>& m, uint64_t a, uint64_t b, uint64_t t, uint64_t cap) {
        msgs.insert(msgs.end(), m.begin(), m.end());
        off.push_back(msgs.size());
        lo.push_back(a);
        hi.push_back(b);
        target.push_back(t);
        out_off.push_back(out_off.back() + cap);
    }
};

// count_only: a null out_off, so every job only counts.
int check(const char* what, const Batch& b, uint32_t rchunk, int policy, uint64_t seed, uint64_t bytes, int nshards,
          uint64_t buffer, bool count_only, uint64_t min_sub_batches, bool must_rerun) {
    const size_t n = b.lo.size();
    std::vector<uint64_t> nonces(b.out_off.back(), kMark), hashes(b.out_off.back(), kMark), totals(n, kMark);
    uint64_t info[4];
    if (hostcheck_collect_below_batch(b.msgs.data(), b.off.data(), n, b.lo.data(), b.hi.data(), b.target.data(),
                                      rchunk, policy, seed, bytes, nshards, buffer,
                                      count_only ? nullptr : b.out_off.data(), count_only ? nullptr : nonces.data(),
                                      count_only ? nullptr : hashes.data(), totals.data(), info)) {
        std::printf("%s: the replay refused the batch\n", what);
        return 1;
    }
    if (info[0] > buffer || info[2] < min_sub_batches || (must_rerun && !info[1]) || (count_only && (info[0] || info[1]))) {
        std::printf("%s: list fill %llu of %llu, %llu jobs re-run, %llu sub-batches\n", what,
                    (unsigned long long)info[0], (unsigned long long)buffer, (unsigned long long)info[1],
                    (unsigned long long)info[2]);
        return 1;
    }
    for (size_t k = 0; k < n; k++) {
        const uint8_t* m = b.msgs.data() + b.off[k];
        const uint64_t len = b.off[k + 1] - b.off[k];
        const uint64_t cap = count_only ? 0 : b.out_off[k + 1] - b.out_off[k];
        uint64_t total = 0;
        bool same = true;
        for (uint64_t v = b.lo[k];; v++) {  // ascending: the lowest hits come first
            const uint64_t hv = gpuhash::hash_host(m, len, v);
            if (hv <= b.target[k]) {
                if (total < cap) same = same && nonces[b.out_off[k] + total] == v && hashes[b.out_off[k] + total] == hv;
                total++;
            }
            if (v == b.hi[k]) break;
        }
        for (uint64_t i = std::min(total, cap); i < cap; i++)  // untouched beyond
            same = same && nonces[b.out_off[k] + i] == kMark && hashes[b.out_off[k] + i] == kMark;
        if (totals[k] != total || !same) {
            std::printf("%s: job %zu [%llu, %llu] target %llu cap %llu: total %llu, want %llu%s\n", what, k,
                        (unsigned long long)b.lo[k], (unsigned long long)b.hi[k], (unsigned long long)b.target[k],
                        (unsigned long long)cap, (unsigned long long)totals[k], (unsigned long long)total,
                        same ? "" : ", and the list differs");
            return 1;
        }
    }
    return 0;
}

}  // namespace

int main() {
    Rng rng{2026};
    const uint64_t top = ~0ull;
    const uint64_t starts[] = {0, 9, 95, 990, 9900, 99990, 999900, 99999900ull, 9999999900ull, 999999999900ull,
                               9999999999999900ull, top - 450};
    const size_t lens[] = {0, 1, 8, 42, 50, 55, 58, 61, 63, 64, 120};
    // targets from "nothing qualifies" to "everything does"; room from none to more than the span
    const uint64_t targets[] = {0, top >> 8, top >> 4, top >> 1, top};
    const uint64_t caps[] = {0, 1, 5, 400};
    // 330 jobs: every message length at every start, spans of 1..300 nonces, clipped at 2^64-1
    Batch mixed;
    for (size_t li = 0; li < sizeof lens / sizeof *lens; li++) {
        std::vector<uint8_t> m(lens[li]);
        for (uint8_t& c : m) c = (uint8_t)rng.next();
        for (int rep = 0; rep < 30; rep++) {
            const uint64_t a = starts[rng.next() % (sizeof starts / sizeof *starts)] + rng.next() % 150;
            const uint64_t span = rng.next() % 300;
            mixed.add(m, a, top - a < span ? top : a + span, targets[rng.next() % 5], caps[rng.next() % 4]);
        }
    }
    // the top of uint64: the single nonce 2^64-1 as a hit and as none, ranges ending at it
    Batch high;
    const std::vector<uint8_t> brad = {'b', 'r', 'a', 'd', 'f', 'i', 't', 'z'}, none;
    const uint64_t htop = gpuhash::hash_host(brad.data(), brad.size(), top);
    high.add(brad, top, top, htop, 1);
    high.add(brad, top, top, htop - 1, 1);
    high.add(brad, top - 999, top, top >> 3, 50);
    high.add(none, top - 1200, top, top, 2000);
    high.add(brad, top - 1, top - 1, top, 0);
    high.add(std::vector<uint8_t>(50, 'q'), top - 700, top, top >> 1, 3);
    int bad = 0;
    const int policies[] = {0, 1, 2, 3, 16};
    for (int policy : policies) {
        bad += check("mixed", mixed, 0, policy, (uint64_t)policy, 0, 1, 1u << 20, false, 1, false);
        bad += check("mixed, a list of 64", mixed, 7, policy, 12345, 0, 1, 64, false, 1, true);
        bad += check("high", high, 7, policy, 1, 0, 2, 1u << 20, false, 1, false);
        bad += check("high, a list of 1", high, 0, policy, 987654321, 0, 1, 1, false, 1, true);
    }
    bad += check("mixed, a list of 1", mixed, 0, 0, 1, 0, 1, 1, false, 1, true);
    bad += check("mixed, a list of 8, sub-batches", mixed, 7, 0, 12345, 64 * 1024, 1, 8, false, 3, true);
    bad += check("mixed, sub-batches over three entries", mixed, 0, 0, 987654321, 96 * 1024, 3, 1000, false, 3, false);
    bad += check("mixed, one job per sub-batch", mixed, 0, 0, 1, 1, 1, 1u << 20, false, mixed.lo.size(), false);
    bad += check("mixed, counts only", mixed, 0, 0, 12345, 0, 2, 64, true, 1, false);
    if (bad) return 1;
    std::puts("ok");
    return 0;
}
