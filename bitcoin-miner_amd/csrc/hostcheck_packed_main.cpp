// hostcheck_packed_main.cpp -- TEST-ONLY stand-alone program over the packed replay of
// hostcheck_min_batch and hostcheck_collect_below_batch (GPUHASH_LAYOUT_PACKED_ALWAYS), for a
// sanitizer build (lib/hostcheck_packed_asan: plan.cpp + hostcheck.cpp + this file under
// -fsanitize=address,undefined; tests/test_packed_cpu.py runs it).  It stages and replays flagged
// batches on the CPU -- every message length mod 64 at several digit counts, digit boundaries,
// the top of uint64, jobs above the cap beside packed ones, sub-batches, several entries, a short
// collect list -- and checks every job against a plain ascending scan with hash_host.  Exit
// status 0 and "ok" when all agree; no GPU, no Python.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plan.h"

extern "C" int hostcheck_min_batch(const uint8_t* msgs, const uint64_t* msg_off, uint64_t njobs,
                                   const uint64_t* lower, const uint64_t* upper, uint32_t rchunk, int policy,
                                   uint64_t order_seed, uint64_t batch_bytes, int nshards, uint64_t* out_hashes,
                                   uint64_t* out_nonces, uint64_t* out_fill);
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

struct Batch {
    std::vector<uint8_t> msgs;
    std::vector<uint64_t> off{0}, lo, hi;
    mutable std::vector<std::vector<uint64_t>> scans;  // scan()'s results, kept
    void add(const std::vector<uint8_t>& m, uint64_t a, uint64_t b) {
        msgs.insert(msgs.end(), m.begin(), m.end());
        off.push_back(msgs.size());
        lo.push_back(a);
        hi.push_back(b);
    }
};

// The hashes of job k, ascending.
const std::vector<uint64_t>& scan(const Batch& b, size_t k) {
    b.scans.resize(b.lo.size());
    std::vector<uint64_t>& h = b.scans[k];
    if (!h.empty()) return h;
    for (uint64_t v = b.lo[k];; v++) {
        h.push_back(gpuhash::hash_host(b.msgs.data() + b.off[k], b.off[k + 1] - b.off[k], v));
        if (v == b.hi[k]) break;
    }
    return h;
}

int check_min(const char* what, const Batch& b, int policy, uint64_t seed, uint64_t bytes, int nshards) {
    const size_t n = b.lo.size();
    std::vector<uint64_t> h(n), x(n);
    uint64_t fill[4];
    if (hostcheck_min_batch(b.msgs.data(), b.off.data(), n, b.lo.data(), b.hi.data(), 0, policy, seed, bytes, nshards,
                            h.data(), x.data(), fill)) {
        std::printf("%s: the replay refused the batch\n", what);
        return 1;
    }
    if (fill[2] || fill[0] > fill[1]) {
        std::printf("%s: list fill %llu of %llu, %llu runs over their bound\n", what, (unsigned long long)fill[0],
                    (unsigned long long)fill[1], (unsigned long long)fill[2]);
        return 1;
    }
    for (size_t k = 0; k < n; k++) {
        const std::vector<uint64_t>& hs = scan(b, k);
        const size_t i = (size_t)(std::min_element(hs.begin(), hs.end()) - hs.begin());  // the first of equals
        if (h[k] != hs[i] || x[k] != b.lo[k] + i) {
            std::printf("%s: min job %zu [%llu, %llu]: got (%llu, %llu), want (%llu, %llu)\n", what, k,
                        (unsigned long long)b.lo[k], (unsigned long long)b.hi[k], (unsigned long long)h[k],
                        (unsigned long long)x[k], (unsigned long long)hs[i], (unsigned long long)(b.lo[k] + i));
            return 1;
        }
    }
    return 0;
}

// Targets at the lower quartile of each job's hashes; every third job counts only.
int check_collect(const char* what, const Batch& b, int policy, uint64_t seed, uint64_t buffer, int nshards) {
    const size_t n = b.lo.size();
    std::vector<uint64_t> target(n), off(n + 1, 0), totals(n), info(4);
    std::vector<std::vector<uint64_t>> hs(n);
    for (size_t k = 0; k < n; k++) {
        hs[k] = scan(b, k);
        std::vector<uint64_t> s = hs[k];
        std::sort(s.begin(), s.end());
        target[k] = s[s.size() / 4];
        off[k + 1] = off[k] + (k % 3 == 2 ? 0 : hs[k].size());
    }
    std::vector<uint64_t> on(off[n] + 1), oh(off[n] + 1);
    if (hostcheck_collect_below_batch(b.msgs.data(), b.off.data(), n, b.lo.data(), b.hi.data(), target.data(), 0, policy,
                                      seed, 0, nshards, buffer, off.data(), on.data(), oh.data(), totals.data(),
                                      info.data())) {
        std::printf("%s: the collect replay refused the batch\n", what);
        return 1;
    }
    for (size_t k = 0; k < n; k++) {
        std::vector<uint64_t> want;
        for (size_t i = 0; i < hs[k].size(); i++)
            if (hs[k][i] <= target[k]) want.push_back(b.lo[k] + i);
        bool ok = totals[k] == want.size();
        for (size_t i = 0; ok && off[k + 1] > off[k] && i < want.size(); i++)
            ok = on[off[k] + i] == want[i] && oh[off[k] + i] == hs[k][want[i] - b.lo[k]];
        if (!ok) {
            std::printf("%s: collect job %zu [%llu, %llu]: total %llu, want %zu, or its list differs\n", what, k,
                        (unsigned long long)b.lo[k], (unsigned long long)b.hi[k], (unsigned long long)totals[k],
                        want.size());
            return 1;
        }
    }
    return 0;
}

}  // namespace

int main() {
    Rng rng{2027};
    const uint64_t top = ~0ull;
    const int packed = 64;  // GPUHASH_LAYOUT_PACKED_ALWAYS
    // every message length mod 64, and some beyond one block, at a few digit boundaries each
    const uint64_t starts[] = {0, 7, 95, 9990, 999990, 99999995ull, 99999999995ull, 9999999999999990ull, top - 40};
    Batch classes;
    for (size_t len = 0; len < 64 + 8; len++) {
        const size_t mlen = len < 64 ? len : (len - 64) * 37 + 64;
        std::vector<uint8_t> m(mlen);
        for (uint8_t& c : m) c = (uint8_t)rng.next();
        for (int rep = 0; rep < 3; rep++) {
            const uint64_t a = starts[rng.next() % (sizeof starts / sizeof *starts)] + rng.next() % 5;
            const uint64_t span = rng.next() % 40;
            classes.add(m, a, top - a < span ? top : a + span);
        }
    }
    // jobs of many tiles, a job above the cap (it runs unpacked beside the packed ones), the top
    Batch wide;
    const std::vector<uint8_t> brad = {'b', 'r', 'a', 'd', 'f', 'i', 't', 'z'}, none;
    wide.add(brad, 0, 2999);
    wide.add(std::vector<uint8_t>(61, 'q'), 99000, 101500);
    wide.add(brad, 5, (1ull << 20) + 5);
    wide.add(none, top - 700, top);
    wide.add(brad, top, top);
    for (int i = 0; i < 40; i++) wide.add(std::vector<uint8_t>(i, (uint8_t)('a' + i % 26)), 990 + i, 1010 + 2 * i);
    int bad = 0;
    const int policies[] = {0, 2, 16};
    for (int policy : policies)
        for (uint64_t seed : {0ull, 1ull, 77ull}) {
            bad += check_min("classes", classes, policy | packed, seed, 0, 1);
            bad += check_collect("classes", classes, policy | packed, seed, 1 << 20, 1);
        }
    bad += check_min("wide, sub-batches over three entries", wide, packed, 9, 96 * 1024, 3);
    bad += check_collect("wide, a short list over two entries", wide, packed, 11, 64, 2);
    if (bad) return 1;
    std::puts("ok");
    return 0;
}
