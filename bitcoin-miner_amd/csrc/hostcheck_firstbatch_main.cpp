// hostcheck_firstbatch_main.cpp -- TEST-ONLY stand-alone program over hostcheck_first_below_batch,
// for a sanitizer build (lib/hostcheck_firstbatch_asan: plan.cpp + hostcheck.cpp + this file under
// -fsanitize=address,undefined; tests/test_first_below_batch_cpu.py runs it).  It stages and
// replays first-hit batches on the CPU -- a few hundred jobs with targets of every kind, sub-batches,
// several context entries, the top of uint64 -- and checks every job against a plain ascending scan
// with hash_host that stops at its first hit, and what the replay hashed against the stage order's
// property.  Exit status 0 and "ok" when all agree; no GPU, no Python.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plan.h"

extern "C" int hostcheck_first_below_batch(const uint8_t* msgs, const uint64_t* msg_off, uint64_t njobs,
                                           const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                                           uint32_t rchunk, int policy, uint64_t order_seed, uint64_t batch_bytes,
                                           int nshards, uint64_t* out_hashes, uint64_t* out_nonces, int* out_found,
                                           uint64_t* out_trace, uint64_t* out_fill);

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
    std::vector<uint64_t> off{0}, lo, hi, target;
    // the ascending scan's answers
    std::vector<uint64_t> want_h, want_n;
    std::vector<int> want_found;

    // kind 0: target 0; 1: 2^64-1; 2: the least hash; 3: the median hash; 4: the least hash - 1
    void add(const std::vector<uint8_t>& m, uint64_t a, uint64_t b, int kind) {
        msgs.insert(msgs.end(), m.begin(), m.end());
        off.push_back(msgs.size());
        lo.push_back(a);
        hi.push_back(b);
        std::vector<uint64_t> h;
        for (uint64_t v = a;; v++) {
            h.push_back(gpuhash::hash_host(m.data(), m.size(), v));
            if (v == b) break;
        }
        std::vector<uint64_t> sorted = h;
        std::sort(sorted.begin(), sorted.end());
        const uint64_t least = sorted[0];
        const uint64_t t = kind == 0 ? 0 : kind == 1 ? ~0ull : kind == 2 ? least : kind == 3 ? sorted[h.size() / 2]
                                                                                 : least ? least - 1 : 0;
        target.push_back(t);
        size_t i = 0;
        while (i < h.size() && h[i] > t) i++;  // ascending, stops at its first hit
        want_found.push_back(i < h.size());
        want_h.push_back(i < h.size() ? h[i] : 0);
        want_n.push_back(i < h.size() ? a + i : 0);
    }
};

int digits(uint64_t n) {
    int d = 1;
    while (n >= 10) { n /= 10; d++; }
    return d;
}

int check(const char* what, const Batch& b, uint32_t rchunk, int policy, uint64_t seed, uint64_t bytes, int nshards,
          uint64_t min_sub_batches) {
    const size_t n = b.lo.size();
    const uint64_t mark = 0xDEADBEEFull;
    std::vector<uint64_t> h(n, mark), x(n, mark), trace(3 * n);
    std::vector<int> found(n, -1);
    uint64_t fill[4];
    if (int rc = hostcheck_first_below_batch(b.msgs.data(), b.off.data(), n, b.lo.data(), b.hi.data(), b.target.data(),
                                             rchunk, policy, seed, bytes, nshards, h.data(), x.data(), found.data(),
                                             trace.data(), fill)) {
        std::printf("%s: the replay returned %d\n", what, rc);
        return 1;
    }
    if (fill[2] || fill[0] > fill[1] || fill[3] < min_sub_batches) {
        std::printf("%s: list fill %llu of %llu, %llu runs over their bound, %llu sub-batches\n", what,
                    (unsigned long long)fill[0], (unsigned long long)fill[1], (unsigned long long)fill[2],
                    (unsigned long long)fill[3]);
        return 1;
    }
    for (size_t k = 0; k < n; k++) {
        const uint64_t span = b.hi[k] - b.lo[k] + 1, hashed = trace[3 * k], largest = trace[3 * k + 1],
                       upto = trace[3 * k + 2];
        bool ok = found[k] == b.want_found[k];
        if (ok && found[k]) {
            ok = h[k] == b.want_h[k] && x[k] == b.want_n[k];
            // the stage order's property, and no nonce below the answer left out
            ok = ok && digits(largest) <= digits(x[k]) && upto == x[k] - b.lo[k] + 1;
        } else if (ok) {
            ok = h[k] == mark && x[k] == mark && hashed == span;  // outputs untouched, everything hashed
        }
        if (!ok) {
            std::printf("%s: job %zu [%llu, %llu] target %llu: got %d (%llu, %llu), want %d (%llu, %llu); hashed %llu, "
                        "largest %llu, up to the answer %llu\n", what, k, (unsigned long long)b.lo[k],
                        (unsigned long long)b.hi[k], (unsigned long long)b.target[k], found[k], (unsigned long long)h[k],
                        (unsigned long long)x[k], b.want_found[k], (unsigned long long)b.want_h[k],
                        (unsigned long long)b.want_n[k], (unsigned long long)hashed, (unsigned long long)largest,
                        (unsigned long long)upto);
            return 1;
        }
    }
    return 0;
}

}  // namespace

int main() {
    Rng rng{2027};
    const uint64_t top = ~0ull;
    const uint64_t starts[] = {0, 9, 95, 990, 9900, 99990, 999900, 99999900ull, 9999999900ull, 999999999900ull,
                               9999999999999900ull, top - 450};
    const size_t lens[] = {0, 1, 8, 42, 50, 55, 58, 61, 63, 64, 120};
    // 330 jobs: every message length at every start, spans of 1..300 nonces, clipped at 2^64-1,
    // the five kinds of target in turn
    Batch mixed;
    int kind = 0;
    for (size_t li = 0; li < sizeof lens / sizeof *lens; li++) {
        std::vector<uint8_t> m(lens[li]);
        for (uint8_t& c : m) c = (uint8_t)rng.next();
        for (int rep = 0; rep < 30; rep++) {
            const uint64_t a = starts[rng.next() % (sizeof starts / sizeof *starts)] + rng.next() % 150;
            const uint64_t span = rng.next() % 300;
            mixed.add(m, a, top - a < span ? top : a + span, kind++ % 5);
        }
    }
    // ranges from 0 over several digit counts: the ascending digit order at work
    Batch low;
    for (int k = 0; k < 40; k++) {
        std::vector<uint8_t> m = {'p', 'o', 'w', '-', (uint8_t)('0' + k / 10), (uint8_t)('0' + k % 10)};
        if (k % 3 == 0) m.resize(61, 'x');
        low.add(m, k % 4 ? 0 : 7, 12000 + 100 * (uint64_t)k, 2 + k % 3);
    }
    // the top of uint64: the single nonce 2^64-1, ranges ending at it, an empty message
    Batch high;
    const std::vector<uint8_t> brad = {'b', 'r', 'a', 'd', 'f', 'i', 't', 'z'}, none;
    high.add(brad, top, top, 1);
    high.add(brad, top, top, 0);
    high.add(brad, top - 999, top, 2);
    high.add(none, top - 1200, top, 3);
    high.add(brad, top - 1, top - 1, 4);
    high.add(std::vector<uint8_t>(50, 'q'), top - 700, top, 2);
    int bad = 0;
    const int policies[] = {0, 1, 2, 3, 16};
    for (int policy : policies) {
        bad += check("mixed", mixed, 0, policy, (uint64_t)policy, 0, 1, 1);
        bad += check("low", low, policy == 2 ? 7 : 0, policy, 12345 + (uint64_t)policy, 0, 1, 1);
        bad += check("high", high, 7, policy, 1, 0, 2, 1);
    }
    bad += check("mixed, sub-batches", mixed, 7, 0, 12345, 64 * 1024, 1, 3);
    bad += check("mixed, sub-batches over three entries", mixed, 0, 0, 987654321, 96 * 1024, 3, 3);
    bad += check("mixed, one job per sub-batch", mixed, 0, 0, 1, 1, 1, mixed.lo.size());
    if (bad) return 1;
    std::puts("ok");
    return 0;
}
