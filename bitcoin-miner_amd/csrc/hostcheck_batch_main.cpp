// hostcheck_batch_main.cpp -- TEST-ONLY stand-alone program over hostcheck_min_batch, for a
// sanitizer build (lib/hostcheck_batch_asan: plan.cpp + hostcheck.cpp + this file under
// -fsanitize=address,undefined; tests/test_min_batch_cpu.py runs it).  It stages and replays
// batches on the CPU -- a few hundred jobs, sub-batches, several context entries, the top of
// uint64 -- and checks every job against a plain ascending scan with hash_host.  Exit status 0
// and "ok" when all agree; no GPU, no Python.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plan.h"

extern "C" int hostcheck_min_batch(const uint8_t* msgs, const uint64_t* msg_off, uint64_t njobs,
                                   const uint64_t* lower, const uint64_t* upper, uint32_t rchunk, int policy,
                                   uint64_t order_seed, uint64_t batch_bytes, int nshards, uint64_t* out_hashes,
                                   uint64_t* out_nonces, uint64_t* out_fill);

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
    void add(const std::vector<uint8_t>& m, uint64_t a, uint64_t b) {
        msgs.insert(msgs.end(), m.begin(), m.end());
        off.push_back(msgs.size());
        lo.push_back(a);
        hi.push_back(b);
    }
};

int check(const char* what, const Batch& b, uint32_t rchunk, int policy, uint64_t seed, uint64_t bytes, int nshards,
          uint64_t min_sub_batches) {
    const size_t n = b.lo.size();
    std::vector<uint64_t> h(n), x(n);
    uint64_t fill[4];
    if (hostcheck_min_batch(b.msgs.data(), b.off.data(), n, b.lo.data(), b.hi.data(), rchunk, policy, seed, bytes,
                            nshards, h.data(), x.data(), fill)) {
        std::printf("%s: the replay refused the batch\n", what);
        return 1;
    }
    if (fill[2] || fill[0] > fill[1] || fill[3] < min_sub_batches) {
        std::printf("%s: list fill %llu of %llu, %llu runs over their bound, %llu sub-batches\n", what,
                    (unsigned long long)fill[0], (unsigned long long)fill[1], (unsigned long long)fill[2],
                    (unsigned long long)fill[3]);
        return 1;
    }
    for (size_t k = 0; k < n; k++) {
        const uint8_t* m = b.msgs.data() + b.off[k];
        const uint64_t len = b.off[k + 1] - b.off[k];
        uint64_t bh = 0, bn = 0;
        bool any = false;
        for (uint64_t v = b.lo[k];; v++) {  // ascending, strict '<': the lowest nonce wins ties
            const uint64_t hv = gpuhash::hash_host(m, len, v);
            if (!any || hv < bh) { bh = hv; bn = v; any = true; }
            if (v == b.hi[k]) break;
        }
        if (h[k] != bh || x[k] != bn) {
            std::printf("%s: job %zu [%llu, %llu]: got (%llu, %llu), want (%llu, %llu)\n", what, k,
                        (unsigned long long)b.lo[k], (unsigned long long)b.hi[k], (unsigned long long)h[k],
                        (unsigned long long)x[k], (unsigned long long)bh, (unsigned long long)bn);
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
    // 330 jobs: every message length at every start, spans of 1..300 nonces, clipped at 2^64-1
    Batch mixed;
    for (size_t li = 0; li < sizeof lens / sizeof *lens; li++) {
        std::vector<uint8_t> m(lens[li]);
        for (uint8_t& c : m) c = (uint8_t)rng.next();
        for (int rep = 0; rep < 30; rep++) {
            const uint64_t a = starts[rng.next() % (sizeof starts / sizeof *starts)] + rng.next() % 150;
            const uint64_t span = rng.next() % 300;
            mixed.add(m, a, top - a < span ? top : a + span);
        }
    }
    // the top of uint64: the single nonce 2^64-1, ranges ending at it, an empty message
    Batch high;
    const std::vector<uint8_t> brad = {'b', 'r', 'a', 'd', 'f', 'i', 't', 'z'}, none;
    high.add(brad, top, top);
    high.add(brad, top - 999, top);
    high.add(none, top - 1200, top);
    high.add(brad, top - 1, top - 1);
    high.add(std::vector<uint8_t>(50, 'q'), top - 700, top);
    int bad = 0;
    const int policies[] = {0, 1, 2, 3, 16};
    for (int policy : policies) {
        bad += check("mixed", mixed, 0, policy, (uint64_t)policy, 0, 1, 1);
        bad += check("high", high, 7, policy, 1, 0, 2, 1);
    }
    bad += check("mixed, sub-batches", mixed, 7, 0, 12345, 64 * 1024, 1, 3);
    bad += check("mixed, sub-batches over three entries", mixed, 0, 0, 987654321, 96 * 1024, 3, 3);
    bad += check("mixed, one job per sub-batch", mixed, 0, 0, 1, 1, 1, mixed.lo.size());
    if (bad) return 1;
    std::puts("ok");
    return 0;
}
