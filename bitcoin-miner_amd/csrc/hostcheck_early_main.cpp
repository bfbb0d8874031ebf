// hostcheck_early_main.cpp -- TEST-ONLY stand-alone program over hostcheck_first_below_batch_early,
// for a sanitizer build (lib/hostcheck_early_asan: plan.cpp + hostcheck.cpp + this file under
// -fsanitize=address,undefined; tests/test_first_below_early_cpu.py runs it).  It replays the packed
// rounds and the remainder on the CPU -- digit boundaries inside a chunk and between rounds, the top
// of uint64, a prefix of 1 and of the whole span and more, sub-batches and three context entries --
// and checks every job against a plain ascending scan with hash_host that stops at its first hit,
// the packed nonces against 2x + c_0, and every round's list against its capacity.  Exit status 0
// and "ok" when all agree; no GPU, no Python.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plan.h"

extern "C" int hostcheck_first_below_batch_early(const uint8_t* msgs, const uint64_t* msg_off, uint64_t njobs,
                                                 const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                                                 uint64_t prefix, uint32_t rchunk, int policy, uint64_t order_seed,
                                                 uint64_t batch_bytes, int nshards, uint64_t* out_hashes,
                                                 uint64_t* out_nonces, int* out_found, uint64_t* out_packed,
                                                 uint64_t* out_fill);
extern "C" uint64_t hostcheck_early_limit(uint64_t lower, uint64_t upper, uint64_t target, uint64_t prefix);

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
    std::vector<uint64_t> want_h, want_n;  // the ascending scan's answers
    std::vector<int> want_found;

    // kind 0: target 0; 1: 2^64-1; 2: the least hash; 3: the median hash; 4: the least hash - 1;
    // 5: the least hash from offset `from` on
    void add(const std::vector<uint8_t>& m, uint64_t a, uint64_t b, int kind, uint64_t from = 0) {
        msgs.insert(msgs.end(), m.begin(), m.end());
        off.push_back(msgs.size());
        lo.push_back(a);
        hi.push_back(b);
        std::vector<uint64_t> h;
        for (uint64_t v = a;; v++) {
            h.push_back(gpuhash::hash_host(m.data(), m.size(), v));
            if (v == b) break;
        }
        std::vector<uint64_t> sorted(h.begin() + (long)(kind == 5 ? from : 0), h.end());
        std::sort(sorted.begin(), sorted.end());
        const uint64_t least = sorted[0];
        const uint64_t t = kind == 0 ? 0 : kind == 1 ? ~0ull : kind == 3 ? sorted[sorted.size() / 2]
                           : kind == 4 ? (least ? least - 1 : 0) : least;
        target.push_back(t);
        size_t i = 0;
        while (i < h.size() && h[i] > t) i++;  // ascending, stops at its first hit
        want_found.push_back(i < h.size());
        want_h.push_back(i < h.size() ? h[i] : 0);
        want_n.push_back(i < h.size() ? a + i : 0);
    }
};

int check(const char* what, const Batch& b, uint64_t prefix, uint32_t rchunk, int policy, uint64_t seed, uint64_t bytes,
          int nshards, uint64_t min_stages) {
    const size_t n = b.lo.size();
    const uint64_t mark = 0xDEADBEEFull;
    std::vector<uint64_t> h(n, mark), x(n, mark), packed(n);
    std::vector<int> found(n, -1);
    uint64_t fill[6];
    if (int rc = hostcheck_first_below_batch_early(b.msgs.data(), b.off.data(), n, b.lo.data(), b.hi.data(),
                                                   b.target.data(), prefix, rchunk, policy, seed, bytes, nshards,
                                                   h.data(), x.data(), found.data(), packed.data(), fill)) {
        std::printf("%s: the replay returned %d\n", what, rc);
        return 1;
    }
    if (fill[2] || fill[4] || fill[0] > fill[1] || fill[3] < min_stages) {
        std::printf("%s: list fill %llu of %llu, %llu + %llu stages over their bound, %llu round stages\n", what,
                    (unsigned long long)fill[0], (unsigned long long)fill[1], (unsigned long long)fill[2],
                    (unsigned long long)fill[4], (unsigned long long)fill[3]);
        return 1;
    }
    for (size_t k = 0; k < n; k++) {
        const uint64_t limit = hostcheck_early_limit(b.lo[k], b.hi[k], b.target[k], prefix);
        bool ok = found[k] == b.want_found[k] && packed[k] <= limit;
        if (ok && found[k]) {
            const uint64_t at = x[k] - b.lo[k];  // the work bound, for an answer inside the front
            ok = h[k] == b.want_h[k] && x[k] == b.want_n[k] && (at >= limit || packed[k] <= 2 * at + fill[5]);
        } else if (ok) {
            ok = h[k] == mark && x[k] == mark && packed[k] == limit;  // outputs untouched, the whole front hashed
        }
        if (!ok) {
            std::printf("%s: job %zu [%llu, %llu] target %llu: got %d (%llu, %llu), want %d (%llu, %llu); packed %llu of "
                        "%llu, c_0 %llu\n", what, k, (unsigned long long)b.lo[k], (unsigned long long)b.hi[k],
                        (unsigned long long)b.target[k], found[k], (unsigned long long)h[k], (unsigned long long)x[k],
                        b.want_found[k], (unsigned long long)b.want_h[k], (unsigned long long)b.want_n[k],
                        (unsigned long long)packed[k], (unsigned long long)limit, (unsigned long long)fill[5]);
            return 1;
        }
    }
    return 0;
}

}  // namespace

int main() {
    Rng rng{2028};
    const uint64_t top = ~0ull;
    const uint64_t starts[] = {0, 9, 95, 990, 9900, 99990, 999900, 99999900ull, 9999999900ull, 999999999900ull,
                               9999999999999900ull, top - 450};
    const size_t lens[] = {0, 1, 8, 42, 50, 55, 58, 61, 63, 64, 120, 1300};
    // every message length at every start, spans of 1..300 nonces, clipped at 2^64-1, five kinds of target
    Batch mixed;
    int kind = 0;
    for (size_t li = 0; li < sizeof lens / sizeof *lens; li++) {
        std::vector<uint8_t> m(lens[li]);
        for (uint8_t& c : m) c = (uint8_t)rng.next();
        for (int rep = 0; rep < 16; rep++) {
            const uint64_t a = starts[rng.next() % (sizeof starts / sizeof *starts)] + rng.next() % 150;
            const uint64_t span = rng.next() % 300;
            mixed.add(m, a, top - a < span ? top : a + span, kind++ % 5);
        }
    }
    // a digit boundary five nonces into the first chunk, and the answer some rounds later: across
    // 10^d inside a chunk and between rounds, and the top of uint64
    Batch cross;
    const uint64_t lows[] = {95, 9990, 99999990ull, 10000000000000000000ull - 100, top - 5000};
    for (size_t i = 0; i < 5; i++) {
        std::vector<uint8_t> m = {'s', 't', 'a', 'm', 'p', (uint8_t)('0' + i)};
        if (i % 2) m.resize(57, 'y');
        cross.add(m, lows[i], lows[i] + 5000, 5, 3000);
    }
    cross.add({'b', 'r', 'a', 'd'}, top, top, 1);
    cross.add({'b', 'r', 'a', 'd'}, top, top, 0);
    // 1100 two-nonce jobs beside them bring c_0 down to 1024: the answers from offset 3000 on then
    // lie in the second round [1024, 3072) or the third [3072, 7168)
    for (uint64_t i = 0; i < 1100; i++) cross.add({'f', (uint8_t)i, (uint8_t)(i >> 8)}, 98 + i % 3, 99 + i % 3, 1 + i % 2);
    int bad = 0;
    const uint64_t prefixes[] = {0, 1, 64, 1000, 5001, 1ull << 20};
    for (uint64_t prefix : prefixes) {
        bad += check("mixed", mixed, prefix, prefix == 64 ? 7 : 0, (int)(prefix % 4), prefix, 0, 1, 1);
        bad += check("cross", cross, prefix, 0, 0, 12345 + prefix, 0, 1, 1);
        bad += check("cross, descending", cross, prefix, 7, 16, 1, 0, 2, 1);
    }
    bad += check("mixed, sub-batches", mixed, 1ull << 20, 7, 0, 12345, 16 * 1024, 1, 3);
    bad += check("mixed, sub-batches over three entries", mixed, 1000, 0, 0, 987654321, 16 * 1024, 3, 3);
    bad += check("cross over three entries", cross, 1ull << 20, 0, 3, 987654321, 0, 3, 3);
    bad += check("mixed, one job per sub-batch", mixed, 64, 0, 0, 1, 1, 1, mixed.lo.size());
    if (bad) return 1;
    std::puts("ok");
    return 0;
}
