// pack.h -- the packed layout for tiny batch jobs (gpuhash_min_batch and
// gpuhash_collect_below_batch under GPUHASH_LAYOUT_PACKED_ALWAYS): every lane
// hashes one (job, nonce) from the job's midstate.  Everything that decides which bytes a lane
// hashes is here, once: the kernel (pack_kernel.hip) and the CPU replay (hostcheck.cpp) call the
// same functions, as they share part_min_nonce (plan.h).  Plain C++, no HIP.
//
//   job record  the chaining value after all whole 64-byte blocks of the message, the tail
//               words (the last m mod 64 message bytes, then ' ', zero-padded), the message's
//               bits before the digits, and the job's index in the batch stage
//   segment     a job's nonces of one digit count d
//   class       (o = m mod 64, d): it fixes every digit's byte position, where 0x80 goes and
//               whether the tail is one block or two.  (The length field is per job: it depends
//               on m, not only on o.)
//   tile        256 consecutive items of one class's flattened nonce space -- the class's
//               segments end to end, in job order -- with the first and last segment a lane of
//               it can belong to.  One workgroup pass; o and d are uniform in it.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "plan.h"

#if defined(__clang__)
#define GPUHASH_UNROLL _Pragma("unroll")
#else
#define GPUHASH_UNROLL
#endif

namespace gpuhash {

constexpr uint32_t kPackTile = 256;
constexpr uint64_t kPackMaxSpan = GPUHASH_PACKED_MAX_SPAN;
// tiles per grab, at most: clamp(remaining / (2 * grid), 1, kPackMaxPiece), k_scan's rule
constexpr uint32_t kPackMaxPiece = 8;
constexpr uint32_t kPackNoJob = 0xFFFFFFFFu;

struct PackJob {
    uint32_t cv[8];
    uint32_t tail[16];
    uint64_t bits;  // 8 * (m + 1): the hashed bits before the digits
    uint32_t job;   // the job's index in its stage: its per-job words and the tag of its entries
    uint32_t pad_;
};

struct PackSeg {
    uint64_t start;  // position of its first item in its class's flattened space
    uint64_t n0;     // its first nonce
    uint32_t count;  // <= kPackMaxSpan
    uint32_t rec;    // its job's record
};

struct PackTile {
    uint64_t item0;               // the class-space position of lane 0
    uint32_t seg_first, seg_last;  // the segments of lane 0 and of the tile's last live lane
    uint32_t o, d;
};

// Tail blocks of class (o, d): o + 1 bytes of message and ' ', d digits, 0x80 and 8 length bytes.
GPUHASH_HD inline int pack_blocks(uint32_t o, uint32_t d) { return o + d + 10u > 64u ? 2 : 1; }

// A segment of c consecutive class-space items meets at most this many of the 64-item windows
// its class's space is cut into (a window is one wave of one tile): an interval of c items that
// starts a <= 63 items into a window ends in window floor((a + c - 1) / 64).  Every tile is taken
// once (the work counter), and a wave appends at most one entry per job it holds lanes of
// (k_pack), so this bounds a segment's result-list entries.
inline uint64_t pack_seg_entries(uint64_t c) { return (c + 62) / 64 + 1; }

GPUHASH_HD constexpr uint32_t pack_k(int t) {
    constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
        0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
        0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
        0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
        0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
        0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
        0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    return K[t];
}

GPUHASH_HD inline uint32_t pack_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// One SHA-256 compression of the 16 words w (used up as the rolling schedule) into st.
GPUHASH_HD inline void pack_compress(uint32_t (&st)[8], uint32_t (&w)[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    GPUHASH_UNROLL
    for (int t = 0; t < 64; t++) {
        if (t >= 16) {
            const uint32_t w15 = w[(t - 15) & 15], w2 = w[(t - 2) & 15];
            w[t & 15] += (pack_rotr(w15, 7) ^ pack_rotr(w15, 18) ^ (w15 >> 3)) + w[(t - 7) & 15] +
                         (pack_rotr(w2, 17) ^ pack_rotr(w2, 19) ^ (w2 >> 10));
        }
        const uint32_t t1 = h + (pack_rotr(e, 6) ^ pack_rotr(e, 11) ^ pack_rotr(e, 25)) + ((e & f) ^ (~e & g)) +
                            pack_k(t) + w[t & 15];
        const uint32_t t2 = (pack_rotr(a, 2) ^ pack_rotr(a, 13) ^ pack_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g; g = f; f = e; e = d + t1;
        d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d;
    st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// x < 10^4 as four ASCII digits, most significant in the top byte.
GPUHASH_HD inline uint32_t pack_ascii4(uint32_t x) {
    const uint32_t a = x / 1000u, r = x - a * 1000u, b = r / 100u, s = r - b * 100u, c = s / 10u;
    return 0x30303030u + ((a << 24) | (b << 16) | (c << 8) | (s - c * 10u));
}

// The 20 decimal digits of n, right-aligned with leading '0's, as 5 big-endian words: exact for
// every n up to 2^64-1 (n = a * 10^16 + b * 10^8 + c, a <= 1844).
GPUHASH_HD inline void pack_digits20(uint64_t n, uint32_t (&R)[6]) {
    const uint64_t hi = n / 100000000ull;
    const uint32_t c = (uint32_t)(n - hi * 100000000ull);
    const uint32_t a = (uint32_t)(hi / 100000000ull), b = (uint32_t)(hi - (uint64_t)a * 100000000ull);
    const uint32_t b1 = b / 10000u, c1 = c / 10000u;
    R[0] = pack_ascii4(a);
    R[1] = pack_ascii4(b1);
    R[2] = pack_ascii4(b - b1 * 10000u);
    R[3] = pack_ascii4(c1);
    R[4] = pack_ascii4(c - c1 * 10000u);
}

// The tail block(s) of nonce n (d digits) of a job whose record holds `tail` and `bits`, class
// (o, d): w[0..15], and w[16..31] when pack_blocks(o, d) is 2.  The digits and the 0x80 after
// them are one 21-byte string, shifted as a whole by amounts that depend on (o, d) only -- uniform
// in a tile -- and every array index below is a constant once the loops are unrolled: nothing is
// indexed by a run-time value.
GPUHASH_HD inline void pack_build(const uint32_t (&tail)[16], uint64_t bits, uint32_t o, uint32_t d, uint64_t n,
                                  uint32_t (&w)[32]) {
    GPUHASH_UNROLL
    for (int j = 0; j < 16; j++) { w[j] = tail[j]; w[16 + j] = 0u; }
    uint32_t R[6];
    pack_digits20(n, R);
    R[5] = 0x80000000u;
    // the 20 - d leading pad digits go
    const uint32_t pad = 20u - d;
    GPUHASH_UNROLL
    for (int k = 0; k < 5; k++) {
        const uint32_t z = pad > 4u * k ? pad - 4u * k : 0u;  // bytes of word k to clear, from the top
        R[k] = z >= 4u ? 0u : R[k] & (0xFFFFFFFFu >> (8u * z));
    }
    // In a virtual array V of 5 + 32 words, V[5 + j] = w[j], byte 0 of R lands at byte
    // o + 1 + d: its byte 20 - d, the first digit, is then byte o + 1 of the block.
    const uint32_t pos = o + 1u + d, sh = (pos & 3u) * 8u, q = pos >> 2;  // q <= 21
    uint32_t T[7];
    T[0] = R[0] >> sh;
    GPUHASH_UNROLL
    for (int k = 1; k < 6; k++) T[k] = (uint32_t)((((uint64_t)R[k - 1] << 32) | R[k]) >> sh);
    T[6] = (uint32_t)(((uint64_t)R[5] << 32) >> sh);
    // V[q + k] = T[k]: T moved up by q words in five binary stages of constant-index moves (a
    // loop over the 22 values of q with `w[qq + k - 5] |= T[k]` inside came back from the compiler
    // as one run-time index, and w in scratch)
    uint32_t V[28];
    GPUHASH_UNROLL
    for (int j = 0; j < 28; j++) V[j] = j < 7 ? T[j] : 0u;
    GPUHASH_UNROLL
    for (int s = 0; s < 5; s++) {
        const bool up = (q >> s) & 1u;
        GPUHASH_UNROLL
        for (int j = 27; j >= 0; j--) V[j] = up ? (j >= (1 << s) ? V[j - (1 << s) < 0 ? 0 : j - (1 << s)] : 0u) : V[j];
    }
    GPUHASH_UNROLL
    for (int j = 0; j < 23; j++) w[j] |= V[j + 5];
    const uint64_t len = bits + 8ull * d;
    if (pack_blocks(o, d) == 1) {
        w[14] |= (uint32_t)(len >> 32);
        w[15] |= (uint32_t)len;
    } else {
        w[30] = (uint32_t)(len >> 32);
        w[31] = (uint32_t)len;
    }
}

// Hash(msg, n) of the job of `rec`, n a d-digit nonce, class (o, d): the first two words of the
// digest.
GPUHASH_HD inline void pack_hash(const PackJob& rec, uint32_t o, uint32_t d, uint64_t n, uint32_t& H0, uint32_t& H1) {
    uint32_t w[32], st[8], tail[16];
    GPUHASH_UNROLL
    for (int j = 0; j < 16; j++) tail[j] = rec.tail[j];
    GPUHASH_UNROLL
    for (int j = 0; j < 8; j++) st[j] = rec.cv[j];
    pack_build(tail, rec.bits, o, d, n, w);
    uint32_t b0[16];
    GPUHASH_UNROLL
    for (int j = 0; j < 16; j++) b0[j] = w[j];
    pack_compress(st, b0);
    if (pack_blocks(o, d) == 2) {
        uint32_t b1[16];
        GPUHASH_UNROLL
        for (int j = 0; j < 16; j++) b1[j] = w[16 + j];
        pack_compress(st, b1);
    }
    H0 = st[0];
    H1 = st[1];
}

// The segment of `item` among a tile's: the largest s in [first, last] with segs[s].start <=
// item.  A tile spans at most 256 segments, so 8 halvings settle it.
GPUHASH_HD inline uint32_t pack_find_seg(const PackSeg* segs, uint32_t first, uint32_t last, uint64_t item) {
    uint32_t lo = first, hi = last;
    for (int it = 0; it < 9 && lo < hi; it++) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (segs[mid].start <= item) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

// ---- host only: the tables of a stage's packed jobs ----

struct PackTables {
    std::vector<PackJob> recs;
    std::vector<PackSeg> segs;  // by class, then by job
    std::vector<PackTile> tiles;
    uint64_t nonces = 0;
    uint64_t entries = 0;  // the sum of pack_seg_entries: the min mode's result-list bound
    int blocks = 0;        // the most tail blocks of any segment

    bool empty() const { return recs.empty(); }

    // The record of a message: its midstate over the whole blocks and its tail.  (`job` is the
    // stage's to set, add_job.)
    static PackJob record(const uint8_t* msg, uint64_t len) {
        PackJob r{};
        std::copy(kIV, kIV + 8, r.cv);
        const uint64_t whole = len / 64, o = len % 64;
        for (uint64_t b = 0; b < whole; b++) {
            uint32_t w[16];
            for (int j = 0; j < 16; j++) {
                const uint8_t* p = msg + 64 * b + 4 * j;
                w[j] = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
            }
            sha256_compress(r.cv, w);
        }
        for (uint64_t i = 0; i <= o; i++) {
            const uint8_t c = i < o ? msg[64 * whole + i] : (uint8_t)' ';
            r.tail[i >> 2] |= (uint32_t)c << (24 - 8 * (i & 3));
        }
        r.bits = 8 * (len + 1);
        return r;
    }

    // Adds job `job` of the stage: msg of len bytes over [lo, hi], hi - lo < kPackMaxSpan.
    void add_job(uint32_t job, const uint8_t* msg, uint64_t len, uint64_t lo, uint64_t hi) {
        add_job(job, record(msg, len), lo, hi);
    }

    // The same from a record built before (record()): a caller that stages one job many times
    // (the rounds of gpuhash_first_below_batch_early) compresses its whole blocks once.
    void add_job(uint32_t job, const PackJob& built, uint64_t lo, uint64_t hi) {
        PackJob r = built;
        r.job = job;
        const uint32_t o = (uint32_t)(r.bits / 8 - 1) % 64;
        const uint32_t rec = (uint32_t)recs.size();
        recs.push_back(r);
        for (int d = num_digits(lo); d <= num_digits(hi); d++) {
            const uint64_t a = std::max<uint64_t>(lo, d == 1 ? 0 : pow10u(d - 1));
            const uint64_t b = d == 20 ? hi : std::min(hi, pow10u(d) - 1);
            pend_.push_back(Pending{(uint32_t)o, (uint32_t)d, PackSeg{0, a, (uint32_t)(b - a + 1), rec}});
            nonces += b - a + 1;
            entries += pack_seg_entries(b - a + 1);
            blocks = std::max(blocks, pack_blocks((uint32_t)o, (uint32_t)d));
        }
    }

    // Orders the segments by class and cuts every class's space into tiles.
    void finish() {
        std::stable_sort(pend_.begin(), pend_.end(), [](const Pending& x, const Pending& y) {
            return x.o != y.o ? x.o < y.o : x.d < y.d;
        });
        for (size_t i = 0; i < pend_.size();) {
            size_t e = i;
            uint64_t total = 0;
            for (; e < pend_.size() && pend_[e].o == pend_[i].o && pend_[e].d == pend_[i].d; e++) {
                pend_[e].seg.start = total;
                total += pend_[e].seg.count;
                segs.push_back(pend_[e].seg);
            }
            size_t s = i, t = i;  // the segments of a tile's first and last item
            for (uint64_t item0 = 0; item0 < total; item0 += kPackTile) {
                const uint64_t last = std::min(item0 + kPackTile, total) - 1;
                while (s + 1 < e && pend_[s + 1].seg.start <= item0) s++;
                while (t + 1 < e && pend_[t + 1].seg.start <= last) t++;
                tiles.push_back(PackTile{item0, (uint32_t)s, (uint32_t)t, pend_[i].o, pend_[i].d});
            }
            i = e;
        }
        pend_.clear();
    }

   private:
    struct Pending {
        uint32_t o, d;
        PackSeg seg;
    };
    std::vector<Pending> pend_;
};

// The metadata bytes a packed job adds to a batch stage, at most (batch_job_bytes' counterpart,
// stage.h): its record, its per-job words and share of the list head, and per digit count a
// segment, the tiles its items can open (one more than they fill) and, unless the stage collects,
// its result-list entries; then the packed group's own counter block, offset word and alignment
// gaps, priced on every job.
inline uint64_t pack_job_bytes(uint64_t lo, uint64_t hi, bool collects) {
    uint64_t b = sizeof(PackJob) + (collects ? 24 : 8) + 16 + 40 + 8 + 5 * 16;
    for (int d = num_digits(lo); d <= num_digits(hi); d++) {
        const uint64_t a = std::max<uint64_t>(lo, d == 1 ? 0 : pow10u(d - 1));
        const uint64_t e = d == 20 ? hi : std::min(hi, pow10u(d) - 1);
        const uint64_t c = e - a + 1;
        b += sizeof(PackSeg) + sizeof(PackTile) * (c / kPackTile + 2);
        if (!collects) b += sizeof(BatchEntry) * pack_seg_entries(c);
    }
    return b;
}

}  // namespace gpuhash
