// hostcheck.cpp -- TEST-ONLY CPU view of the planner (libgpuhash_hostcheck.so).
//
// Exposes the launch plan the HIP library would execute and replays, in plain C++,
// the data flow a scan kernel performs for ONE nonce from that launch's descriptor
// (uniform words, lane/loop digit insertion, precomputed S0/S1/CV midstates, extra
// padding block).  tests/test_plan.py compares it against the oracle on CPU so that a
// wrong host precomputation is caught without a GPU.  Not linked into libgpuhash.so
// and never used to produce a search result.
#include <algorithm>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

#include "collect.h"
#include "plan.h"
#include "stage.h"

using namespace gpuhash;

static int g_policy = kLayoutAuto;

// plan_range makes one Launch (about 700 bytes) per value of the leading digits H: a launch holds
// at most 10^(s + q) <= 10^10 nonces (plan.h, kMaxLaunchDigits; a lane table's rectangle at most
// 1024 * 10^8), so a whole 20-digit group is some 10^9 launches and the vector they are appended
// to (plan_range's `out`) ends in std::bad_alloc.  The engine never plans such a range in one
// piece (a search is cut into slices first); this library hands plans to ctypes, which an
// exception must not reach.  The bound is a deliberate over-estimate of the launches of
// [lower, upper] under any policy: it counts a launch per 10^min(d, 8) nonces of digit group d,
// the least any layout gives a launch, where most layouts give 10^9 or 10^10.  So it also refuses
// ranges whose plan would fit (2^48 nonces of the 15-digit group are about 28,000 launches, and
// refused); no test plans one, and a refusal is a return code, not a wrong plan.
constexpr uint64_t kMaxPlanLaunches = 1u << 18;
constexpr int kPlanTooLarge = -2;  // refused by the estimate, or std::bad_alloc all the same
constexpr int kPlanThrew = -3;     // any other exception: a fault of the planner, not of the range

static bool plan_too_large(uint64_t lower, uint64_t upper) {
    uint64_t est = 0;
    for (int d = num_digits(lower); d <= num_digits(upper); d++) {
        const uint64_t a = std::max(lower, d == 1 ? 0 : pow10u(d - 1));
        const uint64_t b = std::min(upper, d == 20 ? UINT64_MAX : pow10u(d) - 1);
        est += (b - a) / pow10u(std::min(d, 8)) + 32;
    }
    return est > kMaxPlanLaunches;
}

// f(), unless the plan is too large to hold; no exception leaves it.
template <class F>
static int guarded(uint64_t lower, uint64_t upper, F&& f) {
    if (plan_too_large(lower, upper)) return kPlanTooLarge;
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return kPlanTooLarge;
    } catch (...) {
        return kPlanThrew;
    }
}

extern "C" {

// Layout policy used by every plan_* / hostcheck_* call below (plan.h LayoutPolicy).
void hostcheck_set_layout_policy(int policy) { g_policy = policy; }

struct gpuhash_plan_info {
    int J, C2, EX, d, q, s;
    uint64_t lo, hi, base;
    uint32_t nblocks, R, rchunk, nrchunks, p_first, p_last, r_first, r_last;
    uint32_t stride, tail;  // tail-digit launches: nonces = tail (mod stride) in [lo, hi]
};

static std::vector<Launch> plan_of(const uint8_t* msg, uint64_t len, uint64_t lower, uint64_t upper,
                                   uint32_t rchunk, bool host_ptab = false) {
    std::vector<Launch> v;
    plan_range(msg, len, lower, upper, v, rchunk, g_policy, host_ptab);
    return v;
}

static gpuhash_plan_info plan_info(const Launch& l) {
    const LaunchDesc& D = l.desc;
    return gpuhash_plan_info{l.J, l.C2, l.EX, l.d, l.q, l.s, l.lo, l.hi, D.base, l.nblocks,
                             D.R, D.rchunk, D.nrchunks, D.p_first, D.p_last, D.r_first, D.r_last,
                             D.stride, D.tail};
}

int gpuhash_plan_count(const uint8_t* msg, uint64_t len, uint64_t lower, uint64_t upper, uint32_t rchunk) {
    if (lower > upper) return -1;
    return guarded(lower, upper, [&] { return (int)plan_of(msg, len, lower, upper, rchunk).size(); });
}

int gpuhash_plan_get(const uint8_t* msg, uint64_t len, uint64_t lower, uint64_t upper,
                     uint32_t rchunk, int idx, gpuhash_plan_info* out) {
    if (lower > upper || !out) return -1;
    return guarded(lower, upper, [&] {
        const std::vector<Launch> v = plan_of(msg, len, lower, upper, rchunk);
        if (idx < 0 || idx >= (int)v.size()) return -1;
        *out = plan_info(v[(size_t)idx]);
        return 0;
    });
}

// Whole plan in one call: fills up to cap entries, returns the launch count.
// gpuhash_plan_count, _get and _all return -2 for a range whose plan is too large to hold, -3
// should the planner throw anything but std::bad_alloc.
int gpuhash_plan_all(const uint8_t* msg, uint64_t len, uint64_t lower, uint64_t upper,
                     uint32_t rchunk, gpuhash_plan_info* out, int cap) {
    if (lower > upper) return -1;
    return guarded(lower, upper, [&] {
        const std::vector<Launch> v = plan_of(msg, len, lower, upper, rchunk);
        for (int i = 0; i < (int)v.size() && i < cap; i++) out[i] = plan_info(v[(size_t)i]);
        return (int)v.size();
    });
}

int gpuhash_shard(uint64_t msg_len, uint64_t lower, uint64_t upper, int n, uint64_t* lo,
                  uint64_t* hi, int* empty) {
    if (lower > upper || n < 1) return -1;
    std::vector<Shard> s = shard_range(msg_len, lower, upper, n, g_policy);
    for (int i = 0; i < n; i++) {
        lo[i] = s[(size_t)i].lo;
        hi[i] = s[(size_t)i].hi;
        empty[i] = s[(size_t)i].empty;
    }
    return 0;
}

// The cost model's price of the plan of [lower, upper] (plan_cost): what a shard of that
// range really costs under the layouts plan_range picks for it.
double gpuhash_plan_cost(const uint8_t* msg, uint64_t len, uint64_t lower, uint64_t upper) {
    if (lower > upper) return -1;
    double cost = 0;
    const int rc = guarded(lower, upper, [&] {
        cost = plan_cost(plan_of(msg, len, lower, upper, 0));
        return 0;
    });
    return rc ? (double)rc : cost;
}

}  // extern "C"

// The data flow of one nonce of launch l, given as the kernel holds it: the lane value p
// (C2 = 3: x) and the loop value r.
static uint64_t replay_hash(const Launch& l, uint32_t p, uint32_t r) {
    const LaunchDesc& D = l.desc;
    if (l.C2 == 3) {
        const uint32_t x = p;
        const uint32_t* P = &l.ptab[16ull * r];
        uint32_t W[64], st[8];
        std::memcpy(W, D.U, 64);
        W[0] |= ascii4(x / D.R1);
        W[1] |= (ascii4(x % D.R1) & D.qmask) << D.loop_shift;
        sha256_expand(W);
        std::memcpy(st, P, 32);
        // round 0 from the table's partial sums (as the kernel's ut_hash), then 1..63
        const uint32_t kw0 = kK[0] + W[0];
        uint32_t s1[8] = {P[8] + P[9] + kw0, st[0], st[1], st[2], st[3] + P[8] + kw0, st[4], st[5], st[6]};
        sha256_rounds(s1, W, 1, 64);
        return ((uint64_t)(P[0] + s1[0]) << 32) | (uint32_t)(P[1] + s1[1]);
    }
    const uint32_t alo = ascii4(p % 10000u), ahi = ascii4((p / 10000u) % 10000u);
    uint32_t W[64], st[8], cv[8];
    std::memcpy(W, D.U, 64);
    const int J = l.J;
    if (l.C2) {
        uint32_t V[64];
        std::memcpy(V, D.U1, 64);
        if (J == 0 || l.C2 == 2) { V[15] |= alo & D.mask_lo; V[14] |= ahi & D.mask_hi; }
        else { V[15] |= ahi & D.mask_hi; W[0] |= alo & D.mask_lo; }
        sha256_expand(V);
        std::memcpy(st, D.S1, 32);
        sha256_rounds(st, V, 14, 64);
        for (int i = 0; i < 8; i++) cv[i] = D.CV1[i] + st[i];
        std::memcpy(st, cv, 32);
        if (J == 1 && l.C2 == 1) sha256_rounds(st, W, 0, 1);  // W[1..] unused by round 0
    } else {
        std::memcpy(st, D.S0, 32);
        std::memcpy(cv, D.CV, 32);
        if (J >= 2) {
            W[J - 2] |= ahi & D.mask_hi;
            W[J - 1] |= alo & D.mask_lo;
            sha256_rounds(st, W, J - 2, J);
        } else if (J == 1) {
            W[0] |= alo & D.mask_lo;
            sha256_rounds(st, W, 0, 1);
        }
    }
    int t0 = J;
    if (l.C2 == 2) {  // two loop words: W_0 = 4 digits of r / R1, W_1 = digits of r % R1
        W[0] = D.U[0] | ascii4(r / D.R1);
        W[1] = D.U[1] | ((ascii4(r % D.R1) & D.qmask) << D.loop_shift);
        t0 = 0;
    } else {
        W[J] = D.U[J] | ((ascii4(r) & D.qmask) << D.loop_shift);
    }
    sha256_expand(W);
    sha256_rounds(st, W, t0, 64);
    uint32_t y[8];
    for (int i = 0; i < 8; i++) y[i] = cv[i] + st[i];
    if (l.EX) {
        uint32_t s2[8];
        std::memcpy(s2, y, 32);
        uint32_t kwx_minus_k[64];
        for (int t = 0; t < 64; t++) kwx_minus_k[t] = D.KWX[t] - kK[t];
        sha256_rounds(s2, kwx_minus_k, 0, 64);
        for (int i = 0; i < 8; i++) y[i] += s2[i];
    }
    return ((uint64_t)y[0] << 32) | y[1];
}

extern "C" {

// Replays the kernel's per-nonce computation from launch `idx`'s descriptor.  Returns 0, -1 for
// a bad range or index, -2 for a nonce outside the launch, -3 for one outside a lane table's
// rectangle, -4 for a range whose plan is too large to hold (as the plan entry points' -2) and
// -5 should the planner or the replay throw anything else: no exception leaves it.
static int desc_hash(const uint8_t* msg, uint64_t len, uint64_t lower, uint64_t upper,
                     uint32_t rchunk, int idx, uint64_t nonce, uint64_t* out) {
    const std::vector<Launch> v = plan_of(msg, len, lower, upper, rchunk, /*host_ptab=*/true);
    if (idx < 0 || idx >= (int)v.size()) return -1;
    const Launch& l = v[(size_t)idx];
    const LaunchDesc& D = l.desc;
    if (nonce < l.lo || nonce > l.hi) return -2;
    if (l.C2 == 3) {
        // lane table: x = lane value (W_0/W_1 digits), r = loop value (p-table entry)
        const uint64_t off = nonce - D.base;
        const uint32_t r = (uint32_t)(off / D.RQ), x = (uint32_t)(off % D.RQ);
        if (x < D.p_first || x > D.p_last || r >= D.R) return -3;  // not a rectangle
        *out = replay_hash(l, x, r);
        return 0;
    }
    // tail-digit launch: the kernel iterates k = nonce / stride; the tail digit is a
    // constant byte of D.U
    if (nonce % D.stride != D.tail) return -2;
    const uint64_t off = nonce / D.stride - D.base;
    *out = replay_hash(l, (uint32_t)(off / D.R), (uint32_t)(off % D.R));
    return 0;
}

int hostcheck_desc_hash(const uint8_t* msg, uint64_t len, uint64_t lower, uint64_t upper,
                        uint32_t rchunk, int idx, uint64_t nonce, uint64_t* out) {
    if (lower > upper || !out) return -1;
    if (plan_too_large(lower, upper)) return -4;
    try {
        return desc_hash(msg, len, lower, upper, rchunk, idx, nonce, out);
    } catch (const std::bad_alloc&) {
        return -4;
    } catch (...) {
        return -5;
    }
}

}  // extern "C"

// ---- first-hit search (gpuhash_first_below): CPU replay of the kernel's MODE 2 ----
//
// The same plan, variant groups, pieces, parts, masks, lower-bound function
// (part_min_nonce, plan.h) and skip rule as k_scan<.., 2>, with the per-descriptor replay
// above as the hash.  What a GPU decides by timing -- the order in which workgroups take
// the pieces, and which of them read the shared bound before another publishes -- is
// chosen here by a seed, so the tests can show the answer does not depend on it.

namespace {

// One part of a piece, as the kernel's inner loop cuts it: a row of one descriptor and the
// loop values [r0, r1).
struct Part {
    const Launch* l;      // for the hash replay
    const LaunchDesc* D;  // the descriptor as the kernel reads it, in the metadata buffer
    uint32_t row, r0, r1;
    uint64_t pos;   // position of (row, r0) in the group's row-iterations
    uint64_t dend;  // end of the part's descriptor there (offs[i + 1])
};

// One variant group as k_scan finds it in the metadata buffer, and the pieces it hands out.
struct VGroup {
    std::vector<const Launch*> ls;
    const unsigned long long* offs;  // ls.size() + 1 prefix offsets in row-iterations
    const LaunchDesc* descs;
    std::vector<std::pair<uint64_t, uint64_t>> pieces;  // [x, end)
};

// Resident workgroups assumed for the grab sizes (8 per CU on 256 CUs; the real figure
// comes from the occupancy query and only changes how the same work is cut).
constexpr unsigned int kReplayGrid = 2048;

// A device run as the engine stages it (stage.h): the buffer fill() wrote, which dev_run
// uploads, and the groups read back out of it.
struct Staged {
    Stage st;
    std::vector<uint8_t> meta;
    std::vector<VGroup> groups;

    Staged(const uint8_t* msg, uint64_t len, uint64_t lo, uint64_t hi, uint32_t rchunk, int policy)
        : st(msg, len, lo, hi, rchunk, policy, /*host_ptab=*/true), meta(st.bytes) {
        read_groups();
    }

    // A batch stage: plans[k] = job k's plan, with host p-tables.
    // packed: the jobs of it that run packed (stage.h, StageJobs::which), or null.
    Staged(std::vector<std::vector<Launch>>& plans, uint32_t rchunk,
           const std::vector<const BatchJob*>* packed = nullptr)
        : st(plans, rchunk, packed), meta(st.bytes) {
        read_groups();
    }

    // A first-hit batch stage: as above, with target[k] job k's target.
    Staged(std::vector<std::vector<Launch>>& plans, const uint64_t* target, uint32_t rchunk,
           const std::vector<const BatchJob*>* packed = nullptr)
        : st(plans, target, rchunk, packed), meta(st.bytes) {
        read_groups();
    }

    // A collect batch stage: as above, with lists[k] whether job k lists and the list's capacity.
    Staged(std::vector<std::vector<Launch>>& plans, const uint64_t* target, const uint8_t* lists,
           uint64_t buffer_entries, uint32_t rchunk, const std::vector<const BatchJob*>* packed = nullptr)
        : st(plans, target, lists, buffer_entries, rchunk, packed), meta(st.bytes) {
        read_groups();
    }

   private:
    void read_groups() {
        st.fill(meta.data());
        for (const StageGroup& sg : st.groups) {
            VGroup g;
            for (size_t k : sg.idx) g.ls.push_back(&st.plan[k]);
            g.offs = reinterpret_cast<const unsigned long long*>(meta.data() + sg.offs_at);
            g.descs = reinterpret_cast<const LaunchDesc*>(meta.data() + sg.desc_at);
            const uint64_t total = g.offs[g.ls.size()], grid = Stage::grid(sg, kReplayGrid);
            // guided self-scheduling: piece = clamp(remaining / (2 * grid), gmin, gmax)
            for (uint64_t cur = 0; cur < total;) {
                const uint64_t p = std::clamp<uint64_t>((total - cur) / (2 * grid), st.gmin, st.gmax);
                g.pieces.push_back({cur, std::min(cur + p, total)});
                cur += p;
            }
            groups.push_back(std::move(g));
        }
    }
};

void cut_parts(const VGroup& g, uint64_t x, uint64_t end, std::vector<Part>& out) {
    const int ndesc = (int)g.ls.size();
    while (x < end) {
        int i = 0;
        while (i + 1 < ndesc && g.offs[i + 1] <= x) i++;
        const LaunchDesc& D = g.descs[i];
        const uint32_t rel = (uint32_t)(x - g.offs[i]);
        const uint32_t row = rel / D.R, r0 = rel - row * D.R;
        const uint64_t left = end - x;
        const uint32_t r1 = (uint64_t)(D.R - r0) < left ? D.R : r0 + (uint32_t)left;
        out.push_back(Part{g.ls[(size_t)i], &D, row, r0, r1, x, g.offs[i + 1]});
        x += r1 - r0;
    }
}

// Calls f(lane value, loop value, nonce) for every nonce the kernel's masks admit in a
// part: lanes up to p_last, and r within [r_first, r_last] on the launch's first / last
// lane value (scan_row's lane_ok, rlo, rhi; scan_row_lt has only lane_ok).
template <class F>
void for_each_nonce(const Part& pt, F&& f) {
    const LaunchDesc& D = *pt.D;
    for (uint32_t t = 0; t < (uint32_t)kBlock; t++) {
        const uint64_t p64 = (uint64_t)D.p_first + (uint64_t)pt.row * 256u + t;
        if (p64 > D.p_last) break;
        const uint32_t p = (uint32_t)p64;
        if (pt.l->C2 == 3) {
            for (uint32_t r = pt.r0; r < pt.r1; r++) f(p, r, D.base + (uint64_t)r * D.RQ + p);
            continue;
        }
        const uint32_t rlo = p == D.p_first ? D.r_first : 0u;
        const uint32_t rhi = p == D.p_last ? D.r_last : D.R - 1u;
        for (uint32_t r = std::max(pt.r0, rlo); r < pt.r1 && r <= rhi; r++)
            f(p, r, (D.base + (uint64_t)p * D.R + r) * D.stride + D.tail);
    }
}

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
};

// The order a group's pieces are taken in: order_seed 0 ascending, 1 descending, else shuffled.
std::vector<size_t> piece_order(const VGroup& g, uint64_t order_seed, Rng& rng) {
    std::vector<size_t> order(g.pieces.size());
    std::iota(order.begin(), order.end(), (size_t)0);
    if (order_seed == 1) std::reverse(order.begin(), order.end());
    else if (order_seed != 0)
        for (size_t i = order.size(); i > 1; i--) std::swap(order[i - 1], order[rng.next() % i]);
    return order;
}

// One run of the sub-range `sub` in collecting mode (the kernel's MODE 3): its groups back to back
// on one counter and one list of `room` entries (0: count only); appends past the list's end are
// counted and dropped.
void collect_run(const uint8_t* msg, uint64_t len, const SubRange& sub, uint32_t rchunk, uint64_t target,
                 int policy, uint64_t order_seed, Rng& rng, uint64_t room, SubResult& out) {
    const Staged staged(msg, len, sub.lo, sub.hi, rchunk, policy);
    for (const VGroup& g : staged.groups) {
        std::vector<Part> parts;
        for (size_t k : piece_order(g, order_seed, rng)) {
            parts.clear();
            cut_parts(g, g.pieces[k].first, g.pieces[k].second, parts);
            for (const Part& pt : parts)
                for_each_nonce(pt, [&](uint32_t p, uint32_t r, uint64_t n) {
                    const uint64_t h = replay_hash(*pt.l, p, r);
                    if (h > target) return;
                    const uint64_t slot = out.count++;  // the atomic add
                    if (slot < room) out.hits.push_back(Hit{h, n});
                });
        }
    }
}

}  // namespace

extern "C" {

// The stage of a device run over [lower, upper] (stage.h), as dev_run builds it.  Per variant
// group, in launch order and up to cap groups, 14 words of out: J, C2, EX, descriptors, the d
// and c of its largest launch (as gpuhash_launch_record has them), row-iterations, nonces, the
// byte positions in the metadata buffer of its counters, prefix offsets, descriptors and p-table
// room, and the sizes of the last two.  *bytes is the buffer's size, and meta[0, *bytes) the
// buffer as fill() writes it, if meta_cap allows.  Returns the group count.
int hostcheck_stage(const uint8_t* msg, uint64_t len, uint64_t lower, uint64_t upper, uint32_t rchunk,
                    uint64_t* out, int cap, uint64_t* bytes, uint8_t* meta, uint64_t meta_cap) {
    if (lower > upper || !bytes) return -1;
    const Stage st(msg, len, lower, upper, rchunk, g_policy);
    for (int i = 0; i < (int)st.groups.size() && i < cap; i++) {
        const StageGroup& g = st.groups[(size_t)i];
        const uint64_t row[14] = {(uint64_t)g.J, (uint64_t)g.C2, (uint64_t)g.EX, g.idx.size(), (uint64_t)g.d,
                                  (uint64_t)g.c, g.total, g.nonces, g.work_at, g.offs_at, g.desc_at, g.ptab_at,
                                  sizeof(LaunchDesc) * g.idx.size(), g.ptab_bytes};
        std::memcpy(out + 14 * i, row, sizeof row);
    }
    *bytes = st.bytes;
    if (meta && meta_cap >= st.bytes) st.fill(meta);
    return (int)st.groups.size();
}

// The first-hit search of [lower, upper] as the kernels run it.  order_seed picks the order
// in which each variant group's pieces are taken: 0 ascending, 1 strictly descending, any
// other value a shuffle in which random batches of 1-8 pieces are "in flight" together,
// i.e. all read the shared bound before any of them publishes a hit.  Returns 0 and
// *found, (*hash, *nonce) (untouched when nothing qualifies), and in *pieces_skipped the
// pieces whose every part the skip rule dropped unhashed.
// The kernel's second step -- a skipped part of a descriptor other than a lane table's takes
// the rest of that descriptor off the work counter (atomicMax) -- is replayed as a list of
// cancelled position ranges.  On the GPU it only touches pieces not yet handed out, which
// all lie further on; here it drops those positions from every piece visited later, in
// whatever order, which skips more than the kernel can and so checks the rule harder.
int hostcheck_first_below(const uint8_t* msg, uint64_t len, uint64_t lower, uint64_t upper,
                          uint32_t rchunk, uint64_t target, uint64_t order_seed, uint64_t* hash,
                          uint64_t* nonce, int* found, uint64_t* pieces_skipped) {
    if (lower > upper || !hash || !nonce || !found || !pieces_skipped) return -1;
    const Staged run(msg, len, lower, upper, rchunk, g_policy);
    uint64_t bound = ~0ull;  // the word `thresh` points to
    bool any = false;
    uint64_t best_n = 0, best_h = 0, skipped = 0;
    Rng rng{order_seed};
    for (const VGroup& g : run.groups) {  // the groups run back to back on one stream
        std::vector<std::pair<uint64_t, uint64_t>> cancelled;  // [from, to) positions
        auto is_cancelled = [&](uint64_t pos) {
            for (const auto& c : cancelled)
                if (pos >= c.first && pos < c.second) return true;
            return false;
        };
        const std::vector<size_t> order = piece_order(g, order_seed, rng);
        for (size_t at = 0; at < order.size();) {
            const size_t batch = order_seed <= 1 ? 1 : std::min<size_t>(1 + rng.next() % 8, order.size() - at);
            const uint64_t seen = bound;  // read once per grab, before the batch publishes
            uint64_t publish = ~0ull;
            bool hit = false;
            for (size_t k = at; k < at + batch; k++) {
                std::vector<Part> parts;
                cut_parts(g, g.pieces[order[k]].first, g.pieces[order[k]].second, parts);
                bool all_skipped = true;
                for (const Part& pt : parts) {
                    if (is_cancelled(pt.pos)) continue;
                    if (part_min_nonce(*pt.D, pt.l->C2, pt.row, pt.r0) > seen) {
                        if (pt.l->C2 != 3) cancelled.push_back({pt.pos, pt.dend});
                        continue;
                    }
                    all_skipped = false;
                    for_each_nonce(pt, [&](uint32_t p, uint32_t r, uint64_t n) {
                        const uint64_t h = replay_hash(*pt.l, p, r);
                        if (h > target) return;
                        if (!any || n < best_n) { best_n = n; best_h = h; any = true; }
                        if (!hit || n < publish) { publish = n; hit = true; }
                    });
                }
                skipped += all_skipped ? 1 : 0;
            }
            if (hit && publish < bound) bound = publish;  // atomicMin
            at += batch;
        }
    }
    *found = any ? 1 : 0;
    *pieces_skipped = skipped;
    if (any) { *hash = best_h; *nonce = best_n; }
    return 0;
}

// gpuhash_collect_below as the engine runs it: the same collector (collect.h) over the same
// slices and shards, with each sub-range run replayed in plain C++ from its plan's
// descriptors, rows, pieces and masks, as hostcheck_first_below replays MODE 2.  What a GPU
// decides by timing is the order of the appends to the device list, and so which hits a
// full list drops: order_seed picks the order in which each variant group's pieces are taken
// (0 ascending, 1 descending, else a shuffle), and within a piece hits are appended lane by
// lane, which is not ascending either.  The list holds buffer_entries entries (when a list is
// asked for) and appends past its end are counted and dropped, as in the kernel.  `policy` is
// the layout policy of this call.  slice_nonces (0: the engine's, stage.h) is the slice per shard
// and nshards the number of context entries.  Returns 0 and *out_total, the lowest
// min(cap, total) hits in out_nonces / out_hashes (untouched beyond), and in *out_runs how
// many sub-range runs the collector asked for, re-runs included.
int hostcheck_collect_below(const uint8_t* msg, uint64_t len, uint64_t lower, uint64_t upper,
                            uint32_t rchunk, uint64_t target, int policy, uint64_t order_seed,
                            uint64_t buffer_entries, uint64_t cap, uint64_t slice_nonces, int nshards,
                            uint64_t* out_nonces, uint64_t* out_hashes, uint64_t* out_total,
                            uint64_t* out_runs) {
    if (lower > upper || !out_total || !out_runs || nshards < 1 || (cap && (!out_nonces || !out_hashes)))
        return -1;
    uint64_t runs = 0;
    Rng rng{order_seed};
    const uint64_t B = std::max<uint64_t>(buffer_entries, 1);
    auto run_one = [&](const SubRange& sub, bool want_list, SubResult& out) {
        runs++;
        // the word the kernel reads its capacity from
        collect_run(msg, len, sub, rchunk, target, policy, order_seed, rng, want_list ? B : 0, out);
    };
    auto run = [&](const std::vector<SubRange>& batch, bool want_list, std::vector<SubResult>& res) {
        for (size_t i = 0; i < batch.size(); i++) run_one(batch[i], want_list, res[i]);
        return 0;
    };
    auto split = [&](uint64_t lo, uint64_t hi, std::vector<SubRange>& batch) {
        split_slice(len, lo, hi, nshards, policy, batch);
    };
    Collector<decltype(run), decltype(split)> c(B, (size_t)cap, run, split);
    if (int rc = c.collect(lower, upper, slice_width((uint64_t)nshards, slice_nonces))) return rc;
    for (size_t i = 0; i < c.held.size(); i++) {
        out_nonces[i] = c.held[i].nonce;
        out_hashes[i] = c.held[i].hash;
    }
    *out_total = c.total;
    *out_runs = runs;
    return 0;
}

// Every part of every piece of the plan of [lower, upper], for checking the lower-bound
// function directly: bound[i] = part_min_nonce of part i, least[i] = the smallest nonce the
// kernel's masks admit in it, count[i] = how many they admit (0: least[i] is unset).
// Fills up to cap entries; returns the number of parts.
int hostcheck_parts(const uint8_t* msg, uint64_t len, uint64_t lower, uint64_t upper, uint32_t rchunk,
                    uint64_t* bound, uint64_t* least, uint64_t* count, int cap) {
    if (lower > upper) return -1;
    const Staged run(msg, len, lower, upper, rchunk, g_policy);
    int n = 0;
    for (const VGroup& g : run.groups) {
        for (const auto& pc : g.pieces) {
            std::vector<Part> parts;
            cut_parts(g, pc.first, pc.second, parts);
            for (const Part& pt : parts) {
                if (n < cap) {
                    uint64_t lo = 0, c = 0;
                    for_each_nonce(pt, [&](uint32_t, uint32_t, uint64_t x) {
                        if (!c || x < lo) lo = x;
                        c++;
                    });
                    bound[n] = part_min_nonce(*pt.D, pt.l->C2, pt.row, pt.r0);
                    least[n] = lo;
                    count[n] = c;
                }
                n++;
            }
        }
    }
    return n;
}

}  // extern "C"

// ---- batch search (gpuhash_min_batch): CPU replay of the kernel's MODE 4 ----
//
// A batch stage's groups, pieces, parts and masks as k_scan<.., 4> walks them, from the bytes
// fill() wrote: the descriptor lookup that resumes from the previous part (batch_find), the
// job-change flush, the per-job pruning words and the result list with its bound.  A workgroup
// is replayed with its four waves' running bests.  What a GPU decides by timing -- which
// workgroup takes which piece, and what a workgroup reads in a pruning word before another has
// flushed -- is chosen by a seed, within what the work counter allows: a workgroup's pieces are
// ascending, since every grab returns a higher position than the one before.

namespace {

struct ReplayWave {
    uint64_t h = ~0ull, n = ~0ull;
    uint32_t T = 0xFFFFFFFFu;
};

struct ReplayWg {
    std::vector<size_t> pieces;  // ascending
    size_t next = 0;
    ReplayWave w[4];
    uint32_t job = 0xFFFFFFFFu;  // kNoJob
    int idx = 0;                 // batch_find's hint
};

// One run of a batch on one context entry; appends to nothing outside it.
struct BatchReplay {
    const Staged& run;
    std::vector<uint64_t> thresh;
    std::vector<BatchEntry> list;
    Rng* jitter = nullptr;

    explicit BatchReplay(const Staged& r) : run(r), thresh(r.st.njobs) {
        std::memcpy(thresh.data(), r.meta.data() + r.st.thresh_at, 8 * r.st.njobs);  // as fill() armed them
    }

    void flush(ReplayWg& wg) {
        uint64_t bh = wg.w[0].h, bn = wg.w[0].n;
        for (int i = 1; i < 4; i++)
            if (wg.w[i].h < bh || (wg.w[i].h == bh && wg.w[i].n < bn)) { bh = wg.w[i].h; bn = wg.w[i].n; }
        if (bh != ~0ull || bn != ~0ull) {
            thresh[wg.job] = std::min(thresh[wg.job], bh);
            list.push_back(BatchEntry{bh, bn, wg.job, 0});
        }
    }

    // The kernel's batch_find: the largest i with offs[i] <= x, from a hint that is any index.
    static int find(const VGroup& g, int i, uint64_t x) {
        const int ndesc = (int)g.ls.size();
        int lo = 0, hi = ndesc - 1;
        if (g.offs[i] > x) {
            hi = i - 1;
        } else if (i + 1 < ndesc && g.offs[i + 1] <= x) {
            i++;
            if (i + 1 < ndesc && g.offs[i + 1] <= x) lo = i + 1;
            else lo = hi = i;
        } else {
            return i;
        }
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (g.offs[mid] <= x) lo = mid;
            else hi = mid - 1;
        }
        return lo;
    }

    void piece(const VGroup& g, ReplayWg& wg, uint64_t x, uint64_t end) {
        if (wg.job != 0xFFFFFFFFu)  // the grab: tighten T from the current job's word
            for (ReplayWave& w : wg.w) w.T = std::min(w.T, (uint32_t)(thresh[wg.job] >> 32));
        while (x < end) {
            // the hint is whatever descriptor some wave of the workgroup found last: under a
            // shuffle, now and then any index at all
            if (jitter && jitter->next() % 4 == 0) wg.idx = (int)(jitter->next() % g.ls.size());
            const int i = wg.idx = find(g, wg.idx, x);
            const LaunchDesc& D = g.descs[i];
            const uint32_t rel = (uint32_t)(x - g.offs[i]);
            const uint32_t row = rel / D.R, r0 = rel - row * D.R;
            const uint64_t left = end - x;
            const uint32_t r1 = (uint64_t)(D.R - r0) < left ? D.R : r0 + (uint32_t)left;
            if (D.job != wg.job) {
                if (wg.job != 0xFFFFFFFFu) flush(wg);
                wg.job = D.job;
                for (ReplayWave& w : wg.w) w = ReplayWave{~0ull, ~0ull, (uint32_t)(thresh[D.job] >> 32)};
            }
            const Part pt{g.ls[(size_t)i], &D, row, r0, r1, x, g.offs[i + 1]};
            for_each_nonce(pt, [&](uint32_t p, uint32_t r, uint64_t n) {
                ReplayWave& w = wg.w[((p - D.p_first) & 255u) >> 6];
                const uint64_t h = replay_hash(*pt.l, p, r);
                const uint32_t h0 = (uint32_t)(h >> 32);
                if (h0 > w.T) return;  // the prune: H0 <= wb.T takes the slow path
                if (h < w.h || (h == w.h && n < w.n)) {
                    w.h = h;
                    w.n = n;
                    w.T = std::min(w.T, h0);
                }
            });
            x += r1 - r0;
        }
    }

    void group(size_t gi, uint64_t order_seed, Rng& rng) {
        const VGroup& g = run.groups[gi];
        const size_t np = g.pieces.size();
        jitter = order_seed > 1 ? &rng : nullptr;
        const size_t grid = Stage::grid(run.st.groups[gi], std::min<unsigned int>(kReplayGrid, kBatchMaxGrid));
        // seed 0: one workgroup takes every piece, ascending.  seed 1: as many workgroups as the
        // grid allows take contiguous shares and run one after the other, the LAST share first
        // (strictly descending pieces when there is a workgroup per piece).  Else 2-8 workgroups
        // in flight, each piece dealt to a random one, and the next piece to run picked at
        // random among the workgroups' next ones.
        const size_t W = order_seed == 0 ? 1 : order_seed == 1 ? std::min(grid, np)
                                                               : std::min({grid, np, (size_t)(2 + rng.next() % 7)});
        std::vector<ReplayWg> wgs(W);
        for (size_t k = 0; k < np; k++) {
            const size_t w = order_seed == 0 ? 0 : order_seed == 1 ? k * W / np : rng.next() % W;
            wgs[w].pieces.push_back(k);
        }
        auto step = [&](ReplayWg& wg) {
            const auto& pc = g.pieces[wg.pieces[wg.next++]];
            piece(g, wg, pc.first, pc.second);
            if (wg.next == wg.pieces.size() && wg.job != 0xFFFFFFFFu) flush(wg);  // the end of the kernel
        };
        if (order_seed <= 1) {
            for (size_t w = W; w-- > 0;)
                while (wgs[w].next < wgs[w].pieces.size()) step(wgs[w]);
            return;
        }
        std::vector<size_t> live;
        for (size_t w = 0; w < W; w++)
            if (!wgs[w].pieces.empty()) live.push_back(w);
        while (!live.empty()) {
            const size_t at = rng.next() % live.size();
            ReplayWg& wg = wgs[live[at]];
            step(wg);
            if (wg.next == wg.pieces.size()) live.erase(live.begin() + (long)at);
        }
    }
};

// ---- the packed group of a batch stage (pack.h): CPU replay of k_pack ----
//
// The group's tiles, segments and records from the bytes fill() wrote, and per lane pack.h's own
// segment search, block building and compression -- never hash_host: the byte placement is what
// the replay is for.  A wave's lanes are cut into runs of one job, as the kernel's ballot cuts
// them, and a wave runs in two steps: it hashes and READS (the min mode's plain read of
// thresh[job]), then does its atomics and stores.  Under a shuffle 2-8 workgroups are in flight,
// each with ascending tiles and its waves in a random order, and the next step is any workgroup's:
// other waves' atomics land between a wave's read and its own, and half the reads return the
// stalest value there is, the word as armed.

struct PackLane {
    uint64_t h, n;
};

struct PackRun {
    uint32_t job;
    std::vector<PackLane> lanes;
    uint64_t seen = ~0ull;
};

struct PackReplay {
    const PackJob* recs;
    const PackSeg* segs;
    const PackTile* tiles;
    uint64_t total;

    explicit PackReplay(const Staged& r)
        : recs(reinterpret_cast<const PackJob*>(r.meta.data() + r.st.pack_recs_at)),
          segs(reinterpret_cast<const PackSeg*>(r.meta.data() + r.st.pack_segs_at)),
          tiles(reinterpret_cast<const PackTile*>(r.meta.data() + r.st.pack_tiles_at)),
          total(r.st.pack.tiles.size()) {}

    std::vector<PackRun> wave(uint64_t x, uint32_t wv) const {
        const PackTile& T = tiles[x];
        std::vector<PackRun> runs;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t item = T.item0 + 64 * wv + lane;
            const PackSeg& S = segs[pack_find_seg(segs, T.seg_first, T.seg_last, item)];
            const uint64_t idx = item - S.start;
            if (idx >= S.count) continue;  // idle: past the class's end
            const PackJob& rec = recs[S.rec];
            uint32_t H0, H1;
            pack_hash(rec, T.o, T.d, S.n0 + idx, H0, H1);
            if (runs.empty() || runs.back().job != rec.job) runs.push_back(PackRun{rec.job, {}});
            runs.back().lanes.push_back(PackLane{(uint64_t)H0 << 32 | H1, S.n0 + idx});
        }
        return runs;
    }

    // order_seed 0: tiles and waves ascending; 1: descending; else the shuffle above.
    template <class Read, class Commit>
    void group(uint64_t order_seed, Rng& rng, Read&& read, Commit&& commit) const {
        auto whole = [&](uint64_t x, uint32_t wv) {
            std::vector<PackRun> runs = wave(x, wv);
            for (PackRun& r : runs) read(r, false);
            for (PackRun& r : runs) commit(r);
        };
        if (order_seed <= 1) {
            for (uint64_t i = 0; i < total; i++)
                for (uint32_t v = 0; v < 4; v++) order_seed ? whole(total - 1 - i, 3 - v) : whole(i, v);
            return;
        }
        struct Wg {
            std::vector<uint64_t> tiles;
            size_t next = 0;
            uint32_t done = 0, order[4] = {0, 1, 2, 3};
            bool pending = false;
            std::vector<PackRun> runs;
        };
        std::vector<Wg> wgs(2 + rng.next() % 7);
        for (uint64_t x = 0; x < total; x++) wgs[rng.next() % wgs.size()].tiles.push_back(x);
        std::vector<size_t> live;
        for (size_t w = 0; w < wgs.size(); w++)
            if (!wgs[w].tiles.empty()) live.push_back(w);
        while (!live.empty()) {
            const size_t at = rng.next() % live.size();
            Wg& wg = wgs[live[at]];
            if (!wg.pending) {
                if (!wg.done)
                    for (size_t i = 4; i > 1; i--) std::swap(wg.order[i - 1], wg.order[rng.next() % i]);
                wg.runs = wave(wg.tiles[wg.next], wg.order[wg.done]);
                for (PackRun& r : wg.runs) read(r, rng.next() % 2 == 0);
                wg.pending = true;
                continue;
            }
            for (PackRun& r : wg.runs) commit(r);
            wg.pending = false;
            if (++wg.done == 4) { wg.done = 0; wg.next++; }
            if (wg.next == wg.tiles.size()) live.erase(live.begin() + (long)at);
        }
    }
};

// The min mode over the stage's pruning words and list, which `rep` holds for the unpacked groups
// too.  The store is bounded by the capacity in the list's head; returns the appends it left out.
uint64_t pack_min_group(const Staged& staged, BatchReplay& rep, uint64_t order_seed, Rng& rng) {
    const PackReplay pk(staged);
    uint32_t head[4];
    std::memcpy(head, staged.meta.data() + staged.st.list_at, sizeof head);
    const uint64_t cap = head[1];
    uint64_t dropped = 0;
    pk.group(order_seed, rng,
             [&](PackRun& r, bool stale) {
                 // the segmented minimum: the run's best by (hash, nonce) in its first lane
                 PackLane b = r.lanes[0];
                 for (const PackLane& l : r.lanes)
                     if (l.h < b.h || (l.h == b.h && l.n < b.n)) b = l;
                 r.lanes.assign(1, b);
                 r.seen = stale ? ~0ull : rep.thresh[r.job];
             },
             [&](PackRun& r) {
                 const PackLane& b = r.lanes[0];
                 if (b.h > r.seen) return;
                 const uint64_t old = rep.thresh[r.job];  // the atomicMin
                 rep.thresh[r.job] = std::min(old, b.h);
                 if (b.h > old) return;
                 if (rep.list.size() + dropped < cap) rep.list.push_back(BatchEntry{b.h, b.n, r.job, 0});
                 else dropped++;
             });
    return dropped;
}

}  // namespace

extern "C" {

// gpuhash_min_batch as the engine runs it: the same sub-batches (for_each_sub_batch under
// batch_bytes, 0: the engine's bound), runs over nshards context entries (batch_runs) and batch
// stages, each run replayed as above with the order of its pieces chosen by order_seed (0, 1 or
// a shuffle, see BatchReplay::group).  Under a policy with GPUHASH_LAYOUT_PACKED_ALWAYS the jobs
// that pack are staged and replayed as the packed group (PackReplay), whose appends count towards
// the fill whether the bounded store kept them or not.  msg_off has njobs + 1 entries.  Returns 0 and the per-job
// results, and in out_fill[0..3]: the largest result-list fill of any run, that run's bound
// (Stage::list_cap), how many runs filled their list past its bound (0, or the bound is wrong),
// and the number of sub-batches.
int hostcheck_min_batch(const uint8_t* msgs, const uint64_t* msg_off, uint64_t njobs, const uint64_t* lower,
                        const uint64_t* upper, uint32_t rchunk, int policy, uint64_t order_seed,
                        uint64_t batch_bytes, int nshards, uint64_t* out_hashes, uint64_t* out_nonces,
                        uint64_t* out_fill) {
    if (!msg_off || !lower || !upper || !out_hashes || !out_nonces || !out_fill || !njobs || nshards < 1) return -1;
    for (uint64_t k = 0; k < njobs; k++)
        if (lower[k] > upper[k] || msg_off[k + 1] < msg_off[k]) return -1;
    Rng rng{order_seed};
    uint64_t fill[4] = {0, 0, 0, 0};
    auto plan = [&](size_t k) {
        const uint64_t len = msg_off[k + 1] - msg_off[k];
        const BatchJob j{len ? msgs + msg_off[k] : nullptr, len, lower[k], upper[k]};
        if (packs(policy, j.lo, j.hi)) return plan_packed_job(j);
        return plan_job(j, rchunk, policy, /*host_ptab=*/true);
    };
    auto run = [&](size_t first, std::vector<PlannedJob>& jobs) {
        fill[3]++;
        for (const auto& r : batch_runs(jobs, (size_t)nshards)) {
            StageJobs sj(jobs, r.first, r.second);
            const Staged staged(sj.plans, rchunk, sj.which());
            BatchReplay rep(staged);
            uint64_t dropped = 0;  // what the packed group's bounded store left out
            for (size_t gi = 0; gi < staged.groups.size(); gi++) {
                if (staged.st.groups[gi].C2 == 4) dropped += pack_min_group(staged, rep, order_seed, rng);
                else rep.group(gi, order_seed, rng);
            }
            const uint64_t filled = rep.list.size() + dropped;
            if (filled >= fill[0]) { fill[0] = filled; fill[1] = staged.st.list_cap; }
            fill[2] += filled > staged.st.list_cap ? 1 : 0;
            for (size_t k = r.first; k < r.second; k++) out_hashes[first + k] = out_nonces[first + k] = ~0ull;
            for (const BatchEntry& e : rep.list) {  // the host's fold
                uint64_t &h = out_hashes[first + r.first + e.job], &n = out_nonces[first + r.first + e.job];
                if (e.hash < h || (e.hash == h && e.nonce < n)) { h = e.hash; n = e.nonce; }
            }
        }
        return 0;
    };
    if (int rc = for_each_sub_batch((size_t)njobs, batch_bytes_bound(batch_bytes), plan, run)) return rc;
    std::memcpy(out_fill, fill, sizeof fill);
    return 0;
}

// The stage of ONE run of a batch (all njobs jobs on one context entry, no sub-batch cut) under
// hostcheck_set_layout_policy's policy (with GPUHASH_LAYOUT_PACKED_ALWAYS: the packed group last), as hostcheck_stage gives a single search's: the same 14
// words per variant group, *bytes and meta, and in extra[0..7] the bytes the host uploads, the
// byte position and size of the per-job pruning words, the byte position of the result list
// (its 16-byte head first) and its capacity in entries, the size of an entry, and the number
// of K+W tables and their words in all.
int hostcheck_stage_batch(const uint8_t* msgs, const uint64_t* msg_off, uint64_t njobs, const uint64_t* lower,
                          const uint64_t* upper, uint32_t rchunk, uint64_t* out, int cap, uint64_t* bytes,
                          uint64_t* extra, uint8_t* meta, uint64_t meta_cap) {
    if (!msg_off || !lower || !upper || !bytes || !extra || !njobs) return -1;
    std::vector<std::vector<Launch>> plans(njobs);
    std::vector<BatchJob> jobs(njobs);  // under GPUHASH_LAYOUT_PACKED_ALWAYS: the jobs that run packed
    std::vector<const BatchJob*> packed(njobs, nullptr);
    bool any = false;
    for (uint64_t k = 0; k < njobs; k++) {
        if (lower[k] > upper[k] || msg_off[k + 1] < msg_off[k]) return -1;
        const uint64_t len = msg_off[k + 1] - msg_off[k];
        jobs[k] = BatchJob{len ? msgs + msg_off[k] : nullptr, len, lower[k], upper[k]};
        if (packs(g_policy, lower[k], upper[k])) packed[k] = &jobs[k], any = true;
        else plan_range(jobs[k].msg, len, lower[k], upper[k], plans[k], rchunk, g_policy);
    }
    const Stage st(plans, rchunk, any ? &packed : nullptr);
    for (int i = 0; i < (int)st.groups.size() && i < cap; i++) {
        const StageGroup& g = st.groups[(size_t)i];
        const uint64_t row[14] = {(uint64_t)g.J, (uint64_t)g.C2, (uint64_t)g.EX, g.idx.size(), (uint64_t)g.d,
                                  (uint64_t)g.c, g.total, g.nonces, g.work_at, g.offs_at, g.desc_at, g.ptab_at,
                                  sizeof(LaunchDesc) * g.idx.size(), g.ptab_bytes};
        std::memcpy(out + 14 * i, row, sizeof row);
    }
    *bytes = st.bytes;
    const uint64_t ex[8] = {st.upload_bytes, st.thresh_at, 8 * st.njobs, st.list_at, st.list_cap,
                            sizeof(BatchEntry), st.tabs.size(), st.tab_words};
    std::memcpy(extra, ex, sizeof ex);
    if (meta && meta_cap >= st.bytes) {
        std::memset(meta, 0, st.bytes);
        st.fill(meta);
    }
    return (int)st.groups.size();
}

}  // extern "C"

// ---- first-hit batch (gpuhash_first_below_batch): CPU replay of the kernel's MODE 5 ----
//
// A first-hit batch stage's groups in stage order (ascending digits), pieces, parts and masks as
// k_scan<.., 5> walks them, from the bytes fill() wrote: MODE 4's descriptor lookup and job change,
// MODE 2's slow path, skip rule and drain against the current job's words.  A workgroup is replayed
// with its four waves' hits; its pieces ascend.  What a GPU decides by timing is chosen by a seed:
// which workgroup takes which piece, and -- under a shuffle -- what a workgroup reads in a bound
// word: now and then not the word as it stands but as it stood when the group's launch began, the
// stalest value a read in that launch can return (the launches run back to back on one stream, so
// whatever earlier launches published is there).
// The drain (atomicMax on the work counter) is replayed as in hostcheck_first_below: as cancelled
// position ranges that drop those positions from every piece visited later, in whatever order,
// which skips more than the kernel can.

namespace {

struct FirstWg {
    std::vector<size_t> pieces;  // ascending
    size_t next = 0;
    uint64_t n[4] = {0, 0, 0, 0}, h[4] = {0, 0, 0, 0};
    bool found[4] = {false, false, false, false};
    uint32_t job = 0xFFFFFFFFu;  // kNoJob
    uint64_t bound = ~0ull;      // as read at the last grab or job change
    int idx = 0;                 // batch_find's hint
};

// What the replay did for one job.
struct JobTrace {
    uint64_t lo = 0, hashed = 0, largest = 0;
    std::vector<bool> seen;  // per nonce of the job's range, while it is small enough to hold
    bool twice = false;      // some nonce was hashed twice: the pieces overlapped
};

struct FirstBatchReplay {
    const Staged& run;
    std::vector<uint64_t> words;  // {bound, target} per job, as fill() armed them
    std::vector<uint64_t> at_launch;  // the bounds when the current group's launch began
    std::vector<BatchEntry> list;
    std::vector<JobTrace>& trace;
    std::vector<std::pair<uint64_t, uint64_t>> cancelled;  // of the current group, [from, to)
    Rng* jitter = nullptr;

    FirstBatchReplay(const Staged& r, std::vector<JobTrace>& t) : run(r), words(2 * r.st.njobs), trace(t) {
        std::memcpy(words.data(), r.meta.data() + r.st.thresh_at, 16 * r.st.njobs);
    }

    uint64_t read_bound(uint32_t job) {
        if (jitter && jitter->next() % 4 == 0) return at_launch[job];
        return words[2 * (size_t)job];
    }

    void flush(FirstWg& wg) {
        if (wg.job == 0xFFFFFFFFu) return;
        bool any = false;
        uint64_t bn = 0, bh = 0;
        for (int i = 0; i < 4; i++)
            if (wg.found[i] && (!any || wg.n[i] < bn)) { bn = wg.n[i]; bh = wg.h[i]; any = true; }
        if (any) list.push_back(BatchEntry{bh, bn, wg.job, 0});
    }

    bool is_cancelled(uint64_t pos, uint64_t& to) const {
        for (const auto& c : cancelled)
            if (pos >= c.first && pos < c.second) { to = c.second; return true; }
        return false;
    }

    void piece(const VGroup& g, FirstWg& wg, uint64_t x, uint64_t end) {
        if (wg.job != 0xFFFFFFFFu) wg.bound = read_bound(wg.job);  // the grab
        while (x < end) {
            uint64_t to;
            if (is_cancelled(x, to)) {  // never handed out
                x = std::min(to, end);
                continue;
            }
            if (jitter && jitter->next() % 4 == 0) wg.idx = (int)(jitter->next() % g.ls.size());
            const int i = wg.idx = BatchReplay::find(g, wg.idx, x);
            const LaunchDesc& D = g.descs[i];
            const Launch& l = *g.ls[(size_t)i];
            const uint32_t rel = (uint32_t)(x - g.offs[i]);
            const uint32_t row = rel / D.R, r0 = rel - row * D.R;
            const uint64_t left = end - x;
            const uint32_t r1 = (uint64_t)(D.R - r0) < left ? D.R : r0 + (uint32_t)left;
            if (D.job != wg.job) {
                flush(wg);
                wg.job = D.job;
                for (bool& f : wg.found) f = false;
                wg.bound = read_bound(D.job);
            }
            const uint64_t target = words[2 * (size_t)D.job + 1];
            const uint64_t lb = std::max(part_min_nonce(D, l.C2, row, r0), desc_min_nonce(D, l.C2));
            if (lb > wg.bound) {
                if (l.C2 != 3) {
                    // the drain, with the kernel's look at the next 64 descriptors: the unbroken
                    // run of those that lie wholly above their own job's bound goes with it
                    int k = i + 1;
                    while (k < (int)g.ls.size() && k <= i + 64 &&
                           desc_min_nonce(g.descs[k], l.C2) > read_bound(g.descs[k].job))
                        k++;
                    cancelled.push_back({x, g.offs[k]});
                    x = std::min<uint64_t>(g.offs[i + 1], end);
                } else {
                    x += r1 - r0;
                }
                continue;
            }
            const Part pt{&l, &D, row, r0, r1, x, g.offs[i + 1]};
            JobTrace& tr = trace[D.job];
            for_each_nonce(pt, [&](uint32_t p, uint32_t r, uint64_t n) {
                tr.hashed++;
                tr.largest = std::max(tr.largest, n);
                if (n - tr.lo < tr.seen.size()) {
                    tr.twice = tr.twice || tr.seen[n - tr.lo];
                    tr.seen[n - tr.lo] = true;
                }
                const uint64_t h = replay_hash(l, p, r);
                if (h > target) return;
                const int w = (int)(((p - D.p_first) & 255u) >> 6);
                if (wg.found[w] && n >= wg.n[w]) return;
                wg.n[w] = n;
                wg.h[w] = h;
                wg.found[w] = true;
                words[2 * (size_t)D.job] = std::min(words[2 * (size_t)D.job], n);  // atomicMin, at the hit
            });
            x += r1 - r0;
        }
    }

    // BatchReplay::group's workgroups and orders.
    void group(size_t gi, uint64_t order_seed, Rng& rng) {
        const VGroup& g = run.groups[gi];
        const size_t np = g.pieces.size();
        jitter = order_seed > 1 ? &rng : nullptr;
        cancelled.clear();
        at_launch.resize(run.st.njobs);
        for (size_t k = 0; k < run.st.njobs; k++) at_launch[k] = words[2 * k];
        const size_t grid = Stage::grid(run.st.groups[gi], std::min<unsigned int>(kReplayGrid, kBatchMaxGrid));
        const size_t W = order_seed == 0 ? 1 : order_seed == 1 ? std::min(grid, np)
                                                               : std::min({grid, np, (size_t)(2 + rng.next() % 7)});
        std::vector<FirstWg> wgs(W);
        for (size_t k = 0; k < np; k++) {
            const size_t w = order_seed == 0 ? 0 : order_seed == 1 ? k * W / np : rng.next() % W;
            wgs[w].pieces.push_back(k);
        }
        auto step = [&](FirstWg& wg) {
            const auto& pc = g.pieces[wg.pieces[wg.next++]];
            piece(g, wg, pc.first, pc.second);
            if (wg.next == wg.pieces.size()) flush(wg);  // the end of the kernel
        };
        if (order_seed <= 1) {
            for (size_t w = W; w-- > 0;)
                while (wgs[w].next < wgs[w].pieces.size()) step(wgs[w]);
            return;
        }
        std::vector<size_t> live;
        for (size_t w = 0; w < W; w++)
            if (!wgs[w].pieces.empty()) live.push_back(w);
        while (!live.empty()) {
            const size_t at = rng.next() % live.size();
            FirstWg& wg = wgs[live[at]];
            step(wg);
            if (wg.next == wg.pieces.size()) live.erase(live.begin() + (long)at);
        }
    }
};

constexpr uint64_t kTraceMaxSpan = 1ull << 24;  // a job's per-nonce record is kept up to this span

}  // namespace

extern "C" {

// gpuhash_first_below_batch as the engine runs it: hostcheck_min_batch's sub-batches and runs, each
// run a first-hit batch stage replayed group by group in stage order, with the order of a group's
// pieces chosen by order_seed (0, 1 or a shuffle, see FirstBatchReplay).  Returns 0, or -2 if some
// nonce was hashed twice, and per job out_found, and (out_hashes, out_nonces) when found (untouched
// otherwise), and in out_trace[3k..3k+2] what the replay hashed for job k: how many nonces, the
// largest of them (0 when none), and how many of the nonces from lower[k] to the answer it hashed
// (found jobs of at most 2^24 nonces; else all ones).  out_fill is hostcheck_min_batch's.
int hostcheck_first_below_batch(const uint8_t* msgs, const uint64_t* msg_off, uint64_t njobs, const uint64_t* lower,
                                const uint64_t* upper, const uint64_t* target, uint32_t rchunk, int policy,
                                uint64_t order_seed, uint64_t batch_bytes, int nshards, uint64_t* out_hashes,
                                uint64_t* out_nonces, int* out_found, uint64_t* out_trace, uint64_t* out_fill) {
    if (!msg_off || !lower || !upper || !target || !out_hashes || !out_nonces || !out_found || !out_trace ||
        !out_fill || !njobs || nshards < 1)
        return -1;
    for (uint64_t k = 0; k < njobs; k++)
        if (lower[k] > upper[k] || msg_off[k + 1] < msg_off[k]) return -1;
    Rng rng{order_seed};
    uint64_t fill[4] = {0, 0, 0, 0};
    bool twice = false;
    auto plan = [&](size_t k) {
        const uint64_t len = msg_off[k + 1] - msg_off[k];
        return plan_job(BatchJob{len ? msgs + msg_off[k] : nullptr, len, lower[k], upper[k]}, rchunk, policy,
                        /*host_ptab=*/true, /*pair=*/true);
    };
    auto run = [&](size_t first, std::vector<PlannedJob>& jobs) {
        fill[3]++;
        for (const auto& r : batch_runs(jobs, (size_t)nshards)) {
            const size_t n = r.second - r.first, at = first + r.first;
            std::vector<std::vector<Launch>> plans(n);
            for (size_t k = r.first; k < r.second; k++) plans[k - r.first] = std::move(jobs[k].plan);
            const Staged staged(plans, target + at, rchunk);
            std::vector<JobTrace> trace(n);
            for (size_t k = 0; k < n; k++) {
                trace[k].lo = lower[at + k];
                const uint64_t span = upper[at + k] - lower[at + k];
                if (span < kTraceMaxSpan) trace[k].seen.assign((size_t)span + 1, false);
            }
            FirstBatchReplay rep(staged, trace);
            for (size_t gi = 0; gi < staged.groups.size(); gi++) rep.group(gi, order_seed, rng);
            if (rep.list.size() >= fill[0]) { fill[0] = rep.list.size(); fill[1] = staged.st.list_cap; }
            fill[2] += rep.list.size() > staged.st.list_cap ? 1 : 0;
            for (size_t k = 0; k < n; k++) out_found[at + k] = 0;
            for (const BatchEntry& e : rep.list) {  // the host's fold: the lowest nonce
                const size_t k = at + e.job;
                if (!out_found[k] || e.nonce < out_nonces[k]) { out_hashes[k] = e.hash; out_nonces[k] = e.nonce; }
                out_found[k] = 1;
            }
            for (size_t k = 0; k < n; k++) {
                const JobTrace& t = trace[k];
                twice = twice || t.twice;
                uint64_t upto = ~0ull;
                if (out_found[at + k] && !t.seen.empty()) {
                    upto = 0;
                    for (uint64_t i = 0; i <= out_nonces[at + k] - t.lo; i++) upto += t.seen[(size_t)i] ? 1 : 0;
                }
                const uint64_t row[3] = {t.hashed, t.largest, upto};
                std::memcpy(out_trace + 3 * (at + k), row, sizeof row);
            }
        }
        return 0;
    };
    if (int rc = for_each_sub_batch((size_t)njobs, batch_bytes_bound(batch_bytes), plan, run)) return rc;
    std::memcpy(out_fill, fill, sizeof fill);
    return twice ? -2 : 0;
}

// The stage of ONE run of a first-hit batch, as hostcheck_stage_batch gives a batch's: the same
// words (the per-job region's size is then 16 bytes per job), the groups in launch order.
int hostcheck_stage_first_batch(const uint8_t* msgs, const uint64_t* msg_off, uint64_t njobs, const uint64_t* lower,
                                const uint64_t* upper, const uint64_t* target, uint32_t rchunk, uint64_t* out,
                                int cap, uint64_t* bytes, uint64_t* extra, uint8_t* meta, uint64_t meta_cap) {
    if (!msg_off || !lower || !upper || !target || !bytes || !extra || !njobs) return -1;
    std::vector<std::vector<Launch>> plans(njobs);
    for (uint64_t k = 0; k < njobs; k++) {
        if (lower[k] > upper[k] || msg_off[k + 1] < msg_off[k]) return -1;
        const uint64_t len = msg_off[k + 1] - msg_off[k];
        plan_range(len ? msgs + msg_off[k] : nullptr, len, lower[k], upper[k], plans[k], rchunk, g_policy);
    }
    const Stage st(plans, target, rchunk);
    for (int i = 0; i < (int)st.groups.size() && i < cap; i++) {
        const StageGroup& g = st.groups[(size_t)i];
        const uint64_t row[14] = {(uint64_t)g.J, (uint64_t)g.C2, (uint64_t)g.EX, g.idx.size(), (uint64_t)g.d,
                                  (uint64_t)g.c, g.total, g.nonces, g.work_at, g.offs_at, g.desc_at, g.ptab_at,
                                  sizeof(LaunchDesc) * g.idx.size(), g.ptab_bytes};
        std::memcpy(out + 14 * i, row, sizeof row);
    }
    *bytes = st.bytes;
    const uint64_t ex[8] = {st.upload_bytes, st.thresh_at, st.job_words_bytes() * st.njobs, st.list_at, st.list_cap,
                            sizeof(BatchEntry), st.tabs.size(), st.tab_words};
    std::memcpy(extra, ex, sizeof ex);
    if (meta && meta_cap >= st.bytes) {
        std::memset(meta, 0, st.bytes);
        st.fill(meta);
    }
    return (int)st.groups.size();
}

}  // extern "C"

// ---- early first-hit batch (gpuhash_first_below_batch_early): CPU replay of its rounds ----
//
// The rule, the rounds and their sub-batches as the engine cuts them (stage.h, early_limit and the
// chunk rule; gpuhash.cpp, early_rounds), each round's stage from the bytes fill() wrote and
// k_pack_first over its tiles through PackReplay: pack.h's own hashing, the orders and the stale
// reads of the packed replay (a stale bound is the word as armed, all ones: every round is a stage
// of its own).  A wave's run keeps the lanes at or below the bound it read -- a wave none of whose
// lanes is has nothing to commit, which is the kernel's skip -- and its lowest hit lane does the
// atomicMin and the bounded append.  The skip is modelled by its outcome only: the replay cannot
// catch a fault in the branch itself (a skip that is not wave-uniform, or one placed before the
// runs are computed); the GPU tests alone cover that branch.  The remainder goes through
// hostcheck_first_below_batch.

namespace {

// One round's packed group over the stage's {bound, target} words.  Returns the appends in all,
// kept or not.
uint64_t pack_first_group(const Staged& staged, std::vector<uint64_t>& words, std::vector<BatchEntry>& list,
                          uint64_t order_seed, Rng& rng) {
    const PackReplay pk(staged);
    uint32_t head[4];
    std::memcpy(head, staged.meta.data() + staged.st.list_at, sizeof head);
    const uint64_t cap = head[1];
    uint64_t appended = 0;
    pk.group(order_seed, rng,
             [&](PackRun& r, bool stale) {
                 r.seen = stale ? ~0ull : words[2 * (size_t)r.job];
                 const uint64_t target = words[2 * (size_t)r.job + 1];
                 // the run's lowest hit lane among those that needed their hash
                 std::vector<PackLane> hit;
                 for (const PackLane& l : r.lanes)
                     if (l.n <= r.seen && l.h <= target) { hit.push_back(l); break; }
                 r.lanes = hit;
             },
             [&](PackRun& r) {
                 if (r.lanes.empty()) return;
                 const PackLane& b = r.lanes[0];
                 const uint64_t old = words[2 * (size_t)r.job];  // the atomicMin
                 words[2 * (size_t)r.job] = std::min(old, b.n);
                 if (b.n > old) return;  // equal only at 2^64-1 against the word as armed
                 if (appended++ < cap) list.push_back(BatchEntry{b.h, b.n, r.job, 0});
             });
    return appended;
}

}  // namespace

extern "C" {

uint64_t hostcheck_early_limit(uint64_t lower, uint64_t upper, uint64_t target, uint64_t prefix) {
    return early_limit(lower, upper, target, prefix);
}

uint64_t hostcheck_early_first_chunk(uint64_t fronts) { return early_first_chunk(fronts); }

// gpuhash_first_below_batch_early as the engine runs it.  Returns what hostcheck_first_below_batch
// returns, the per-job results as it gives them, in out_packed[k] the packed nonces handed out to
// job k (the pieces of the rounds it was open in: what it hashed at most), and in out_fill[0..5]:
// the largest result-list fill of any round's stage (appends the bounded store left out included),
// that stage's capacity, how many stages filled their list past it, the number of round stages,
// the remainder's stages over their bound, and c_0.
int hostcheck_first_below_batch_early(const uint8_t* msgs, const uint64_t* msg_off, uint64_t njobs,
                                      const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                                      uint64_t prefix, uint32_t rchunk, int policy, uint64_t order_seed,
                                      uint64_t batch_bytes, int nshards, uint64_t* out_hashes, uint64_t* out_nonces,
                                      int* out_found, uint64_t* out_packed, uint64_t* out_fill) {
    if (!msg_off || !lower || !upper || !target || !out_hashes || !out_nonces || !out_found || !out_packed ||
        !out_fill || !njobs || nshards < 1 || prefix > GPUHASH_BATCH_MAX_SPAN)
        return -1;
    for (uint64_t k = 0; k < njobs; k++)
        if (lower[k] > upper[k] || msg_off[k + 1] < msg_off[k] || upper[k] - lower[k] >= GPUHASH_BATCH_MAX_SPAN)
            return -1;
    Rng rng{order_seed};
    uint64_t fill[6] = {0, 0, 0, 0, 0, 0};
    std::vector<uint64_t> limit(njobs), used(njobs, 0);
    std::vector<size_t> fronts;
    for (uint64_t k = 0; k < njobs; k++) {
        out_found[k] = 0;
        limit[k] = early_limit(lower[k], upper[k], target[k], prefix);
        if (limit[k]) fronts.push_back((size_t)k);
    }
    std::vector<PackJob> recs(njobs);
    for (size_t k : fronts) {
        const uint64_t len = msg_off[k + 1] - msg_off[k];
        recs[k] = PackTables::record(len ? msgs + msg_off[k] : nullptr, len);
    }
    const uint64_t c0 = fill[5] = early_first_chunk(fronts.size());
    const size_t nruns = std::min<size_t>((size_t)nshards, fronts.size());
    for (size_t r = 0; r < nruns; r++) {
        const std::vector<size_t> mine(fronts.begin() + (long)(fronts.size() * r / nruns),
                                       fronts.begin() + (long)(fronts.size() * (r + 1) / nruns));
        for (uint64_t c = c0;; c = early_next_chunk(c)) {
            std::vector<size_t> open;
            std::vector<BatchJob> piece;
            std::vector<uint64_t> tg;
            for (size_t k : mine) {
                if (out_found[k] || used[k] >= limit[k]) continue;
                const uint64_t lo = lower[k] + used[k], len = msg_off[k + 1] - msg_off[k];
                open.push_back(k);
                piece.push_back(BatchJob{len ? msgs + msg_off[k] : nullptr, len, lo,
                                         lo + (std::min(c, limit[k] - used[k]) - 1), &recs[k]});
                tg.push_back(target[k]);
            }
            if (open.empty()) break;
            auto plan = [&](size_t i) {
                PlannedJob p = plan_packed_job(piece[i]);
                p.bytes += 8;
                return p;
            };
            auto run = [&](size_t first, std::vector<PlannedJob>& jobs) {
                StageJobs sj(jobs, 0, jobs.size());
                const Staged staged(sj.plans, tg.data() + first, rchunk, sj.which());
                if (staged.st.groups.size() != 1 || staged.st.groups[0].C2 != 4) return -3;  // the packed group alone
                std::vector<uint64_t> words(2 * jobs.size());
                std::memcpy(words.data(), staged.meta.data() + staged.st.thresh_at, 16 * jobs.size());
                std::vector<BatchEntry> list;
                const uint64_t appended = pack_first_group(staged, words, list, order_seed, rng);
                fill[3]++;
                if (appended >= fill[0]) { fill[0] = appended; fill[1] = staged.st.list_cap; }
                fill[2] += appended > staged.st.list_cap ? 1 : 0;
                for (const BatchEntry& e : list) {  // the host's fold: the lowest nonce
                    const size_t k = open[first + e.job];
                    if (!out_found[k] || e.nonce < out_nonces[k]) { out_hashes[k] = e.hash; out_nonces[k] = e.nonce; }
                    out_found[k] = 1;
                }
                return 0;
            };
            if (int rc = for_each_sub_batch(open.size(), batch_bytes_bound(batch_bytes), plan, run)) return rc;
            for (size_t i = 0; i < open.size(); i++) used[open[i]] += piece[i].hi - piece[i].lo + 1;
        }
    }
    for (uint64_t k = 0; k < njobs; k++) out_packed[k] = used[k];
    // the remainder: the jobs still open, each with its own copy of its message
    std::vector<size_t> sel;
    std::vector<uint64_t> lo2, hi2, tg2, off2(1, 0);
    std::vector<uint8_t> msgs2;
    for (uint64_t k = 0; k < njobs; k++) {
        if (out_found[k] || used[k] > upper[k] - lower[k]) continue;
        sel.push_back((size_t)k);
        lo2.push_back(lower[k] + used[k]);
        hi2.push_back(upper[k]);
        tg2.push_back(target[k]);
        if (msg_off[k + 1] > msg_off[k]) msgs2.insert(msgs2.end(), msgs + msg_off[k], msgs + msg_off[k + 1]);
        off2.push_back(msgs2.size());
    }
    int rc = 0;
    if (!sel.empty()) {
        const size_t n = sel.size();
        std::vector<uint64_t> h2(n), n2(n), trace(3 * n), fill2(4);
        std::vector<int> f2(n);
        rc = hostcheck_first_below_batch(msgs2.data(), off2.data(), n, lo2.data(), hi2.data(), tg2.data(), rchunk, policy,
                                         order_seed, batch_bytes, nshards, h2.data(), n2.data(), f2.data(), trace.data(),
                                         fill2.data());
        if (rc != 0 && rc != -2) return rc;
        fill[4] = fill2[2];
        for (size_t i = 0; i < n; i++) {
            if (!f2[i]) continue;
            out_found[sel[i]] = 1;
            out_hashes[sel[i]] = h2[i];
            out_nonces[sel[i]] = n2[i];
        }
    }
    std::memcpy(out_fill, fill, sizeof fill);
    return rc;
}

}  // extern "C"

// ---- collect batch (gpuhash_collect_below_batch): CPU replay of the kernel's MODE 6 ----
//
// A collect batch stage's groups, pieces, parts and masks as k_scan<.., 6> walks them, from the
// bytes fill() wrote: batch_find's lookup, the job change (nothing to flush: the workgroup takes
// the new job's counter, target and list flag), the per-job counters and the ONE list with its
// 64-bit append counter and its capacity.  What a GPU decides by timing -- which workgroup takes
// which piece, and so the order of the appends and which hits a full list drops -- is chosen by a
// seed, as in BatchReplay::group.  The host side is the engine's: collect.h's fold_collect_batch,
// with the re-runs replayed as hostcheck_collect_below replays a single collection.

namespace {

struct CollectBatchReplay {
    const Staged& run;
    const uint64_t* words;  // per job: counter, target, lists -- as fill() armed them
    std::vector<uint64_t> counts;
    std::vector<BatchEntry> list;
    uint64_t appended = 0;  // the list head's 64-bit counter
    uint64_t cap;           // and its capacity
    Rng* jitter = nullptr;

    explicit CollectBatchReplay(const Staged& r)
        : run(r), words(reinterpret_cast<const uint64_t*>(r.meta.data() + r.st.thresh_at)), counts(r.st.njobs) {
        uint32_t head[4];
        std::memcpy(head, r.meta.data() + r.st.list_at, sizeof head);
        cap = head[2];
        for (size_t k = 0; k < r.st.njobs; k++) counts[k] = words[kCollectJobWords * k];
    }

    void piece(const VGroup& g, ReplayWg& wg, uint64_t x, uint64_t end) {
        while (x < end) {
            if (jitter && jitter->next() % 4 == 0) wg.idx = (int)(jitter->next() % g.ls.size());
            const int i = wg.idx = BatchReplay::find(g, wg.idx, x);
            const LaunchDesc& D = g.descs[i];
            const uint32_t rel = (uint32_t)(x - g.offs[i]);
            const uint32_t row = rel / D.R, r0 = rel - row * D.R;
            const uint64_t left = end - x;
            const uint32_t r1 = (uint64_t)(D.R - r0) < left ? D.R : r0 + (uint32_t)left;
            wg.job = D.job;  // the job change: no per-wave state to leave behind
            const uint64_t target = words[kCollectJobWords * D.job + 1];
            const bool lists = words[kCollectJobWords * D.job + 2] != 0;
            const Part pt{g.ls[(size_t)i], &D, row, r0, r1, x, g.offs[i + 1]};
            for_each_nonce(pt, [&](uint32_t p, uint32_t r, uint64_t n) {
                const uint64_t h = replay_hash(*pt.l, p, r);
                if (h > target) return;
                counts[D.job]++;
                if (!lists) return;
                const uint64_t slot = appended++;
                if (slot < cap) list.push_back(BatchEntry{h, n, D.job, 0});
            });
            x += r1 - r0;
        }
    }

    // The workgroups and the order of their pieces: BatchReplay::group's three kinds.
    void group(size_t gi, uint64_t order_seed, Rng& rng) {
        const VGroup& g = run.groups[gi];
        const size_t np = g.pieces.size();
        jitter = order_seed > 1 ? &rng : nullptr;
        const size_t grid = Stage::grid(run.st.groups[gi], std::min<unsigned int>(kReplayGrid, kBatchMaxGrid));
        const size_t W = order_seed == 0 ? 1 : order_seed == 1 ? std::min(grid, np)
                                                               : std::min({grid, np, (size_t)(2 + rng.next() % 7)});
        std::vector<ReplayWg> wgs(W);
        for (size_t k = 0; k < np; k++) {
            const size_t w = order_seed == 0 ? 0 : order_seed == 1 ? k * W / np : rng.next() % W;
            wgs[w].pieces.push_back(k);
        }
        auto step = [&](ReplayWg& wg) {
            const auto& pc = g.pieces[wg.pieces[wg.next++]];
            piece(g, wg, pc.first, pc.second);
        };
        if (order_seed <= 1) {
            for (size_t w = W; w-- > 0;)
                while (wgs[w].next < wgs[w].pieces.size()) step(wgs[w]);
            return;
        }
        std::vector<size_t> live;
        for (size_t w = 0; w < W; w++)
            if (!wgs[w].pieces.empty()) live.push_back(w);
        while (!live.empty()) {
            const size_t at = rng.next() % live.size();
            ReplayWg& wg = wgs[live[at]];
            step(wg);
            if (wg.next == wg.pieces.size()) live.erase(live.begin() + (long)at);
        }
    }
};

// The packed group's collect mode over the stage's counters and list, which `rep` holds for the
// unpacked groups too: per run one add on the job's counter and, if the job lists, one on the
// list's append counter; the hits are stored in lane order while the slot is below the capacity.
void pack_collect_group(const Staged& staged, CollectBatchReplay& rep, uint64_t order_seed, Rng& rng) {
    const PackReplay pk(staged);
    pk.group(order_seed, rng,
             [&](PackRun& r, bool) {
                 const uint64_t target = rep.words[kCollectJobWords * r.job + 1];
                 std::vector<PackLane> hits;
                 for (const PackLane& l : r.lanes)
                     if (l.h <= target) hits.push_back(l);
                 r.lanes.swap(hits);
             },
             [&](PackRun& r) {
                 if (r.lanes.empty()) return;
                 rep.counts[r.job] += r.lanes.size();
                 if (!rep.words[kCollectJobWords * r.job + 2]) return;
                 const uint64_t base = rep.appended;
                 rep.appended += r.lanes.size();
                 for (size_t i = 0; i < r.lanes.size(); i++)
                     if (base + i < rep.cap) rep.list.push_back(BatchEntry{r.lanes[i].h, r.lanes[i].n, r.job, 0});
             });
}

}  // namespace

extern "C" {

// gpuhash_collect_below_batch as the engine runs it: the same sub-batches (for_each_sub_batch under
// batch_bytes, 0: the engine's bound), runs over nshards context entries (batch_runs), collect
// batch stages and fold (collect.h, fold_collect_batch), each run replayed as above with the order
// of its pieces chosen by order_seed (0, 1 or a shuffle) and a list of buffer_entries entries, and
// each re-run replayed as hostcheck_collect_below replays a collection (one shard, the same list
// size).  Under a policy with GPUHASH_LAYOUT_PACKED_ALWAYS the jobs that pack are staged and
// replayed as the packed group (pack_collect_group); a re-run is unpacked, as in the engine.
// msg_off has njobs + 1 entries; out_off has njobs + 1 entries or is null (every cap 0).
// Returns 0 and out_totals[k], the lowest min(cap_k, total_k) hits of job k from out_off[k] on in
// out_nonces / out_hashes (untouched beyond), and in out_info[0..3]: the largest number of entries
// any run's list held, the number of jobs that were re-run, the number of sub-batches, and the
// number of sub-range runs the re-runs' collectors asked for.
int hostcheck_collect_below_batch(const uint8_t* msgs, const uint64_t* msg_off, uint64_t njobs,
                                  const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                                  uint32_t rchunk, int policy, uint64_t order_seed, uint64_t batch_bytes,
                                  int nshards, uint64_t buffer_entries, const uint64_t* out_off,
                                  uint64_t* out_nonces, uint64_t* out_hashes, uint64_t* out_totals,
                                  uint64_t* out_info) {
    if (!msg_off || !lower || !upper || !target || !out_totals || !out_info || !njobs || nshards < 1) return -1;
    std::vector<size_t> caps(njobs, 0);
    std::vector<uint8_t> lists(njobs, 0);
    for (uint64_t k = 0; k < njobs; k++) {
        if (lower[k] > upper[k] || msg_off[k + 1] < msg_off[k]) return -1;
        if (out_off && out_off[k + 1] < out_off[k]) return -1;
        caps[k] = out_off ? (size_t)(out_off[k + 1] - out_off[k]) : 0;
        lists[k] = caps[k] ? 1 : 0;
    }
    if (out_off && out_off[njobs] > 0 && (!out_nonces || !out_hashes)) return -1;
    Rng rng{order_seed};
    const uint64_t B = std::max<uint64_t>(buffer_entries, 1);
    uint64_t info[4] = {0, 0, 0, 0};
    std::vector<JobHits> res(njobs);
    auto message = [&](size_t k, uint64_t& len) {
        len = msg_off[k + 1] - msg_off[k];
        return len ? msgs + msg_off[k] : nullptr;
    };
    auto plan = [&](size_t k) {
        uint64_t len;
        const uint8_t* const m = message(k, len);
        const BatchJob j{m, len, lower[k], upper[k]};
        if (packs(policy, j.lo, j.hi)) return plan_packed_job(j, /*collects=*/true);
        return plan_job(j, rchunk, policy, /*host_ptab=*/true, /*pair=*/false, /*collects=*/true);
    };
    auto run = [&](size_t first, std::vector<PlannedJob>& jobs) {
        info[2]++;
        const auto runs = batch_runs(jobs, (size_t)nshards);
        for (size_t ri = 0; ri < runs.size(); ri++) {
            const auto& r = runs[ri];
            const size_t k0 = first + r.first, n = r.second - r.first;
            StageJobs sj(jobs, r.first, r.second);
            const Staged staged(sj.plans, target + k0, lists.data() + k0, B, rchunk, sj.which());
            CollectBatchReplay rep(staged);
            for (size_t gi = 0; gi < staged.groups.size(); gi++) {
                if (staged.st.groups[gi].C2 == 4) pack_collect_group(staged, rep, order_seed, rng);
                else rep.group(gi, order_seed, rng);
            }
            info[0] = std::max<uint64_t>(info[0], rep.list.size());
            auto rerun = [&](size_t j, size_t cap, JobHits& out) {
                const size_t k = k0 + j;
                uint64_t len;
                const uint8_t* const m = message(k, len);
                auto one = [&](const std::vector<SubRange>& batch, bool want_list, std::vector<SubResult>& rs) {
                    for (size_t i = 0; i < batch.size(); i++) {
                        info[3]++;
                        collect_run(m, len, batch[i], rchunk, target[k], policy, order_seed, rng, want_list ? B : 0,
                                    rs[i]);
                    }
                    return 0;
                };
                auto split = [&](uint64_t a, uint64_t b, std::vector<SubRange>& batch) {
                    batch.push_back(SubRange{a, b, (int)ri});
                };
                Collector<decltype(one), decltype(split)> c(B, cap, one, split);
                const int rc = c.collect(lower[k], upper[k], slice_width(1));
                out.total = c.total;
                out.held = std::move(c.held);
                return rc;
            };
            if (int rc = fold_collect_batch(n, rep.counts.data(), rep.list.data(), rep.list.size(), caps.data() + k0,
                                            -3, rerun, res.data() + k0, &info[1]))
                return rc;
        }
        return 0;
    };
    if (int rc = for_each_sub_batch((size_t)njobs, batch_bytes_bound(batch_bytes), plan, run)) return rc;
    for (uint64_t k = 0; k < njobs; k++) {
        out_totals[k] = res[k].total;
        for (size_t i = 0; i < res[k].held.size(); i++) {
            out_nonces[out_off[k] + i] = res[k].held[i].nonce;
            out_hashes[out_off[k] + i] = res[k].held[i].hash;
        }
    }
    std::memcpy(out_info, info, sizeof info);
    return 0;
}

// The stage of ONE run of a collect batch, as hostcheck_stage_batch gives a batch's: the same
// words (the per-job region's size is then 24 bytes per job; the list's position is that of its
// 16-byte head, which ends the buffer, and its capacity buffer_entries).
int hostcheck_stage_collect_batch(const uint8_t* msgs, const uint64_t* msg_off, uint64_t njobs,
                                  const uint64_t* lower, const uint64_t* upper, const uint64_t* target,
                                  const uint8_t* lists, uint64_t buffer_entries, uint32_t rchunk, uint64_t* out,
                                  int cap, uint64_t* bytes, uint64_t* extra, uint8_t* meta, uint64_t meta_cap) {
    if (!msg_off || !lower || !upper || !target || !lists || !bytes || !extra || !njobs) return -1;
    std::vector<std::vector<Launch>> plans(njobs);
    for (uint64_t k = 0; k < njobs; k++) {
        if (lower[k] > upper[k] || msg_off[k + 1] < msg_off[k]) return -1;
        const uint64_t len = msg_off[k + 1] - msg_off[k];
        plan_range(len ? msgs + msg_off[k] : nullptr, len, lower[k], upper[k], plans[k], rchunk, g_policy);
    }
    const Stage st(plans, target, lists, buffer_entries, rchunk);
    for (int i = 0; i < (int)st.groups.size() && i < cap; i++) {
        const StageGroup& g = st.groups[(size_t)i];
        const uint64_t row[14] = {(uint64_t)g.J, (uint64_t)g.C2, (uint64_t)g.EX, g.idx.size(), (uint64_t)g.d,
                                  (uint64_t)g.c, g.total, g.nonces, g.work_at, g.offs_at, g.desc_at, g.ptab_at,
                                  sizeof(LaunchDesc) * g.idx.size(), g.ptab_bytes};
        std::memcpy(out + 14 * i, row, sizeof row);
    }
    *bytes = st.bytes;
    const uint64_t ex[8] = {st.upload_bytes, st.thresh_at, st.job_words_bytes() * st.njobs, st.list_at, st.list_cap,
                            sizeof(BatchEntry), st.tabs.size(), st.tab_words};
    std::memcpy(extra, ex, sizeof ex);
    if (meta && meta_cap >= st.bytes) {
        std::memset(meta, 0, st.bytes);
        st.fill(meta);
    }
    return (int)st.groups.size();
}

}  // extern "C"
