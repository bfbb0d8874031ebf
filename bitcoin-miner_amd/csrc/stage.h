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
    int d = 0, c = 0;         // digits and digit blocks of its largest launch (the first such)
    // byte positions in the metadata buffer, each 16-byte aligned: the counter block, the
    // n + 1 prefix offsets (8 B each), the n descriptors, and for C2 = 3 the launches' p-tables
    size_t work_at = 0, offs_at = 0, desc_at = 0, ptab_at = 0, ptab_bytes = 0;
};

// A uniform K+W table of C2 = 1 / J = 0 descriptors: block B's words depend only on the digit
// count d, so one table of 64 x R words per d serves all of them; k_ktab builds it from the
// device copy of the first such descriptor, at desc_byte.
struct StageTab {
    int d;
    uint32_t off, R;  // words
    size_t desc_byte;
};

struct Stage {
    std::vector<Launch> plan;  // desc.tab_off set as the kernels read it
    std::vector<StageGroup> groups;  // in first-appearance order of (J, C2, EX)
    std::vector<StageTab> tabs;
    size_t tab_words = 0, bytes = 0;  // of all K+W tables; of the metadata buffer
    uint32_t gmax, gmin;              // piece size bounds

    Stage(const uint8_t* msg, uint64_t len, uint64_t lo, uint64_t hi, uint32_t rchunk, int policy,
          bool host_ptab = false) : gmax(rchunk ? rchunk : kDefaultMaxPiece), gmin(std::min(kMinPiece, gmax)) {
        plan_range(msg, len, lo, hi, plan, rchunk, policy, host_ptab);
        for (size_t i = 0; i < plan.size(); i++) {
            const Launch& l = plan[i];
            auto it = std::find_if(groups.begin(), groups.end(), [&](const StageGroup& g) {
                return g.J == l.J && g.C2 == l.C2 && g.EX == l.EX;
            });
            if (it == groups.end()) it = groups.insert(it, StageGroup{l.J, l.C2, l.EX});
            it->idx.push_back(i);
        }
        auto align = [&] { bytes = (bytes + 15) & ~(size_t)15; };
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
                    auto it = std::find_if(tabs.begin(), tabs.end(), [&](const StageTab& t) { return t.d == l.d; });
                    if (it == tabs.end()) {
                        const size_t at = g.desc_at + k * sizeof(LaunchDesc);
                        it = tabs.insert(it, StageTab{l.d, (uint32_t)tab_words, D.R, at});
                        tab_words += 64ull * D.R;
                    }
                    D.tab_off = it->off;
                }
            }
            bytes += g.ptab_bytes;
            align();
        }
    }

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
    }

    // Workgroups of a group's launch, given the kernel's resident capacity on the device.
    static unsigned int grid(const StageGroup& g, unsigned int resident) {
        const uint64_t pieces = (g.total + kMinPiece - 1) / kMinPiece;
        return (unsigned int)std::min<uint64_t>(resident, std::max<uint64_t>(pieces, 1));
    }
};

}  // namespace gpuhash
