// control.h -- what lets a caller outside a blocking search reach into it: the cancel latch
// (gpuhash_cancel / gpuhash_resume), the progress mailbox (gpuhash_progress) and the word that
// drains a resident launch's work counters.  Host-only, plain C++: no HIP.  gpuhash.cpp uses it
// with the device behind it; control_check_main.cpp runs the same code against fake calls under
// ThreadSanitizer.
#pragma once
#include <atomic>
#include <chrono>
#include <cstdint>
#include <memory>
#include <mutex>
#include <thread>

#include "stage.h"

namespace gpuhash {

// ---- the drain word -------------------------------------------------------------------------
// A scan workgroup takes work with atomicAdd(work, g) and leaves its loop when the value it got
// is >= the group's total, offs[ndesc] (scan_kernel.h, k_scan).  Writing kDrainWord over a
// group's counter therefore ends the launch within one piece per workgroup.
constexpr uint64_t kDrainWord = 1ull << 62;

// The planner's own maxima.  A descriptor holds fewer than 2^32 row-iterations (plan.h: rows * R
// < 2^32), and a stage's descriptors lie in a metadata buffer of at most 1 GiB (stage.h,
// batch_bytes_bound; a single search's slice plans a few hundred), so a group's total is below
// kMaxGroupTotal.
constexpr uint64_t kMaxDescRowIterations = 1ull << 32;
constexpr uint64_t kMaxStageDescs = (1ull << 30) / sizeof(LaunchDesc) + 1;
constexpr uint64_t kMaxGroupTotal = kMaxDescRowIterations * kMaxStageDescs;
// A launch has at most this many workgroups: a batch's kBatchMaxGrid, and far above what any
// device holds resident of a single search's kernels (grid_for; an MI355X holds 2048).
constexpr uint64_t kMaxGrid = 1ull << 20;
constexpr uint64_t kMaxPiece = 1ull << 32;  // gmax is a uint32 (rchunk)
static_assert(kBatchMaxGrid <= kMaxGrid && kDefaultMaxPiece < kMaxPiece, "the bounds cover the planner's values");
// it exceeds every possible offs[ndesc]: a workgroup that grabs after the drain gets a value
// >= total and leaves
static_assert(kDrainWord > kMaxGroupTotal, "the drain word is above every group's total");
// every workgroup adds at most one piece to a drained counter before it leaves, and the counter
// held less than total + grid * gmax before: neither sum wraps
static_assert(kMaxGroupTotal + kMaxGrid * kMaxPiece < kDrainWord, "a live counter stays below the drain word");
static_assert(kDrainWord <= ~0ull - kMaxGrid * kMaxPiece, "a drained counter cannot wrap");
// MODE 5 (and the first-hit skip of MODE 2) raise the counter with atomicMax(work, x), x <=
// offs[ndesc] < kDrainWord: the larger value stays, so a drained counter stays drained

// The least length of a copy that must land while a persistent grid is resident.  Measured on an
// MI355X: the runtime runs a short copy as a shader blit -- an 8-byte or 40-byte
// copy on a second stream completed only when the grid had drained, with or without an event wait
// in front of it -- and hands a long one to a copy engine, which runs beside the grid and whose
// writes the grid's atomics see.
constexpr size_t kControlCopyBytes = 64 * 1024;
static_assert(kControlCopyBytes >= 64 * 1024, "the metadata buffers' least size, which the K+W stage always had");

static_assert(std::atomic<uint32_t>::is_always_lock_free && std::atomic<uint64_t>::is_always_lock_free,
              "gpuhash_cancel is one lock-free store: async-signal-safe");

inline uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// The share of a group's `nonces` whose work has been handed out when its counter reads
// `counter` of `total` row-iterations.
inline uint64_t handed_out(uint64_t nonces, uint64_t counter, uint64_t total) {
    if (!total) return nonces;
    return (uint64_t)((unsigned __int128)nonces * std::min(counter, total) / total);
}

// One per context.  The threads involved:
//   the caller   of a search, holding the context's mutex: begin_call .. end_call
//   the waiters  one per context entry the call runs on (the caller itself when that is one):
//                each sits in host_wait's poll loop, slot = its entry's index
//   outsiders    any thread: cancel(), resume(), progress().  They never take the context's mutex.
class Control {
   public:
    explicit Control(size_t entries) : nslots_(entries), slots_(new Slot[entries]) {}

    // ---- the latch ----
    void cancel() { latch_.store(1u, std::memory_order_seq_cst); }  // this store and nothing else
    void resume() { latch_.store(0u, std::memory_order_seq_cst); }

    // True once the call in flight has seen the latch set; from then on it stays cancelled,
    // whatever resume() does.  Called at call entry, before every run of the entries, and in every
    // iteration of the poll loop (one relaxed load while nothing is set).
    bool observe() {
        if (latch_.load(std::memory_order_relaxed)) seen_.store(1u, std::memory_order_relaxed);
        return seen_.load(std::memory_order_relaxed) != 0;
    }

    // ---- a call's life (the caller, under the context's mutex) ----
    void begin_call(uint64_t total) {
        std::lock_guard<std::mutex> lock(ask_);  // no asker of the last call is still summing
        seen_.store(0u, std::memory_order_relaxed);
        total_.store(total, std::memory_order_relaxed);
        finished_.store(0, std::memory_order_relaxed);
        high_ = 0;
        for (size_t k = 0; k < nslots_; k++) {
            slots_[k].part.store(0, std::memory_order_relaxed);
            slots_[k].served.store(0, std::memory_order_relaxed);
            slots_[k].polling.store(0u, std::memory_order_relaxed);
        }
        ticket_.store(0, std::memory_order_relaxed);
        epoch_.fetch_add(1, std::memory_order_release);  // odd: in flight
    }
    // Releases every progress request still waiting.
    void end_call() { epoch_.fetch_add(1, std::memory_order_release); }

    // ---- the waiters ----
    void poll_enter(size_t slot) { slots_[slot].polling.store(1u, std::memory_order_release); }
    void poll_exit(size_t slot) { slots_[slot].polling.store(0u, std::memory_order_release); }
    // The request this waiter has not answered yet, 0 when there is none.
    uint64_t wanted(size_t slot) const {
        const uint64_t t = ticket_.load(std::memory_order_acquire);
        return t > slots_[slot].served.load(std::memory_order_relaxed) ? t : 0;
    }
    // Answers request `ticket`: `part` nonces of the stage now running on this entry are handed out.
    void publish(size_t slot, uint64_t ticket, uint64_t part) {
        slots_[slot].part.store(part, std::memory_order_relaxed);
        slots_[slot].served.store(ticket, std::memory_order_release);
    }
    // The entry's stage is over: its nonces count as finished.  The part goes first, so that a
    // sum taken in between is short, never double (progress() only ever raises what it reports).
    void stage_done(size_t slot, uint64_t nonces) {
        slots_[slot].part.store(0, std::memory_order_release);
        uint64_t f = finished_.load(std::memory_order_relaxed);
        while (!finished_.compare_exchange_weak(f, sat_add(f, nonces), std::memory_order_release,
                                                std::memory_order_relaxed)) {
        }
    }

    // ---- outsiders ----
    // (done, total) of the call in flight, (0, 0) when there is none or it ends first.  Posts a
    // request and waits until every waiter that is polling has answered it; waiters that are not
    // (between stages, or under a wait mode that does not poll) count with what is finished.
    void progress(uint64_t* out_done, uint64_t* out_total) {
        *out_done = *out_total = 0;
        std::lock_guard<std::mutex> lock(ask_);
        const uint64_t e = epoch_.load(std::memory_order_acquire);
        if (!(e & 1)) return;
        const uint64_t t = ticket_.fetch_add(1, std::memory_order_acq_rel) + 1;
        for (;;) {
            if (epoch_.load(std::memory_order_acquire) != e) return;  // released at call end
            bool ready = true;
            for (size_t k = 0; k < nslots_ && ready; k++)
                ready = !slots_[k].polling.load(std::memory_order_acquire) ||
                        slots_[k].served.load(std::memory_order_acquire) >= t;
            if (ready) break;
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
        const uint64_t total = total_.load(std::memory_order_relaxed);
        // finished_ first: stage_done clears a part before it adds it there, so a part is never
        // counted in both
        uint64_t sum = finished_.load(std::memory_order_acquire);
        for (size_t k = 0; k < nslots_; k++) sum = sat_add(sum, slots_[k].part.load(std::memory_order_acquire));
        high_ = std::max(high_, std::min(sum, total));
        if (epoch_.load(std::memory_order_acquire) != e) return;
        *out_done = high_;
        *out_total = total;
    }

   private:
    struct Slot {
        std::atomic<uint64_t> part{0}, served{0};
        std::atomic<uint32_t> polling{0};
    };
    std::atomic<uint32_t> latch_{0}, seen_{0};
    std::atomic<uint64_t> epoch_{0}, total_{0}, finished_{0}, ticket_{0};
    std::mutex ask_;     // outsiders among themselves, and begin_call: never the context's mutex
    uint64_t high_ = 0;  // under ask_: the most progress() has reported of this call
    const size_t nslots_;
    std::unique_ptr<Slot[]> slots_;
};

}  // namespace gpuhash
