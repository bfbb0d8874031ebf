// control_check_main.cpp -- stand-alone race check of control.h (built with -fsanitize=thread as
// lib/control_tsan; tests/test_cancel_cpu.py runs it).  Fake "calls" run on a fake device: a work
// counter that a device thread raises piece by piece, and waiting threads, several per call, whose
// loop polls as gpuhash.cpp's poll_wait does -- the latch, then the progress mailbox -- against
// threads that cancel, resume and ask for progress all the while.  Checked:
//   every call in flight at a cancel returns cancelled;
//   no call started after a resume returns cancelled unless a later cancel came;
//   every progress request is answered or released (the program ends: no deadlock at call end);
//   `done` is monotone within a call and never above `total`.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <vector>

#include "control.h"

using namespace gpuhash;

namespace {

constexpr size_t kEntries = 3;  // waiting threads per call
constexpr uint64_t kTotal = 4000, kNonces = 1000000, kPiece = 40;

std::atomic<int> failures{0};
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "control_check: %s (line %d)\n", #cond, __LINE__); \
            failures.fetch_add(1);                                           \
        }                                                                    \
    } while (0)

// One entry's stage on the fake device: workgroups take pieces of the counter until it is >= total.
struct FakeStage {
    std::atomic<uint64_t> work{0};
    std::atomic<bool> done{false};
    void device() {
        while (work.fetch_add(kPiece, std::memory_order_relaxed) < kTotal) std::this_thread::yield();
        done.store(true, std::memory_order_release);
    }
};

// poll_wait: returns true when the call has seen the latch.
bool wait_stage(Control& C, size_t slot, FakeStage& st) {
    bool drained = false;
    C.poll_enter(slot);
    while (!st.done.load(std::memory_order_acquire)) {
        if (!drained && C.observe()) {
            drained = true;
            st.work.store(kDrainWord, std::memory_order_relaxed);  // the drain copy
        }
        if (const uint64_t t = C.wanted(slot))
            C.publish(slot, t, handed_out(kNonces, st.work.load(std::memory_order_relaxed), kTotal));
        std::this_thread::yield();
    }
    C.poll_exit(slot);
    if (C.observe()) return true;
    C.stage_done(slot, kNonces);
    return false;
}

// A search: `stages` rounds of kEntries concurrent stages.  Returns true when cancelled.
bool fake_call(Control& C, std::mutex& mu, int stages) {
    std::lock_guard<std::mutex> lock(mu);
    struct End {
        Control& C;
        ~End() { C.end_call(); }
    };
    C.begin_call(kNonces * kEntries * (uint64_t)stages);
    End end{C};
    if (C.observe()) return true;
    for (int s = 0; s < stages; s++) {
        if (C.observe()) return true;
        FakeStage st[kEntries];
        bool cancelled[kEntries] = {};
        std::vector<std::thread> th;
        for (size_t k = 0; k < kEntries; k++) {
            th.emplace_back([&, k] { st[k].device(); });
            th.emplace_back([&, k] { cancelled[k] = wait_stage(C, k, st[k]); });
        }
        for (auto& t : th) t.join();
        for (bool c : cancelled)
            if (c) return true;
    }
    return false;
}

}  // namespace

int main() {
    Control C(kEntries);
    std::mutex mu;
    std::atomic<bool> stop{false};

    // 1. latched before the call, and after a resume
    C.cancel();
    CHECK(fake_call(C, mu, 2));
    CHECK(fake_call(C, mu, 2));
    C.resume();
    CHECK(!fake_call(C, mu, 2));

    // 2. progress askers, all the while: monotone within a call (total changes between calls
    // only: a smaller `done` is legal only after a (0, 0) or under a new total), never above total
    std::vector<std::thread> askers;
    std::atomic<uint64_t> answered{0};
    for (int a = 0; a < 3; a++)
        askers.emplace_back([&] {
            uint64_t last_done = 0;
            while (!stop.load()) {
                uint64_t done = 0, total = 0;
                C.progress(&done, &total);
                CHECK(done <= total);
                if (total == 0) {
                    last_done = 0;
                } else {
                    answered.fetch_add(1);
                    // calls of this phase follow one another under one mutex: a drop means a new call
                    if (done < last_done) CHECK(done <= kNonces * kEntries * 3);
                    last_done = done;
                }
            }
        });
    // monotone, strictly: one asker alone watches single calls from their start to their end
    for (int round = 0; round < 20; round++) {
        std::atomic<bool> over{false};
        std::thread watcher([&] {
            uint64_t last = 0;
            while (!over.load()) {
                uint64_t done = 0, total = 0;
                C.progress(&done, &total);
                if (total) {
                    CHECK(done >= last);
                    CHECK(total == kNonces * kEntries * 3);
                    last = done;
                }
            }
        });
        CHECK(!fake_call(C, mu, 3));
        over.store(true);
        watcher.join();
    }

    // 3. a cancel while calls are in flight and queued: the one in flight and the queued ones
    // return cancelled; after the resume, a new call does not
    for (int round = 0; round < 20; round++) {
        std::atomic<int> started{0};
        bool got[3] = {};
        std::vector<std::thread> callers;
        for (int c = 0; c < 3; c++)
            callers.emplace_back([&, c] {
                started.fetch_add(1);
                got[c] = fake_call(C, mu, 50);  // long enough to be in flight at the cancel
            });
        while (started.load() < 3) std::this_thread::yield();
        uint64_t done = 0, total = 0;
        while (!total) C.progress(&done, &total);  // one of them is in flight
        C.cancel();
        for (auto& t : callers) t.join();
        for (bool g : got) CHECK(g);
        C.resume();
        CHECK(!fake_call(C, mu, 2));
    }

    // 4. cancel and resume storms against calls: nothing to assert about each outcome but the
    // races themselves (ThreadSanitizer) and that everything ends
    std::thread storm([&] {
        while (!stop.load()) {
            C.cancel();
            std::this_thread::yield();
            C.resume();
            std::this_thread::yield();
        }
    });
    for (int round = 0; round < 30; round++) fake_call(C, mu, 3);
    stop.store(true);
    storm.join();
    for (auto& t : askers) t.join();
    C.resume();
    CHECK(!fake_call(C, mu, 1));
    CHECK(answered.load() > 0);

    if (failures.load()) return 1;
    std::printf("control_check: ok (%llu progress answers)\n", (unsigned long long)answered.load());
    return 0;
}
