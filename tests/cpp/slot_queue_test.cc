// Stand-alone check of csrc/slot_queue.h under AddressSanitizer + UBSan and under ThreadSanitizer (tests/test_slot_queue_cpu.py builds
// and runs it): four pusher threads and one taker on a table of 8 slots, as the client threads and the stepping thread use the queue.
//   * every pushed value is taken exactly once, and each slot's values arrive in push order (a slot belongs to one pusher);
//   * OFF values pushed before any ON value are dropped and never seen; "ever" stays set once set;
//   * the pending-slot query is true from the push until the take;
//   * push_locked() under mutex() keeps a caller's own books and the queue in one critical section.
#include <atomic>
#include <cstdio>
#include <mutex>
#include <thread>
#include <vector>
#include "slot_queue.h"

using namespace aprilx;

static std::atomic<int> fails{0};
#define CHECK(c) do { if (!(c)) { if (fails.fetch_add(1) < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

static void single_thread()
{
    SlotQueue<int> q;
    CHECK(!q.ever() && !q.has_pending());
    CHECK(!q.push(3, 0, false));                        // off while nothing was ever on: dropped
    CHECK(!q.ever() && !q.has_pending() && !q.pending(3) && q.take().empty());
    CHECK(q.push(3, 7, true));
    CHECK(q.ever() && q.has_pending() && q.pending(3) && !q.pending(2));
    CHECK(q.push(2, 0, false));                         // off after an on value: queued
    CHECK(q.push(-1, 5, true) && q.push(99, 5, true));  // (out-of-range slots are the taker's to ignore)
    const auto got = q.take();
    CHECK(got.size() == 4 && got[0] == std::make_pair(3, 7) && got[1] == std::make_pair(2, 0) && got[2].first == -1 && got[3].first == 99);
    CHECK(q.ever() && !q.has_pending() && !q.pending(3) && q.take().empty());
    CHECK(q.push(3, 0, false) && q.pending(3));         // "ever" stays
    {
        std::lock_guard<std::mutex> g(q.mutex());
        CHECK(q.pending_locked(3) && q.push_locked(4, 1, true) && q.pending_locked(4));
        CHECK(q.take_locked().size() == 2 && !q.pending_locked(4));
    }
    CHECK(q.ever() && !q.has_pending());
}

static void threads()
{
    constexpr int kSlots = 8, kPushers = 4, kPerSlot = 400;      // 3200 pushes, plus the leading OFF values
    SlotQueue<int> q;
    std::vector<int> books(kSlots, 0);                  // a caller's own state under q.mutex(): the last value pushed for each slot
    std::atomic<int> done{0};
    std::atomic<bool> ever_seen{false}, ever_lost{false};
    std::vector<std::thread> pushers;
    for (int t = 0; t < kPushers; ++t)
        pushers.emplace_back([&, t]() {
            for (int s = t; s < kSlots; s += kPushers) { const bool queued = q.push(s, -1000 - s, false); CHECK(!queued || q.ever()); }      // early OFF values: dropped unless another thread's ON value came first
            for (int i = 1; i <= kPerSlot; ++i)
                for (int s = t; s < kSlots; s += kPushers) {          // slots t and t + 4 are this thread's
                    const int v = s * 100000 + i;
                    if (i % 3 == 0) {                                 // books and push in one critical section
                        std::lock_guard<std::mutex> g(q.mutex());
                        books[(size_t)s] = v;
                        CHECK(q.push_locked(s, v, true) && q.pending_locked(s));
                    } else {
                        CHECK(q.push(s, v, i % 2 == 1));              // (an OFF value after this thread's first ON value: queued)
                    }
                    if (q.ever()) ever_seen.store(true); else if (ever_seen.load()) ever_lost.store(true);
                }
            done.fetch_add(1);
        });
    std::vector<int> last(kSlots, 0);
    std::vector<int> count(kSlots, 0);
    long taken = 0;
    auto drain = [&]() {
        std::vector<std::pair<int, int>> got;
        if (taken % 2) {
            std::lock_guard<std::mutex> g(q.mutex());
            for (int s = 0; s < kSlots; ++s) if (q.pending_locked(s)) CHECK(books[(size_t)s] >= 0);
            got = q.take_locked();
            for (int s = 0; s < kSlots; ++s) CHECK(!q.pending_locked(s));      // true from the push until the take, not longer
        } else got = q.take();
        for (const auto &it : got) {
            const int s = it.first, v = it.second;
            CHECK(s >= 0 && s < kSlots);
            if (s < 0 || s >= kSlots) continue;
            if (v < 0) { CHECK(v == -1000 - s && count[(size_t)s] == 0); continue; }       // an early OFF value that was not dropped came after another slot's ON value, before its own slot's values
            CHECK(v / 100000 == s && v % 100000 == last[(size_t)s] + 1);                  // exactly once, in push order
            last[(size_t)s] = v % 100000; ++count[(size_t)s];
        }
        ++taken;
    };
    while (done.load() < kPushers) { if (q.has_pending()) drain(); else std::this_thread::yield(); }
    for (auto &t : pushers) t.join();
    drain(); drain();
    for (int s = 0; s < kSlots; ++s) CHECK(count[(size_t)s] == kPerSlot && last[(size_t)s] == kPerSlot);
    CHECK(q.ever() && !q.has_pending() && !ever_lost.load());

    // OFF values pushed before ANY on value, from all four threads at once: never seen
    SlotQueue<int> off;
    std::vector<std::thread> offs;
    for (int t = 0; t < kPushers; ++t) offs.emplace_back([&off, t]() { for (int i = 0; i < 200; ++i) CHECK(!off.push((t + i) % kSlots, 0, false)); });
    for (int i = 0; i < 50; ++i) CHECK(off.take().empty() && !off.has_pending());
    for (auto &t : offs) t.join();
    CHECK(off.take().empty() && !off.ever() && !off.has_pending());
}

int main()
{
    single_thread();
    threads();
    if (fails.load()) { printf("%d checks FAILED\n", fails.load()); return 1; }
    printf("all checks passed\n");
    return 0;
}
