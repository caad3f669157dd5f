// Changes of one per-slot opt-in table (confidences, bias sets, search options: DESIGN.md sections 12-14) on their way from the client
// threads to the stepping thread.  Any thread pushes (slot, value) for an idle session's slot; the stepping thread takes everything at
// the start of a flight (Engine::apply_slot_tables).  One rule for every table: an OFF value is dropped while no ON value was ever
// pushed -- an engine where nobody opts in queues nothing, allocates nothing and takes no lock on its hot path.
// No HIP here: tests/cpp/slot_queue_test.cc runs it under the sanitizers as a plain program.
#pragma once
#include <atomic>
#include <mutex>
#include <utility>
#include <vector>

namespace aprilx {

template <typename V> class SlotQueue {
public:
    using Item = std::pair<int, V>;
    // any thread; `on`: the value switches the feature on for its slot.  False: dropped (nothing was ever on)
    bool push(int slot, const V &v, bool on) { std::lock_guard<std::mutex> g(mu_); return push_locked(slot, v, on); }
    // ... for a caller that keeps books of its own under mutex() and pushes in the same critical section
    bool push_locked(int slot, const V &v, bool on)
    {
        if (!on && !ever()) return false;
        items_.emplace_back(slot, v);
        if (on) ever_.store(true, std::memory_order_relaxed);
        has_pending_.store(true, std::memory_order_release);
        return true;
    }
    // stepping thread: everything pushed so far, in push order
    std::vector<Item> take() { std::lock_guard<std::mutex> g(mu_); return take_locked(); }
    std::vector<Item> take_locked()
    {
        std::vector<Item> out;
        out.swap(items_);
        has_pending_.store(false, std::memory_order_release);
        return out;
    }
    // a change of this slot has been pushed and not yet taken (mutex() held)
    bool pending_locked(int slot) const { for (const Item &t : items_) if (t.first == slot) return true; return false; }
    bool pending(int slot) { std::lock_guard<std::mutex> g(mu_); return pending_locked(slot); }
    bool has_pending() const { return has_pending_.load(std::memory_order_acquire); }      // the hot path's only look at the queue
    bool ever() const { return ever_.load(std::memory_order_relaxed); }                    // some ON value has been pushed; never cleared
    std::mutex &mutex() { return mu_; }

private:
    std::mutex mu_;
    std::vector<Item> items_;
    std::atomic<bool> has_pending_{false}, ever_{false};
};

}  // namespace aprilx
