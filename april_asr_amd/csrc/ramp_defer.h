// Ramp merge, the host's bookkeeping of a deferred layer graph ("deferred enqueue").  Pure: no HIP, no
// threads -- the engine calls it under its own lock (engine.cc, settle_pending_layers), tests/cpp/ramp_defer_test.cc drives it alone.
//
// A split feed that is offered to a hosting layer chain in front of it has only its front end and its ready kernel enqueued; which
// layer graph follows -- the one with the head steps or the headless one -- is the DEVICE's decision, made once by that chain's latch
// kernel, which reports it in one 8-byte word in pinned host memory: ramp_outcome_word(generation the latch looked for, hosted).
// The host only reads that word.  A feed's generation is its rank among the engine's ready-kernel launches (1, 2, ...), which the
// host counts as the device does; the latch of the chain in front looks for exactly the deferred feed's generation, so a word of any
// other generation (an older latch's, or the zero the word starts with) is not an answer yet.
#pragma once
#include <cstdint>

namespace aprilx {

inline uint64_t ramp_outcome_word(uint32_t generation, bool hosted) { return ((uint64_t)generation << 32) | (hosted ? 1u : 0u); }

struct RampDefer {
    enum Flavour { WITH_HEAD = 0, HEADLESS = 1 };
    enum Who { BY_WAIT = 0, BY_OTHER = 1 };           // settled by wait_flight / flight_done, or by any other entry (the launch itself included)

    bool pending() const { return pending_; }
    uint32_t wanted() const { return want_; }
    uint64_t deferred = 0, headless = 0, settled_by[2] = {0, 0};

    // A split feed of generation `gen` is launched.  latch_in_front: the feed was offered and the last thing on the layer stream is a
    // chain with a latch.  Without one nothing is deferred: enqueue(WITH_HEAD) runs at once.  With one the feed waits for the word of
    // its generation, and `word_now` is looked at right away (the latch may have run already: a late host).  Returns true while pending.
    template <typename Enqueue> bool launch(uint32_t gen, bool latch_in_front, uint64_t word_now, Enqueue &&enqueue)
    {
        if (pending_) return true;                    // (the caller settles first: a second deferral never stacks on an open one)
        if (!latch_in_front) { enqueue(WITH_HEAD); return false; }
        pending_ = true; want_ = gen; ++deferred;
        return !poll(word_now, BY_OTHER, enqueue);
    }

    // Looks at the word once.  Returns true when nothing is pending after the call (the enqueue ran now, or nothing was deferred).
    template <typename Enqueue> bool poll(uint64_t word_now, Who who, Enqueue &&enqueue)
    {
        if (!pending_) return true;
        if ((uint32_t)(word_now >> 32) != want_) return false;
        pending_ = false;                             // (first: the enqueue runs exactly once even if it looks at this state)
        const Flavour f = (word_now & 1u) ? HEADLESS : WITH_HEAD;
        if (f == HEADLESS) ++headless;
        ++settled_by[who];
        enqueue(f);
        return true;
    }

private:
    bool pending_ = false;
    uint32_t want_ = 0;
};

}  // namespace aprilx
