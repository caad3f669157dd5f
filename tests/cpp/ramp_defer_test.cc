// Stand-alone check of csrc/ramp_defer.h, the host's bookkeeping of a deferred layer graph (tests/test_ramp_defer_cpu.py
// builds and runs it, once plain and once under AddressSanitizer + UBSan).  The engine is replaced by a script: a list of layer graphs
// "enqueued", in order, and an outcome word the script sets where the latch kernel would store it.
//   * every launched feed is enqueued exactly once, in launch order, with the flavour the word of ITS generation names;
//   * a word of another generation (older latch, the initial zero, a far newer one) is never taken for an answer;
//   * without a latch in front nothing is deferred; with one nothing is enqueued before the word is there;
//   * the counters say who settled.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>
#include "ramp_defer.h"

using namespace aprilx;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails++ < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

struct Script {
    RampDefer d;
    uint64_t word = 0;                                      // the pinned word
    uint32_t gen = 0;                                       // ready kernels launched
    std::vector<std::pair<uint32_t, int>> enq;              // (generation, flavour) of every layer graph enqueued
    uint32_t open_gen = 0;
    bool launch(bool latch_in_front)
    {
        const uint32_t g = ++gen;
        open_gen = g;
        return d.launch(g, latch_in_front, word, [&](RampDefer::Flavour f) { enq.emplace_back(g, (int)f); });
    }
    bool poll(RampDefer::Who who)
    {
        const uint32_t g = open_gen;
        return d.poll(word, who, [&](RampDefer::Flavour f) { enq.emplace_back(g, (int)f); });
    }
    // what every other engine entry does: poll until the word is there (the script's latch "runs" after `after` polls)
    void force(uint64_t outcome, int after)
    {
        for (int i = 0; !poll(RampDefer::BY_OTHER); ++i) { CHECK(i <= after); if (i == after) word = outcome; }
    }
};

static void hosted_before_the_poll()
{
    Script s;
    CHECK(!s.launch(false) && s.enq.size() == 1 && s.enq[0] == std::make_pair(1u, (int)RampDefer::WITH_HEAD));      // feed 1: nothing in front
    CHECK(s.launch(true) && s.d.pending() && s.d.wanted() == 2 && s.enq.size() == 1);                                // feed 2: deferred
    s.word = ramp_outcome_word(2, true);                                                                             // feed 1's latch hosts it
    CHECK(s.poll(RampDefer::BY_WAIT) && !s.d.pending());
    CHECK(s.enq.size() == 2 && s.enq[1] == std::make_pair(2u, (int)RampDefer::HEADLESS));
    CHECK(s.poll(RampDefer::BY_WAIT) && s.poll(RampDefer::BY_OTHER) && s.enq.size() == 2);                           // never twice
    CHECK(s.d.deferred == 1 && s.d.headless == 1 && s.d.settled_by[RampDefer::BY_WAIT] == 1 && s.d.settled_by[RampDefer::BY_OTHER] == 0);
}

static void not_hosted()
{
    Script s;
    s.launch(false);
    CHECK(s.launch(true));
    CHECK(!s.poll(RampDefer::BY_WAIT) && !s.poll(RampDefer::BY_WAIT) && s.enq.size() == 1);                          // the latch has not run: nothing yet
    s.word = ramp_outcome_word(2, false);
    CHECK(s.poll(RampDefer::BY_WAIT) && s.enq.size() == 2 && s.enq[1] == std::make_pair(2u, (int)RampDefer::WITH_HEAD));
    CHECK(s.d.headless == 0 && s.d.settled_by[RampDefer::BY_WAIT] == 1);
}

static void another_entry_forces_it()
{
    Script s;
    s.launch(false);
    CHECK(s.launch(true));
    CHECK(!s.poll(RampDefer::BY_WAIT));
    s.force(ramp_outcome_word(2, true), 5);                 // e.g. a slot reset: polls until the latch has run
    CHECK(!s.d.pending() && s.enq.size() == 2 && s.enq[1] == std::make_pair(2u, (int)RampDefer::HEADLESS));
    CHECK(s.d.settled_by[RampDefer::BY_OTHER] == 1 && s.d.settled_by[RampDefer::BY_WAIT] == 0 && s.d.headless == 1);
    CHECK(s.poll(RampDefer::BY_WAIT) && s.enq.size() == 2);
}

static void no_hosting_chain_in_front()
{
    Script s;
    s.word = ramp_outcome_word(1, true);                    // whatever the word holds: nobody asked
    CHECK(!s.launch(false) && !s.d.pending() && s.enq.size() == 1 && s.enq[0].second == RampDefer::WITH_HEAD);
    CHECK(!s.launch(false) && s.enq.size() == 2 && s.enq[1] == std::make_pair(2u, (int)RampDefer::WITH_HEAD));
    CHECK(s.d.deferred == 0 && s.d.headless == 0 && s.d.settled_by[0] == 0 && s.d.settled_by[1] == 0);
}

static void two_feeds_in_a_row()
{
    Script s;
    s.launch(false);                                        // 1
    CHECK(s.launch(true));                                  // 2 deferred behind 1
    s.word = ramp_outcome_word(2, true);
    CHECK(s.poll(RampDefer::BY_WAIT));
    CHECK(s.launch(true) && s.d.wanted() == 3);             // 3 deferred behind 2: the word still holds generation 2's answer
    CHECK(!s.poll(RampDefer::BY_WAIT) && s.enq.size() == 2);
    s.word = ramp_outcome_word(3, false);
    CHECK(s.poll(RampDefer::BY_WAIT));
    CHECK(s.launch(true));                                  // 4
    s.word = ramp_outcome_word(4, true);
    CHECK(s.poll(RampDefer::BY_WAIT));
    const std::vector<std::pair<uint32_t, int>> want = {{1u, 0}, {2u, 1}, {3u, 0}, {4u, 1}};
    CHECK(s.enq == want);
    CHECK(s.d.deferred == 3 && s.d.headless == 2 && s.d.settled_by[RampDefer::BY_WAIT] == 3);
}

static void stale_generation_in_the_word()
{
    Script s;
    s.launch(false);
    s.word = ramp_outcome_word(1, true);                    // an older latch's report, "hosted"
    CHECK(s.launch(true) && s.d.pending() && s.enq.size() == 1);                 // not an answer for generation 2, not even at the launch
    CHECK(!s.poll(RampDefer::BY_WAIT));
    s.word = 0;                                             // the word's initial value
    CHECK(!s.poll(RampDefer::BY_WAIT));
    s.word = ramp_outcome_word(0x80000002u, true);          // same low bits, other generation
    CHECK(!s.poll(RampDefer::BY_WAIT) && s.enq.size() == 1);
    s.word = ramp_outcome_word(2, false);
    CHECK(s.poll(RampDefer::BY_WAIT) && s.enq.size() == 2 && s.enq[1] == std::make_pair(2u, (int)RampDefer::WITH_HEAD));
}

static void late_host_sees_the_word_at_the_launch()
{
    Script s;
    s.launch(false);
    s.word = ramp_outcome_word(2, false);                   // feed 1's latch ran before feed 2 was launched: it found nothing, and said so
    CHECK(!s.launch(true) && !s.d.pending());               // offered, deferred, settled in the same call
    CHECK(s.enq.size() == 2 && s.enq[1] == std::make_pair(2u, (int)RampDefer::WITH_HEAD));
    CHECK(s.d.deferred == 1 && s.d.settled_by[RampDefer::BY_OTHER] == 1);
}

static void a_launch_never_stacks()
{
    Script s;
    s.launch(false);
    CHECK(s.launch(true));
    const uint32_t g = s.open_gen;
    CHECK(s.d.launch(99, true, 0, [&](RampDefer::Flavour) { CHECK(false); }) && s.d.wanted() == g && s.d.deferred == 1);      // refused: still pending, untouched
    s.word = ramp_outcome_word(g, true);
    CHECK(s.poll(RampDefer::BY_OTHER) && s.enq.size() == 2);
}

int main()
{
    hosted_before_the_poll();
    not_hosted();
    another_entry_forces_it();
    no_hosting_chain_in_front();
    two_feeds_in_a_row();
    stale_generation_in_the_word();
    late_host_sees_the_word_at_the_launch();
    a_launch_never_stacks();
    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    printf("all checks passed\n");
    return 0;
}
