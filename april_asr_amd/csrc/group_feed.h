// Group calls of the C ABI, stated once for april_api.cc (aprilx_feed_many, aprilx_feed_many_pipelined, drain, flush) and
// input_format_api.cc (aprilx_feed_many_bytes): the listed sessions by scheduler (GPU), in the order of the list, with their audio
// when the call carries some.  Include behind the definition of AprilASRSession_i.  Header-only: the scheduler harness
// (tests/sched_harness) builds april_api.cc without further files.
#pragma once
#include <algorithm>
#include <vector>
#include "session.h"

namespace aprilx {

struct SchedGroup { Scheduler *sched; std::vector<Session *> ss; std::vector<const short *> pcm; std::vector<size_t> counts; };

inline std::vector<SchedGroup> group_by_scheduler(size_t n, AprilASRSession *sessions, const short *const *pcm16, const size_t *counts)
{
    std::vector<SchedGroup> groups;
    for (size_t i = 0; i < n; ++i) {
        Session *s = &sessions[i]->s;
        auto g = std::find_if(groups.begin(), groups.end(), [&](const SchedGroup &x) { return x.sched == s->sched; });
        if (g == groups.end()) { groups.emplace_back(); g = groups.end() - 1; g->sched = s->sched; }
        g->ss.push_back(s);
        if (pcm16) { g->pcm.push_back(pcm16[i]); g->counts.push_back(counts[i]); }
    }
    return groups;
}

inline void deliver_sync_events_all(size_t n, AprilASRSession *sessions)
{
    for (size_t i = 0; i < n; ++i) if (sessions[i]->s.sync_mode) sessions[i]->s.sched->deliver_sync_events(&sessions[i]->s);
}

// a group feed: each scheduler's sessions are submitted at once so that they step together; every GPU is queued first (no wait),
// then `wait` runs per group, so the GPUs work concurrently.  `bytes`: the counts are bytes (Scheduler::submit); false when a
// scheduler refused its sessions' counts (a partial frame: the caller has checked every count before, so that no GPU is queued then)
template <class Wait> bool feed_groups(size_t n, AprilASRSession *sessions, const short *const *pcm16, const size_t *counts, bool borrow, bool bytes, Wait wait)
{
    std::vector<SchedGroup> groups = group_by_scheduler(n, sessions, pcm16, counts);
    bool ok = true;
    for (SchedGroup &g : groups) ok = g.sched->submit((int)g.ss.size(), g.ss.data(), g.pcm.data(), g.counts.data(), false, false, borrow, bytes) && ok;
    for (SchedGroup &g : groups) wait(g);
    deliver_sync_events_all(n, sessions);
    return ok;
}

}  // namespace aprilx
