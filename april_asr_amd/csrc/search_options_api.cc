// C ABI of the per-session search options (include/aprilx_engine.h "search options").  Kept apart from
// april_api.cc, as resample_api.cc and confidence_api.cc are: the scheduler harness (tests/sched_harness) builds april_api.cc host-only
// against a fake engine, and aprilx_run_decide_opts calls engine code that is not inline.
#include <cmath>
#include <memory>
#include <vector>
#include "../../include/april_api.h"
#include "../../include/aprilx_engine.h"
#include "bias.h"
#include "common.h"
#include "session.h"
#include "api_handles.h"

using namespace aprilx;

namespace {

// the accepted values
bool valid(const AprilxSearchOptions &o)
{
    if (o.size != (uint32_t)sizeof(AprilxSearchOptions)) return false;
    if (o.endpoint_silence_ms < 200u || o.endpoint_silence_ms > 60000u) return false;
    if (o.max_utterance_ms != 0u && (o.max_utterance_ms < 1000u || o.max_utterance_ms > 600000u)) return false;
    return std::isfinite(o.blank_penalty) && std::fabs(o.blank_penalty) <= 100.0f;
}

}  // namespace

extern "C" {

int aprilx_session_set_search_options(AprilASRSession session, const AprilxSearchOptions *options)
{
    if (!session || (options && !valid(*options))) return -1;
    Session *s = &session->s;
    return s->sched->set_search_options(s, options) ? 0 : -1;
}

int aprilx_session_search_options(AprilASRSession session, AprilxSearchOptions *out)
{
    if (!session || !out) return -1;
    Session *s = &session->s;
    // no wait (as aas_realtime_get_speedup): the values change only in aprilx_session_set_search_options, on an idle session
    *out = s->greedy.search_options();
    return s->greedy.has_search_options() ? 1 : 0;
}

int aprilx_run_decide_opts(AprilASRModel model, int n, int op, const float *logits, float early_emit, const int32_t *now_ms, int round,
                           int32_t *state_io, void *records_out, AprilxBias bias, int32_t *bias_state_io, const AprilxSearchOptions *opts)
{
    if (!model || n <= 0 || model->m.engines.empty() || n > model->m.engines[0]->max_slots() || !state_io || !opts) return -1;
    if (op == 0 && (!logits || !now_ms || !records_out || round < 0 || round > 2)) return -1;
    if (bias) {
        if (!bias_state_io || bias->set->vocab != model->m.host.params.token_count || bias->set->vocab_hash != bias_vocab_hash(model->m.host.params)) return -1;
        for (int i = 0; i < n; ++i) if (bias_state_io[i] < -1 || bias_state_io[i] >= bias->set->states()) return -1;
    }
    std::vector<SearchOpt> so((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (opts[i].size == 0) { so[(size_t)i] = SearchOpt{0u, 0.0f}; continue; }
        if (!valid(opts[i])) return -1;
        so[(size_t)i] = SearchOpt{opts[i].endpoint_silence_ms, opts[i].blank_penalty};
    }
    DecideRequest q = DecideRequest::round_of(n, op, logits, early_emit, now_ms, round, state_io, records_out);
    if (bias) { q.set = bias->set.get(); q.bias_state_io = bias_state_io; }
    q.opts = so.data();
    model->m.engines[0]->debug_decide(q);
    return 0;
}

int aprilx_greedy_set_search_options(AprilxGreedy g, const AprilxSearchOptions *options)
{
    if (!g || (options && !valid(*options))) return -1;
    g->g.set_search_options(options);
    return 0;
}

}  // extern "C"
