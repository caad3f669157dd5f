// C ABI of the per-token confidences (include/aprilx_engine.h "per-token confidence and alternatives").
// Kept apart from april_api.cc, as resample_api.cc is: the scheduler harness (tests/sched_harness) builds april_api.cc host-only
// against a fake engine, and aprilx_run_confidence calls engine code that is not inline.
#include <cstring>
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

int run_confidence(AprilASRModel model, int n, const float *logits, int k, AprilxTokenInfo *out, const BiasSet *set, const int32_t *bias_state)
{
    if (!model || n <= 0 || model->m.engines.empty() || n > model->m.engines[0]->max_slots() || n > model->m.engines[0]->max_batch()) return -1;
    if (!logits || !out || k < 1 || k > kConfMaxAlt) return -1;
    std::vector<ConfRecord> rec((size_t)n);
    std::vector<int32_t> trie(bias_state, bias_state + (set ? n : 0));      // (the request's states are in/out)
    DecideRequest q;
    q.n = n; q.logits = logits; q.conf_k = k; q.conf_out = rec.data(); q.set = set; q.bias_state_io = trie.data();
    model->m.engines[0]->debug_decide(q);
    // the same conversion a live session's tokens get (Greedy::fill_info)
    for (int i = 0; i < n; ++i) {
        const ConfRecord &c = rec[(size_t)i];
        AprilxTokenInfo &o = out[i];
        memset(&o, 0, sizeof o);
        o.size = (uint32_t)sizeof(AprilxTokenInfo);
        o.eval_index = (uint64_t)i;
        o.n_alt = (uint32_t)(c.n_alt < 0 ? 0 : (c.n_alt > k ? k : c.n_alt));
        o.lse = c.lse;
        o.token_logprob = o.n_alt ? c.alt_logit[0] - c.lse : __builtin_nanf("");
        o.blank_logprob = c.blank_val - c.lse;
        for (int j = 0; j < 8; ++j) o.alt_id[j] = -1;
        for (uint32_t j = 0; j < o.n_alt; ++j) { o.alt_id[j] = c.alt_id[j]; o.alt_logit[j] = c.alt_logit[j]; }
    }
    return 0;
}

}  // namespace

extern "C" {

int aprilx_session_set_confidence(AprilASRSession session, int n_alternatives)
{
    if (!session || n_alternatives < 0 || n_alternatives > kConfMaxAlt) return -1;
    Session *s = &session->s;
    return s->sched->set_confidence(s, n_alternatives) ? 0 : -1;
}

int aprilx_session_confidence(AprilASRSession session)
{
    if (!session) return 0;
    Session *s = &session->s;
    s->sched->wait_idle(s);
    return s->greedy.confidence();
}

int aprilx_run_confidence(AprilASRModel model, int n, const float *logits, int k, AprilxTokenInfo *out)
{
    return run_confidence(model, n, logits, k, out, nullptr, nullptr);
}

int aprilx_run_confidence_biased(AprilASRModel model, int n, const float *logits, int k, AprilxBias bias, const int32_t *bias_state, AprilxTokenInfo *out)
{
    if (!model || !bias || !bias_state || n <= 0) return -1;
    if (bias->set->vocab != model->m.host.params.token_count || bias->set->vocab_hash != bias_vocab_hash(model->m.host.params)) return -1;
    for (int i = 0; i < n; ++i) if (bias_state[i] < -1 || bias_state[i] >= bias->set->states()) return -1;
    return run_confidence(model, n, logits, k, out, bias->set.get(), bias_state);
}

}  // extern "C"
