// C ABI of the text-corpus language model (include/aprilx_engine.h "language model").  Kept apart from
// april_api.cc, as bias.cc and search_options_api.cc are: the scheduler harness (tests/sched_harness) builds april_api.cc and session.cc
// host-only against a fake engine; what they need of a model is inline in lm.h.  The builder itself is lm.cc.
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../../include/april_api.h"
#include "../../include/aprilx_engine.h"
#include "bias.h"
#include "lm.h"
#include "common.h"
#include "session.h"
#include "api_handles.h"

using namespace aprilx;

namespace {

static_assert(kLmMaxVocab == kBiasMaxVocab, "the LM forms use the biased forms' LDS table");

void put_err(char *err, size_t cap, const std::string &e)
{
    if (!err || !cap) return;
    strncpy(err, e.c_str(), cap - 1);
    err[cap - 1] = 0;
}

// the accepted values; the message names the one that is not
const char *bad_options(float w, float b)
{
    if (!std::isfinite(w) || w < 0.0f || w > kLmMaxWeight) return "the language-model weight must be finite and 0 <= w <= 10";
    if (!std::isfinite(b) || std::fabs(b) > kLmMaxTokenBonus) return "the per-token bonus must be finite and |b| <= 100";
    return nullptr;
}

bool fits(const LmSet &lm, const ModelParams &p) { return lm.vocab == p.token_count && lm.blank == p.blank_id && lm.vocab_hash == bias_vocab_hash(p); }

}  // namespace

extern "C" {

AprilxLm aprilx_lm_create(AprilASRModel model, const void *text, size_t text_len, int order, char *err, size_t err_cap)
{
    put_err(err, err_cap, "");
    if (!model) { put_err(err, err_cap, "no model"); return nullptr; }
    const ModelParams &P = model->m.host.params;
    std::vector<std::string> tokens((size_t)P.token_count);
    for (int i = 0; i < P.token_count; ++i) tokens[(size_t)i] = P.token((size_t)i);
    std::string e;
    std::shared_ptr<LmSet> lm = lm_build(tokens, P.blank_id, bias_vocab_hash(P), text, text_len, order, e);
    put_err(err, err_cap, e);
    if (!lm) return nullptr;
    AprilxLm_i *h = new AprilxLm_i();
    h->lm = lm;
    return h;
}

void aprilx_lm_free(AprilxLm lm) { delete lm; }

int aprilx_lm_info(AprilxLm lm, int32_t *order, int32_t *nodes, int64_t *arcs, int32_t *start, int32_t *alphabet)
{
    if (!lm) return -1;
    const LmSet &m = *lm->lm;
    if (order) *order = m.order;
    if (nodes) *nodes = m.nodes();
    if (arcs) *arcs = m.arcs();
    if (start) *start = m.start;
    if (alphabet) *alphabet = m.alphabet;
    return m.dropped;
}

int aprilx_lm_arrays(AprilxLm lm, int32_t *node_off, int32_t *back, float *bow, uint8_t *arc_byte, float *arc_logp, int32_t *arc_next, float *unk_logp,
                     size_t node_cap, size_t arc_cap)
{
    if (!lm) return -1;
    const LmSet &m = *lm->lm;
    const size_t nn = (size_t)m.nodes(), na = (size_t)m.arcs();
    if ((node_off || back || bow) && node_cap < nn) return -1;
    if ((arc_byte || arc_logp || arc_next) && arc_cap < na) return -1;
    if (node_off) memcpy(node_off, m.node_off.data(), (nn + 1) * 4);      // (nodes + 1 entries: the caller's array holds node_cap + 1)
    if (back) memcpy(back, m.back.data(), nn * 4);
    if (bow) memcpy(bow, m.bow.data(), nn * 4);
    if (arc_byte && na) memcpy(arc_byte, m.arc_byte.data(), na);
    if (arc_logp && na) memcpy(arc_logp, m.arc_logp.data(), na * 4);
    if (arc_next && na) memcpy(arc_next, m.arc_next.data(), na * 4);
    if (unk_logp) *unk_logp = m.unk_logp;
    return 0;
}

int aprilx_lm_score_host(AprilxLm lm, int32_t state, int32_t tok, float *score, int32_t *next)
{
    if (!lm) return -1;
    const LmSet &m = *lm->lm;
    if (state < 0 || state >= m.nodes() || tok < 0 || tok >= m.vocab) return -1;
    float acc = 0.0f;
    const int s = m.score(state, tok, &acc);
    if (score) *score = acc;
    if (next) *next = s;
    return 0;
}

int aprilx_session_set_lm(AprilASRSession session, AprilxLm lm, float weight, float token_bonus)
{
    if (!session) return -1;
    Session *s = &session->s;
    std::shared_ptr<const LmSet> set = lm ? lm->lm : nullptr;
    if (set) {
        if (const char *why = bad_options(weight, token_bonus)) { LOGW("aprilx_session_set_lm: refused: %s", why); return -1; }
        if (!fits(*set, s->model->host.params)) { LOGW("aprilx_session_set_lm: refused: the language model was built for another token list"); return -1; }
    }
    if (!s->sched->set_lm(s, set, weight, token_bonus)) {
        LOGW("aprilx_session_set_lm: refused: the session has audio queued or fed since its creation / last completed flush, or the engine already holds %d other language models", kLmModels);
        return -1;
    }
    return 0;
}

int aprilx_session_lm_state(AprilASRSession session, int32_t *host_state, int32_t *device_state)
{
    if (!session) return -1;
    Session *s = &session->s;
    s->sched->wait_idle(s);
    if (host_state) *host_state = s->greedy.lm_state();
    if (device_state) *device_state = s->eng->read_lm_state(s->slot);
    return s->greedy.lm() ? 1 : 0;
}

int aprilx_greedy_set_lm(AprilxGreedy g, AprilxLm lm, float weight, float token_bonus)
{
    if (!g) return -1;
    if (lm) if (const char *why = bad_options(weight, token_bonus)) { LOGW("aprilx_greedy_set_lm: refused: %s", why); return -1; }
    g->g.set_lm(lm ? lm->lm : nullptr, weight, token_bonus);
    return 0;
}

int aprilx_greedy_lm_state(AprilxGreedy g) { return g ? g->g.lm_state() : -1; }

int aprilx_model_lm_stats(AprilASRModel model, int device_index, uint64_t *launches, int32_t *resident, uint64_t *uploads)
{
    if (!model || device_index < 0 || device_index >= (int)model->m.engines.size() || !launches || !resident || !uploads) return -1;
    model->m.engines[(size_t)device_index]->lm_counts(launches, resident, uploads);
    return 0;
}

int aprilx_run_decide_lm(AprilASRModel model, int n, int op, const float *logits, float early_emit, const int32_t *now_ms, int round, int32_t *state_io,
                         void *records_out, AprilxBias bias, int32_t *bias_state_io, const AprilxSearchOptions *opts, AprilxLm lm, int32_t *lm_state_io,
                         float weight, float token_bonus)
{
    if (!model || n <= 0 || model->m.engines.empty() || n > model->m.engines[0]->max_slots() || !state_io || !lm || !lm_state_io) return -1;
    if (op == 0 && (!logits || !now_ms || !records_out || round < 0 || round > 2)) return -1;
    const ModelParams &P = model->m.host.params;
    if (bad_options(weight, token_bonus) || !fits(*lm->lm, P)) return -1;
    for (int i = 0; i < n; ++i) if (lm_state_io[i] < -1 || lm_state_io[i] >= lm->lm->nodes()) return -1;
    if (bias) {
        if (!bias_state_io || bias->set->vocab != P.token_count || bias->set->vocab_hash != bias_vocab_hash(P)) return -1;
        for (int i = 0; i < n; ++i) if (bias_state_io[i] < -1 || bias_state_io[i] >= bias->set->states()) return -1;
    }
    std::vector<SearchOpt> so;
    if (opts) {
        so.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            if (opts[i].size == 0) { so[(size_t)i] = SearchOpt{0u, 0.0f}; continue; }
            const AprilxSearchOptions &o = opts[i];      // (the accepted values of section 14, as aprilx_run_decide_opts checks them)
            if (o.size != (uint32_t)sizeof o || o.endpoint_silence_ms < 200u || o.endpoint_silence_ms > 60000u) return -1;
            if (o.max_utterance_ms != 0u && (o.max_utterance_ms < 1000u || o.max_utterance_ms > 600000u)) return -1;
            if (!std::isfinite(o.blank_penalty) || std::fabs(o.blank_penalty) > 100.0f) return -1;
            so[(size_t)i] = SearchOpt{o.endpoint_silence_ms, o.blank_penalty};
        }
    }
    DecideRequest q = DecideRequest::round_of(n, op, logits, early_emit, now_ms, round, state_io, records_out);
    if (bias) { q.set = bias->set.get(); q.bias_state_io = bias_state_io; }
    if (opts) q.opts = so.data();
    q.lm = lm->lm.get(); q.lm_state_io = lm_state_io; q.lm_weight = weight; q.lm_bonus = token_bonus;
    model->m.engines[0]->debug_decide(q);
    return 0;
}

int aprilx_run_confidence_lm(AprilASRModel model, int n, const float *logits, int k, AprilxBias bias, const int32_t *bias_state, AprilxLm lm,
                             const int32_t *lm_state, float weight, float token_bonus, AprilxTokenInfo *out)
{
    if (!model || n <= 0 || model->m.engines.empty() || n > model->m.engines[0]->max_slots() || n > model->m.engines[0]->max_batch()) return -1;
    if (!logits || !out || k < 1 || k > kConfMaxAlt || !lm || !lm_state) return -1;
    const ModelParams &P = model->m.host.params;
    if (bad_options(weight, token_bonus) || !fits(*lm->lm, P)) return -1;
    for (int i = 0; i < n; ++i) if (lm_state[i] < -1 || lm_state[i] >= lm->lm->nodes()) return -1;
    if (bias) {
        if (!bias_state || bias->set->vocab != P.token_count || bias->set->vocab_hash != bias_vocab_hash(P)) return -1;
        for (int i = 0; i < n; ++i) if (bias_state[i] < -1 || bias_state[i] >= bias->set->states()) return -1;
    }
    std::vector<ConfRecord> rec((size_t)n);
    std::vector<int32_t> trie(bias ? bias_state : lm_state, (bias ? bias_state : lm_state) + n), node(lm_state, lm_state + n);      // (the request's states are in/out)
    DecideRequest q;
    q.n = n; q.logits = logits; q.conf_k = k; q.conf_out = rec.data();
    if (bias) { q.set = bias->set.get(); q.bias_state_io = trie.data(); }
    q.lm = lm->lm.get(); q.lm_state_io = node.data(); q.lm_weight = weight; q.lm_bonus = token_bonus;
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

}  // extern "C"
