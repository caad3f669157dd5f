// Phrase boosting (include/aprilx_engine.h "phrase boosting"): the host-side builder of a bias set and the C ABI.
// Kept apart from april_api.cc, as resample_api.cc and confidence_api.cc are: the scheduler harness (tests/sched_harness) builds
// april_api.cc and session.cc host-only against a fake engine; what they need of a set is inline in bias.h.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../../include/april_api.h"
#include "../../include/aprilx_engine.h"
#include "bias.h"
#include "common.h"
#include "session.h"
#include "api_handles.h"

using namespace aprilx;

namespace {

struct TrieNode { int child[256]; float best; TrieNode() : best(0.0f) { for (int &c : child) c = -1; } };

// The text of a token: its bytes in the model's token list up to the NUL.  Tokens with an empty text and the blank have no edges.
struct Vocab {
    std::vector<std::string> text;
    std::vector<std::vector<int>> by_first;    // non-blank, non-empty tokens by their first byte, ids ascending
    Vocab(const ModelParams &p) : by_first(256)
    {
        text.resize((size_t)p.token_count);
        for (int i = 0; i < p.token_count; ++i) {
            text[(size_t)i] = p.token((size_t)i);
            if (i != p.blank_id && !text[(size_t)i].empty()) by_first[(unsigned char)text[(size_t)i][0]].push_back(i);
        }
    }
};

// some sequence of tokens spells exactly `s`
bool spellable(const Vocab &v, const std::string &s)
{
    std::vector<char> reach(s.size() + 1, 0);
    reach[0] = 1;
    for (size_t i = 0; i < s.size(); ++i) {
        if (!reach[i]) continue;
        for (int t : v.by_first[(unsigned char)s[i]]) {
            const std::string &x = v.text[(size_t)t];
            if (i + x.size() <= s.size() && s.compare(i, x.size(), x) == 0) reach[i + x.size()] = 1;
        }
    }
    return reach[s.size()] != 0;
}

struct Edge { int tok, next; float bonus; };

// strict (kBiasStrict): the emitted edges are the tokens PERMITTED at every state -- own edges whose target can still reach the end of
// a phrase, and the root's such edges at the root and where a phrase ends; without the flag the code takes the path it took before
std::shared_ptr<BiasSet> build_set(const ModelParams &P, size_t n, const char *const *phrases, const float *boosts, uint32_t flags, std::string &err)
{
    const bool strict = (flags & kBiasStrict) != 0;
    if (n == 0 || !phrases || !boosts) { err = "a bias set needs at least one phrase"; return nullptr; }
    if (P.token_count > kBiasMaxVocab) { err = "phrase boosting supports vocabularies of at most " + std::to_string(kBiasMaxVocab) + " tokens"; return nullptr; }
    const Vocab voc(P);
    std::vector<TrieNode> trie(1);
    auto set = std::make_shared<BiasSet>();
    set->vocab = P.token_count;
    set->vocab_hash = bias_vocab_hash(P);
    set->flags = flags;
    std::vector<int> ends;                                          // the node where every kept phrase ends
    for (size_t i = 0; i < n; ++i) {
        const std::string where = "phrase " + std::to_string(i);
        if (!phrases[i] || !phrases[i][0]) { err = where + " is empty"; return nullptr; }
        std::string s = phrases[i];
        if (s.size() > (size_t)kBiasMaxPhraseBytes) { err = where + " is longer than " + std::to_string(kBiasMaxPhraseBytes) + " bytes"; return nullptr; }
        const float b = boosts[i];
        if (!std::isfinite(b)) { err = where + ": the boost is not finite"; return nullptr; }
        if (std::fabs(b) > kBiasMaxBoost) { err = where + ": |boost| exceeds " + std::to_string((int)kBiasMaxBoost); return nullptr; }
        if (s[0] != ' ') s.insert(s.begin(), ' ');                 // phrases start at word boundaries
        if (!spellable(voc, s)) { ++set->dropped; continue; }     // reported (aprilx_bias_info, the message), never kept
        int node = 0;
        for (unsigned char c : s) {
            if (trie[(size_t)node].child[c] < 0) {
                if ((int)trie.size() >= kBiasMaxStates) { err = "the phrases need more than " + std::to_string(kBiasMaxStates) + " trie states"; return nullptr; }
                trie[(size_t)node].child[c] = (int)trie.size();
                trie.emplace_back();
                trie.back().best = b;                               // best(node): the largest boost of the phrases through the node
            } else {
                TrieNode &t = trie[(size_t)trie[(size_t)node].child[c]];
                if (b > t.best) t.best = b;
            }
            node = trie[(size_t)node].child[c];
        }
        ends.push_back(node);
    }
    const int S = (int)trie.size();
    std::vector<char> terminal((size_t)S, 0);
    for (int e : ends) terminal[(size_t)e] = 1;
    // own edges of state s: every non-blank token whose whole text can be walked from s, ids ascending
    auto own_edges = [&](int s, std::vector<Edge> &out) {
        out.clear();
        for (int c = 0; c < 256; ++c) {
            if (trie[(size_t)s].child[c] < 0) continue;
            for (int t : voc.by_first[(size_t)c]) {
                int node = s;
                for (unsigned char ch : voc.text[(size_t)t]) { node = trie[(size_t)node].child[ch]; if (node < 0) break; }
                if (node >= 0) out.push_back(Edge{t, node, trie[(size_t)node].best});
            }
        }
        std::sort(out.begin(), out.end(), [](const Edge &a, const Edge &b) { return a.tok < b.tok; });
    };
    std::vector<Edge> root, own;
    // strict: live(s) = a phrase ends at s, or an own edge of s leads to a live state.  An own edge leads to a descendant, and a node's
    // number is larger than its parent's, so one pass from the last node down IS the fixed point.  Only edges to live states are kept.
    std::vector<char> live;
    if (strict) {
        live = terminal;
        for (int s = S - 1; s >= 0; --s) {
            if (live[(size_t)s]) continue;
            own_edges(s, own);
            for (const Edge &e : own) if (live[(size_t)e.next]) { live[(size_t)s] = 1; break; }
        }
    }
    auto prune = [&](std::vector<Edge> &v) {
        if (strict) v.erase(std::remove_if(v.begin(), v.end(), [&](const Edge &e) { return !live[(size_t)e.next]; }), v.end());
    };
    own_edges(0, root);
    prune(root);
    set->state_off.assign((size_t)S + 1, 0);
    for (int s = 0; s < S; ++s) {
        // effective edges: the state's own, plus the root's for every token it has none for (a new match may start where this one breaks;
        // in a strict set only where a phrase has ended: inside a phrase nothing but its continuations is permitted)
        if (s == 0) own = root; else { own_edges(s, own); prune(own); }
        const bool with_root = s != 0 && (!strict || terminal[(size_t)s]);
        size_t i = 0, j = 0;
        while (i < own.size() || (with_root && j < root.size())) {
            Edge e;
            if (!with_root || j >= root.size() || (i < own.size() && own[i].tok <= root[j].tok)) {
                e = own[i];
                if (with_root && j < root.size() && root[j].tok == e.tok) ++j;
                ++i;
            } else e = root[j++];
            set->edge_tok.push_back(e.tok); set->edge_next.push_back(e.next); set->edge_bonus.push_back(e.bonus);
        }
        if ((int64_t)set->edge_tok.size() > kBiasMaxEdges) { err = "the phrases need more than " + std::to_string(kBiasMaxEdges) + " token edges"; return nullptr; }
        set->state_off[(size_t)s + 1] = (int32_t)set->edge_tok.size();
    }
    // a phrase that can be spelled keeps the edges of its spelling (each leads to a live state), so pruning loses none: the phrases left
    // out of a strict set are section 13's unspellable ones, and a set with none left would permit nothing
    if (strict && ends.empty()) { err = "no phrase of the strict set can be spelled with the model's tokens: the session could emit nothing"; return nullptr; }
    if (set->dropped) err = std::to_string(set->dropped) + " phrase(s) cannot be spelled with the model's tokens and were left out";
    return set;
}

void put_err(char *err, size_t cap, const std::string &e)
{
    if (!err || !cap) return;
    strncpy(err, e.c_str(), cap - 1);
    err[cap - 1] = 0;
}

}  // namespace

extern "C" {

AprilxBias aprilx_bias_create(AprilASRModel model, size_t n, const char *const *phrases, const float *boosts, char *err, size_t err_cap)
{
    return aprilx_bias_create_ex(model, n, phrases, boosts, 0, err, err_cap);
}

AprilxBias aprilx_bias_create_ex(AprilASRModel model, size_t n, const char *const *phrases, const float *boosts, uint32_t flags, char *err, size_t err_cap)
{
    put_err(err, err_cap, "");
    if (!model) { put_err(err, err_cap, "no model"); return nullptr; }
    if (flags & ~(uint32_t)APRILX_BIAS_STRICT) { put_err(err, err_cap, "unknown flag bits"); return nullptr; }
    static_assert(APRILX_BIAS_STRICT == kBiasStrict, "the ABI's flag is BiasSet's");
    std::string e;
    std::shared_ptr<BiasSet> set = build_set(model->m.host.params, n, phrases, boosts, flags, e);
    put_err(err, err_cap, e);
    if (!set) return nullptr;
    AprilxBias_i *h = new AprilxBias_i();
    h->set = set;
    return h;
}

void aprilx_bias_free(AprilxBias bias) { delete bias; }

int aprilx_bias_info(AprilxBias bias, int32_t *states, int64_t *edges)
{
    if (!bias) return -1;
    if (states) *states = bias->set->states();
    if (edges) *edges = bias->set->edges();
    return bias->set->dropped;
}

int aprilx_bias_flags(AprilxBias bias) { return bias ? (int)bias->set->flags : -1; }

int aprilx_bias_edges(AprilxBias bias, int32_t state, int32_t *tok, int32_t *next, float *bonus, size_t cap)
{
    if (!bias || state < 0 || state >= bias->set->states()) return -1;
    const BiasSet &b = *bias->set;
    const size_t e0 = (size_t)b.state_off[(size_t)state], cnt = (size_t)b.state_off[(size_t)state + 1] - e0;
    if (cnt > cap) return (tok || next || bonus) ? -1 : (int)cnt;
    if (tok) memcpy(tok, b.edge_tok.data() + e0, cnt * 4);
    if (next) memcpy(next, b.edge_next.data() + e0, cnt * 4);
    if (bonus) memcpy(bonus, b.edge_bonus.data() + e0, cnt * 4);
    return (int)cnt;
}

int aprilx_session_set_bias(AprilASRSession session, AprilxBias bias)
{
    if (!session) return -1;
    Session *s = &session->s;
    std::shared_ptr<const BiasSet> set = bias ? bias->set : nullptr;
    if (set && (set->vocab != s->model->host.params.token_count || set->vocab_hash != bias_vocab_hash(s->model->host.params))) return -1;      // built for another token list
    return s->sched->set_bias(s, set) ? 0 : -1;
}

int aprilx_session_bias_state(AprilASRSession session, int32_t *host_state, int32_t *device_state)
{
    if (!session) return -1;
    Session *s = &session->s;
    s->sched->wait_idle(s);
    if (host_state) *host_state = s->greedy.bias_state();
    if (device_state) *device_state = s->eng->read_bias_state(s->slot);
    return s->greedy.bias() ? 1 : 0;
}

int aprilx_run_decide_biased(AprilASRModel model, int n, int op, const float *logits, float early_emit, const int32_t *now_ms, int round,
                             int32_t *state_io, void *records_out, AprilxBias bias, int32_t *bias_state_io)
{
    if (!model || n <= 0 || model->m.engines.empty() || n > model->m.engines[0]->max_slots() || !state_io) return -1;
    if (op == 0 && (!logits || !now_ms || !records_out || round < 0 || round > 2)) return -1;
    if (!bias || !bias_state_io || bias->set->vocab != model->m.host.params.token_count || bias->set->vocab_hash != bias_vocab_hash(model->m.host.params)) return -1;
    for (int i = 0; i < n; ++i) if (bias_state_io[i] < -1 || bias_state_io[i] >= bias->set->states()) return -1;
    DecideRequest q = DecideRequest::round_of(n, op, logits, early_emit, now_ms, round, state_io, records_out);
    q.set = bias->set.get(); q.bias_state_io = bias_state_io;
    model->m.engines[0]->debug_decide(q);
    return 0;
}

int aprilx_greedy_set_bias(AprilxGreedy g, AprilxBias bias)
{
    if (!g) return -1;
    g->g.set_bias(bias ? bias->set : nullptr);
    return 0;
}

int aprilx_greedy_bias_state(AprilxGreedy g) { return g ? g->g.bias_state() : -1; }

}  // extern "C"
