// Text-corpus language model: the builder.  Host only, no GPU, no other file of the engine: plain text and a
// token list in, the automaton of lm.h out -- deterministic, byte-identical for the same input (tests/lm_ref.py states the same
// arithmetic in numpy; tests/cpp/lm_walk_test.cc runs this file under the sanitizers as a plain program).
#include <algorithm>
#include <cmath>
#include <map>
#include "lm.h"

namespace aprilx {

namespace {

// contexts in node order: by length, then by bytes ascending (unsigned)
struct CtxLess {
    bool operator()(const std::string &a, const std::string &b) const
    {
        if (a.size() != b.size()) return a.size() < b.size();
        return std::lexicographical_compare(a.begin(), a.end(), b.begin(), b.end(), [](char x, char y) { return (unsigned char)x < (unsigned char)y; });
    }
};

struct Ctx {
    std::map<unsigned char, uint64_t> cnt;         // C(h, c) > 0, bytes ascending
    uint64_t total = 0;                            // C(h)
    int node = 0;
    std::vector<double> p;                         // P(c | h) of the arcs, in arc order
};

}  // namespace

std::shared_ptr<LmSet> lm_build(const std::vector<std::string> &tokens, int blank, uint64_t vocab_hash, const void *text, size_t text_len, int order, std::string &err)
{
    err.clear();
    if (order < kLmMinOrder || order > kLmMaxOrder) { err = "the order must be " + std::to_string(kLmMinOrder) + " .. " + std::to_string(kLmMaxOrder); return nullptr; }
    if (tokens.size() > (size_t)kLmMaxVocab) { err = "language models support vocabularies of at most " + std::to_string(kLmMaxVocab) + " tokens"; return nullptr; }
    if (!text && text_len) { err = "no text"; return nullptr; }
    if (text_len > kLmMaxCorpusBytes) { err = "the corpus is larger than 64 MiB"; return nullptr; }
    auto set = std::make_shared<LmSet>();
    set->vocab = (int)tokens.size(); set->blank = blank; set->vocab_hash = vocab_hash; set->order = order;
    bool in_a[256] = {false};
    set->tok_off.assign(tokens.size() + 1, 0);
    for (size_t i = 0; i < tokens.size(); ++i) {
        for (unsigned char c : tokens[i]) { set->tok_bytes.push_back(c); if ((int)i != blank) in_a[c] = true; }
        set->tok_off[i + 1] = (int32_t)set->tok_bytes.size();
    }
    if (in_a[kLmBos]) { err = "a token's text contains the byte 0x0A, which language models use as the start of a line"; return nullptr; }
    for (bool b : in_a) set->alphabet += b ? 1 : 0;

    // ---- normalisation and counts
    std::map<std::string, Ctx, CtxLess> ctx;
    const unsigned char *p = (const unsigned char *)text;
    const int N = order;
    size_t kept = 0;
    std::string line;
    for (size_t at = 0; at <= text_len; ) {
        size_t end = at;
        while (end < text_len && p[end] != kLmBos) ++end;
        line.assign(1, (char)kLmBos);                                  // b_0
        bool foreign = false, pending_space = true;                    // (the prepended ' ' is the first pending one)
        bool any = false;
        for (size_t i = at; i < end; ++i) {
            unsigned char c = p[i];
            if (c == '\r' || c == '\t') c = ' ';
            if (c == ' ') { pending_space = true; continue; }
            if (pending_space) { line.push_back(' '); pending_space = false; }
            line.push_back((char)c);
            any = true;
            if (!in_a[c]) foreign = true;
        }
        at = end + 1;
        if (!any) continue;                                            // empty line
        if (foreign || !in_a[(unsigned char)' ']) { ++set->dropped; continue; }
        ++kept;
        const int m = (int)line.size() - 1;
        for (int i = 1; i <= m; ++i)
            for (int k = 0; k <= std::min(N - 1, i); ++k) {
                Ctx &c = ctx[line.substr((size_t)(i - k), (size_t)k)];
                ++c.cnt[(unsigned char)line[(size_t)i]];
                ++c.total;
            }
        if ((int64_t)ctx.size() > kLmMaxNodes) { err = "the corpus needs more than 4 Mi nodes"; return nullptr; }
    }
    if (!kept) { err = "no line of the corpus is left" + (set->dropped ? " (" + std::to_string(set->dropped) + " dropped for bytes no token has)" : std::string()); return nullptr; }

    // ---- nodes (the map's order is the numbering: the root "" first), estimation in float64, arcs
    int n_nodes = 0;
    int64_t n_arcs = 0;
    for (auto &kv : ctx) { kv.second.node = n_nodes++; n_arcs += (int64_t)kv.second.cnt.size(); }
    if (n_arcs > kLmMaxArcs) { err = "the corpus needs more than 16 Mi arcs"; return nullptr; }
    auto node_of = [&](const std::string &h) -> const Ctx * { auto it = ctx.find(h); return it == ctx.end() ? nullptr : &it->second; };
    const Ctx &root = ctx.begin()->second;
    const double A = (double)set->alphabet, Te = (double)root.cnt.size(), Ce = (double)root.total;
    set->unk_logp = (float)std::log(Te / ((Ce + Te) * A));
    set->node_off.assign((size_t)n_nodes + 1, 0);
    set->back.assign((size_t)n_nodes, 0);
    set->bow.assign((size_t)n_nodes, 0.0f);
    set->arc_byte.reserve((size_t)n_arcs); set->arc_logp.reserve((size_t)n_arcs); set->arc_next.reserve((size_t)n_arcs);
    for (auto &kv : ctx) {
        const std::string &h = kv.first;
        Ctx &c = kv.second;
        const double T = (double)c.cnt.size(), C = (double)c.total;
        const Ctx *lower = h.empty() ? nullptr : node_of(h.substr(1));     // exists: C(h') >= C(h)
        set->back[(size_t)c.node] = lower ? lower->node : 0;
        set->bow[(size_t)c.node] = (float)std::log(T / (C + T));
        c.p.reserve(c.cnt.size());
        for (const auto &bc : c.cnt) {
            double P;
            if (!lower) P = ((double)bc.second + Te / A) / (Ce + Te);
            else {
                const size_t j = (size_t)std::distance(lower->cnt.begin(), lower->cnt.find(bc.first));
                P = ((double)bc.second + T * lower->p[j]) / (C + T);
            }
            c.p.push_back(P);
            std::string hc = h + (char)bc.first;
            if ((int)hc.size() > N - 1) hc.erase(0, 1);
            const Ctx *nx;
            while (!(nx = node_of(hc))) hc.erase(0, 1);                    // (ends at the root at the latest)
            set->arc_byte.push_back(bc.first);
            set->arc_logp.push_back((float)std::log(P));
            set->arc_next.push_back(nx->node);
        }
        set->node_off[(size_t)c.node + 1] = (int32_t)set->arc_byte.size();
    }
    set->start = node_of(std::string(1, (char)kLmBos))->node;
    if (set->dropped) err = std::to_string(set->dropped) + " line(s) of the corpus hold a byte no token has and were left out";
    return set;
}

}  // namespace aprilx
