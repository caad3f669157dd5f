// Phrase boosting: a bias set as the search uses it -- the byte trie of the phrases, flattened into the
// effective token edges of every trie node (CSR, sorted by token id).  Built on the host (bias.cc, no GPU), uploaded per engine at
// first use, walked by the decision kernel (kernels_bias.inc) and, independently, by the host's state machine (Greedy).
// Header-only on purpose: session.cc is also built without bias.cc (tests/sched_harness).
#pragma once
#include <cstdint>
#include <vector>
#include "model_loader.h"

namespace aprilx {

constexpr int kBiasMaxStates = 65535;              // a state fits the kernel's 16-bit LDS cell
constexpr int64_t kBiasMaxEdges = 4 << 20;         // effective edges of one set
constexpr int kBiasMaxPhraseBytes = 256;
constexpr float kBiasMaxBoost = 100.0f;
constexpr int kBiasMaxVocab = 8192;                // 6 bytes of LDS per token in the biased decision kernel (48 KB)
constexpr uint32_t kBiasStrict = 1;                // BiasSet::flags (APRILX_BIAS_STRICT): a token without an edge is forbidden, not "no bonus"

// FNV-1a over the token texts (each with its NUL) and the blank id: a set only fits the token list it was built for
inline uint64_t bias_vocab_hash(const ModelParams &p)
{
    uint64_t h = 1469598103934665603ull;
    auto byte = [&](unsigned char c) { h = (h ^ c) * 1099511628211ull; };
    for (int i = 0; i < p.token_count; ++i) { const char *t = p.token((size_t)i); do byte((unsigned char)*t); while (*t++); }
    for (int k = 0; k < 4; ++k) byte((unsigned char)(p.blank_id >> (8 * k)));
    return h;
}

struct BiasSet {
    int vocab = 0;                                 // of the model it was built for
    uint64_t vocab_hash = 0;                       // bias_vocab_hash of that model's token list
    uint32_t flags = 0;                            // kBiasStrict: the edges below are the PERMITTED tokens of every state (a closed phrase list)
    int dropped = 0;                               // phrases no token sequence can spell (left out of the trie)
    std::vector<int32_t> state_off;                // [states + 1]
    std::vector<int32_t> edge_tok, edge_next;      // [edges] effective edges of state s: [state_off[s], state_off[s + 1]), token ids ascending
    std::vector<float> edge_bonus;
    int states() const { return (int)state_off.size() - 1; }
    int64_t edges() const { return (int64_t)edge_tok.size(); }
    // effective edge (s, tok), or -1: the token leads to the root with bonus 0 (a strict set: the search never decides for such a token
    // unless nothing permitted beat the initial value and the blank lost as well -- the NaN row of decide_body --, then to the root too)
    int find(int s, int tok) const
    {
        int lo = state_off[(size_t)s], hi = state_off[(size_t)s + 1];
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (edge_tok[(size_t)mid] < tok) lo = mid + 1; else hi = mid;
        }
        return lo < state_off[(size_t)s + 1] && edge_tok[(size_t)lo] == tok ? lo : -1;
    }
    int next(int s, int tok) const { const int e = find(s, tok); return e < 0 ? 0 : edge_next[(size_t)e]; }
};

}  // namespace aprilx
