// Text-corpus language model: a byte-level n-gram model as the search uses it -- the back-off automaton of an
// interpolated Witten-Bell estimate (nodes = the seen contexts, CSR arcs sorted by byte), the token text table, and the fp32 walk.
// Built on the host (lm.cc, no GPU), uploaded per engine at first use, walked per token by the decision kernel (kernels_lm.inc) and,
// independently, by the host's state machine (Greedy).
// Header-only on purpose: session.cc is also built without lm.cc (tests/sched_harness).
#pragma once
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace aprilx {

constexpr int kLmMaxVocab = 8192;                  // kBiasMaxVocab: the LM forms of the decision kernel use the biased forms' LDS table
constexpr int kLmMinOrder = 2, kLmMaxOrder = 8, kLmDefaultOrder = 5;
constexpr size_t kLmMaxCorpusBytes = (size_t)64 << 20;
constexpr int64_t kLmMaxNodes = 4 << 20, kLmMaxArcs = 16 << 20;
constexpr float kLmMaxWeight = 10.0f, kLmMaxTokenBonus = 100.0f;
constexpr unsigned char kLmBos = 0x0A;             // context only, never predicted
constexpr int kLmModels = 8;                       // descriptor table entries of one engine

struct LmSet {
    int vocab = 0, blank = 0;                      // of the model it was built for
    uint64_t vocab_hash = 0;                       // bias_vocab_hash of that model's token list
    int order = 0, dropped = 0, alphabet = 0;      // N; corpus lines dropped for a byte outside the alphabet; |A|
    int start = 0;                                 // the node of the one-byte context BOS (never 0: 0 is the root)
    float unk_logp = 0.0f;
    std::vector<int32_t> node_off;                 // [nodes + 1]
    std::vector<int32_t> back;                     // [nodes] the node of the context without its first byte (root: root)
    std::vector<float> bow;                        // [nodes]
    std::vector<uint8_t> arc_byte;                 // [arcs] arcs of node s: [node_off[s], node_off[s + 1]), bytes ascending
    std::vector<float> arc_logp;
    std::vector<int32_t> arc_next;
    std::vector<int32_t> tok_off;                  // [vocab + 1] into tok_bytes: the text of every token (section 13's text model)
    std::vector<uint8_t> tok_bytes;
    int nodes() const { return (int)back.size(); }
    int64_t arcs() const { return (int64_t)arc_byte.size(); }
    int find(int s, unsigned char c) const
    {
        int lo = node_off[(size_t)s], hi = node_off[(size_t)s + 1];
        const int end = hi;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (arc_byte[(size_t)mid] < c) lo = mid + 1; else hi = mid;
        }
        return lo < end && arc_byte[(size_t)lo] == c ? lo : -1;
    }
    // one byte: fp32 additions in the order written (the file is compiled without contraction; there is no product here anyway)
    void step(int &s, unsigned char c, float &acc) const
    {
        for (;;) {
            const int e = find(s, c);
            if (e >= 0) { acc = acc + arc_logp[(size_t)e]; s = arc_next[(size_t)e]; return; }
            if (s == 0) { acc = acc + unk_logp; return; }
            acc = acc + bow[(size_t)s]; s = back[(size_t)s];
        }
    }
    // score(s, tok): the walk over the bytes of the token's text from node s; returns the new node
    int score(int s, int tok, float *acc_out) const
    {
        float acc = 0.0f;
        for (int i = tok_off[(size_t)tok]; i < tok_off[(size_t)tok + 1]; ++i) step(s, tok_bytes[(size_t)i], acc);
        if (acc_out) *acc_out = acc;
        return s;
    }
    int next(int s, int tok) const { return score(s, tok, nullptr); }
};

// lm.cc (not in the scheduler harness): the model of `text` for the token list `tokens` (the text of every token, the blank included;
// the blank's bytes are not part of the alphabet).  Null and a message in err when refused; a note in err when lines were dropped.
std::shared_ptr<LmSet> lm_build(const std::vector<std::string> &tokens, int blank, uint64_t vocab_hash, const void *text, size_t text_len, int order, std::string &err);

}  // namespace aprilx
