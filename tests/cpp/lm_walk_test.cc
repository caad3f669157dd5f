// The language-model builder (csrc/lm.cc) and the walk (csrc/lm.h) as a plain host program, for AddressSanitizer + UBSan
// (tests/test_lm_cpu.py builds and runs it; no GPU, no Python): corpora with edge shapes through every order, every (node, token) pair
// walked, the structural promises of DESIGN.md section 20 checked on the arrays.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "lm.h"

using namespace aprilx;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static void check_model(const LmSet &m, const std::vector<std::string> &tokens)
{
    const int n = m.nodes();
    CHECK(n >= 2 && m.start > 0 && m.start < n && m.back[0] == 0);
    CHECK((int)m.node_off.size() == n + 1 && m.node_off[0] == 0 && m.node_off[(size_t)n] == (int32_t)m.arcs());
    CHECK(m.arc_logp.size() == m.arc_byte.size() && m.arc_next.size() == m.arc_byte.size() && (int)m.bow.size() == n);
    for (int s = 0; s < n; ++s) {
        CHECK(m.back[(size_t)s] >= 0 && m.back[(size_t)s] < n && (s == 0 || m.back[(size_t)s] < s));      // a shorter context has a smaller number
        CHECK(std::isfinite(m.bow[(size_t)s]) && m.bow[(size_t)s] < 0.0f);
        CHECK(m.node_off[(size_t)s] < m.node_off[(size_t)s + 1]);                                          // every node has seen a byte
        for (int e = m.node_off[(size_t)s]; e < m.node_off[(size_t)s + 1]; ++e) {
            CHECK(e == m.node_off[(size_t)s] || m.arc_byte[(size_t)e - 1] < m.arc_byte[(size_t)e]);
            CHECK(m.arc_byte[(size_t)e] != kLmBos && m.arc_next[(size_t)e] >= 0 && m.arc_next[(size_t)e] < n);
            CHECK(std::isfinite(m.arc_logp[(size_t)e]) && m.arc_logp[(size_t)e] <= 0.0f);
        }
    }
    CHECK(std::isfinite(m.unk_logp) && m.unk_logp < 0.0f);
    for (int s = 0; s < n; ++s)
        for (int t = 0; t < (int)tokens.size(); ++t) {
            float acc = 1.0f;
            const int nx = m.score(s, t, &acc);
            CHECK(nx >= 0 && nx < n && std::isfinite(acc) && acc <= 0.0f);
            if (tokens[(size_t)t].empty()) CHECK(nx == s && acc == 0.0f);
            CHECK(m.next(s, t) == nx);
        }
}

int main()
{
    const std::vector<std::string> tokens = {"<blk>", " a", " ab", "b", "c", " cab", "", "abcabcabcabc", "z", " ", "\xc3\xa9"};
    const std::string corpora[] = {
        "ab cab\n",
        "a\n",
        "ab cab\r\nab  cab\t c\n\n\n   \nabcabcabcabc ab\nab cab",
        "x\nab\nqq q\n b a c\n",
        std::string("ab\0cab\nab\n", 10),
        " \xc3\xa9 \xc3\xa9\xc3\xa9 ab\n",
    };
    std::string err;
    for (const std::string &text : corpora)
        for (int order = kLmMinOrder; order <= kLmMaxOrder; ++order) {
            std::shared_ptr<LmSet> m = lm_build(tokens, 0, 42, text.data(), text.size(), order, err);
            CHECK(m != nullptr);
            if (!m) { printf("refused: %s\n", err.c_str()); continue; }
            CHECK(m->order == order && m->vocab == (int)tokens.size() && m->alphabet == 7);
            check_model(*m, tokens);
            std::shared_ptr<LmSet> again = lm_build(tokens, 0, 42, text.data(), text.size(), order, err);
            CHECK(again && again->arc_logp == m->arc_logp && again->arc_next == m->arc_next && again->bow == m->bow && again->node_off == m->node_off);
        }
    {   // dropped lines are counted and noted; a corpus without a line left, a bad order, a newline token are refused with a message
        std::shared_ptr<LmSet> m = lm_build(tokens, 0, 42, "ab\nxyz\nq\n", 9, 3, err);
        CHECK(m && m->dropped == 2 && !err.empty());
        CHECK(!lm_build(tokens, 0, 42, "xyz\n\n", 5, 3, err) && !err.empty());
        CHECK(!lm_build(tokens, 0, 42, "", 0, 3, err) && !err.empty());
        CHECK(!lm_build(tokens, 0, 42, nullptr, 0, 3, err) && !err.empty());
        CHECK(!lm_build(tokens, 0, 42, "ab\n", 3, 1, err) && !err.empty());
        CHECK(!lm_build(tokens, 0, 42, "ab\n", 3, 9, err) && !err.empty());
        std::vector<std::string> bad = tokens;
        bad[3] = "b\n";
        CHECK(!lm_build(bad, 0, 42, "ab\n", 3, 3, err) && !err.empty());
        // the blank's bytes are not part of the alphabet
        CHECK(!lm_build(tokens, 0, 42, "<blk>\n", 6, 3, err));
    }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("all checks passed\n");
    return 0;
}
