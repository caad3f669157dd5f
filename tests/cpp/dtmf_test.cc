// csrc/dtmf.h alone, as a stand-alone program under AddressSanitizer + UBSan (tests/test_dtmf_cpu.py builds and runs it): the plan and
// its refusals, the tables, frames through steps 1-5 out of buffers of exactly the size the contract reads (an overread is a report),
// the decision's ties, and the event machine.  Prints "all checks passed".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "dtmf.h"

using namespace aprilx;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

struct Ev { int kind; char digit; uint64_t ms; bool operator==(const Ev &o) const { return kind == o.kind && digit == o.digit && ms == o.ms; } };

static std::vector<int16_t> tone(char digit, int n, int rate, double amp_r, double amp_c)
{
    const int k = (int)std::string(kDtmfDigits).find(digit);
    std::vector<int16_t> x((size_t)n);
    for (int j = 0; j < n; ++j) {
        const double t = (double)j / rate;
        const double v = amp_r * std::sin(2.0 * M_PI * kDtmfHz[k / 4] * t + 0.3) + amp_c * std::sin(2.0 * M_PI * kDtmfHz[4 + k % 4] * t + 1.1);
        x[(size_t)j] = (int16_t)std::lrint(v * 32767.0);
    }
    return x;
}

static std::vector<Ev> run_events(const DtmfPlan &p, const std::vector<uint8_t> &codes, bool flush, DtmfMachine *m_out = nullptr)
{
    std::vector<Ev> ev;
    DtmfMachine m;
    auto emit = [&](int kind, char digit, uint64_t ms) { ev.push_back(Ev{kind, digit, ms}); };
    dtmf_events(p, 10, 0, codes.data(), codes.size(), m, emit);
    if (flush) dtmf_flush(10, codes.size(), m, emit);
    if (m_out) *m_out = m;
    return ev;
}

int main()
{
    DtmfOptions def;
    DtmfPlan p;
    // the plan
    CHECK(dtmf_make_plan(16000, 512, 10, def, &p) && p.Wd == 256 && p.half_w == 128.0f && p.on_frames == 2 && p.off_frames == 2);
    CHECK(std::fabs(p.min_power - 1.7592186e9f) < 1e3f && std::fabs(p.twist_hi - 2.5118864f) < 1e-6f && std::fabs(p.twist_lo - 6.3095734f) < 1e-6f);
    CHECK(dtmf_make_plan(8000, 256, 10, def, &p) && p.Wd == 128);
    CHECK(dtmf_make_plan(16000, 200, 10, def, &p) && p.Wd == 200 && p.half_w == 100.0f);
    CHECK(dtmf_window(16000, 191) == 0 && dtmf_window(16000, 192) == 192 && dtmf_window(3999, 512) == 0 && dtmf_window(300000, 8192) == 0);
    CHECK(dtmf_window(256000, 8192) == 4096 && dtmf_window(7999, 256) == 0 && dtmf_window(16000, 0) == 0);
    {
        DtmfOptions o = def; o.min_share = 0.0f; CHECK(!dtmf_make_plan(16000, 512, 10, o, &p));
        o = def; o.min_share = NAN; CHECK(!dtmf_make_plan(16000, 512, 10, o, &p));
        o = def; o.rel_peak_db = 2.0f; CHECK(!dtmf_make_plan(16000, 512, 10, o, &p));
        o = def; o.min_tone_ms = 9; CHECK(!dtmf_make_plan(16000, 512, 10, o, &p));
        o = def; o.min_pause_ms = 1001; CHECK(!dtmf_make_plan(16000, 512, 10, o, &p));
        o = def; o.min_level_dbfs = -71.0f; CHECK(!dtmf_make_plan(16000, 512, 10, o, &p));
        o = def; o.twist_hi_db = INFINITY; CHECK(!dtmf_make_plan(16000, 512, 10, o, &p));
        CHECK(!dtmf_make_plan(16000, 512, 0, def, &p));
        o = def; o.min_tone_ms = 1000; o.min_pause_ms = 10; CHECK(dtmf_make_plan(16000, 512, 25, o, &p) && p.on_frames == 40 && p.off_frames == 1);
    }
    // frames of every digit out of exact-size heap buffers, for a whole and a ragged window
    for (int fft : {512, 200, 128}) {
        const int rate = fft == 128 ? 8000 : 16000;
        CHECK(dtmf_make_plan(rate, fft, 10, def, &p));
        std::vector<float> tab((size_t)kDtmfRows * (size_t)p.Wd);
        dtmf_make_tables(rate, p.Wd, tab.data());
        CHECK(tab[0] == 1.0f && tab[(size_t)8 * (size_t)p.Wd] == 0.0f);
        for (int d = 0; d < 16; ++d) {
            const int n = 3;
            std::vector<int16_t> x = tone(kDtmfDigits[d], (n - 1) * 7 + p.Wd, rate, 0.2, 0.2);      // frames 7 samples apart; the last ends with the buffer
            std::vector<int16_t> fr((size_t)n * (size_t)p.Wd);                                       // ld == Wd: not a sample more than is read
            for (int i = 0; i < n; ++i) for (int j = 0; j < p.Wd; ++j) fr[(size_t)i * p.Wd + j] = x[(size_t)i * 7 + j];
            std::vector<uint8_t> codes((size_t)n);
            std::vector<float> pw((size_t)n * 9);
            dtmf_run_host(p, tab.data(), n, fr.data(), (size_t)p.Wd, codes.data(), pw.data());
            if (fft != 200) for (int i = 0; i < n; ++i) CHECK(codes[(size_t)i] == d + 1);
            // |correlation| of a tone of amplitude A over Wd samples is about A Wd / 2
            const float want = (float)std::pow(0.2 * 32767.0 * p.Wd / 2.0, 2.0);
            CHECK(pw[(size_t)(d / 4)] > 0.5f * want && pw[(size_t)(d / 4)] < 2.0f * want);
            int64_t e = 0;
            for (int j = 0; j < p.Wd; ++j) e += (int64_t)fr[(size_t)j] * fr[(size_t)j];
            CHECK(pw[8] == (float)e);
            std::vector<uint8_t> again((size_t)n);
            dtmf_run_host(p, tab.data(), n, fr.data(), (size_t)p.Wd, again.data(), nullptr);
            CHECK(again == codes);
        }
        // silence, and the lowest sample throughout
        std::vector<int16_t> z((size_t)p.Wd, 0), low((size_t)p.Wd, (int16_t)-32768);
        uint8_t c = 9; float q[9];
        dtmf_run_host(p, tab.data(), 1, z.data(), (size_t)p.Wd, &c, q);
        CHECK(c == 0 && q[8] == 0.0f && q[0] == 0.0f);
        dtmf_run_host(p, tab.data(), 1, low.data(), (size_t)p.Wd, &c, q);
        CHECK(c == 0 && q[8] == (float)p.Wd * 1073741824.0f);
        dtmf_run_host(p, tab.data(), 0, nullptr, 0, nullptr, nullptr);
    }
    // the decision's ties
    CHECK(dtmf_make_plan(16000, 512, 10, def, &p));
    {
        const float big = 1099511627776.0f;      // 2^40
        float q[9] = {0, big, 0, 0, 0, 0, big * p.twist_hi, 0, 0};
        CHECK(dtmf_decide(p, q, q[8]) == 1 + 4 * 1 + 2);
        q[6] = std::nextafter(q[6], INFINITY); CHECK(dtmf_decide(p, q, q[8]) == 0);
        float s[9] = {big, big * p.rel_peak, big, big, 0, 0, 0, big * p.rel_peak, 0};
        CHECK(dtmf_decide(p, s, s[8]) == 1 + 4 * 1 + 3);
        s[2] = std::nextafter(big, INFINITY); CHECK(dtmf_decide(p, s, s[8]) == 0);
        float t[9] = {big, big, 0, 0, big, 0, 0, 0, 0};                       // two equal row peaks: refused by the second
        CHECK(dtmf_decide(p, t, t[8]) == 0);
        float u[9] = {p.min_power, 0, 0, 0, p.min_power, 0, 0, 0, 0};
        CHECK(dtmf_decide(p, u, u[8]) == 1);
        u[8] = NAN; CHECK(dtmf_decide(p, u, u[8]) == 1);
        u[0] = NAN; CHECK(dtmf_decide(p, u, u[8]) == 0);
    }
    // the event machine
    {
        DtmfMachine m;
        CHECK((run_events(p, {0, 5, 0, 0, 5, 5, 0, 0}, false) == std::vector<Ev>{{DTMF_DOWN, '4', 40}, {DTMF_UP, '4', 60}}));
        CHECK((run_events(p, {1, 1, 1, 6, 6, 6}, true, &m) == std::vector<Ev>{{DTMF_DOWN, '1', 0}, {DTMF_UP, '1', 30}, {DTMF_DOWN, '5', 40}, {DTMF_UP, '5', 60}}));
        CHECK(m.held == 0 && m.cand == 0 && m.run == 0);
        CHECK((run_events(p, {0, 2, 2, 2}, true) == std::vector<Ev>{{DTMF_DOWN, '2', 10}, {DTMF_UP, '2', 40}}));
        CHECK((run_events(p, {1, 1, 0, 1, 0, 1, 0, 0, 0}, false) == std::vector<Ev>{{DTMF_DOWN, '1', 0}, {DTMF_UP, '1', 60}}));
        CHECK(run_events(p, {200, 200, 17, 17}, true).empty());              // bytes that are no code count as none
        DtmfOptions o = def; o.min_tone_ms = 10; o.min_pause_ms = 10;
        DtmfPlan p1;
        CHECK(dtmf_make_plan(16000, 512, 10, o, &p1));
        CHECK((run_events(p1, {3, 3, 4, 0, 16}, true) == std::vector<Ev>{{DTMF_DOWN, '3', 0}, {DTMF_UP, '3', 20}, {DTMF_DOWN, 'A', 20}, {DTMF_UP, 'A', 30},
                                                                            {DTMF_DOWN, 'D', 40}, {DTMF_UP, 'D', 50}}));
        CHECK(run_events(p, {}, true).empty());
    }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("all checks passed\n");
    return 0;
}
