// csrc/tone.h alone, as a stand-alone program under AddressSanitizer + UBSan (tests/test_tone_cpu.py builds and runs it): the grid and
// its refusals, the plan, the tables, frames through steps 1-7 out of buffers of exactly the size the contract reads (an overread is a
// report), the decision's edges, and the event machine.  Prints "all checks passed".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tone.h"

using namespace aprilx;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

struct Ev { int kind; uint32_t f1, f2; uint64_t ms; bool operator==(const Ev &o) const { return kind == o.kind && f1 == o.f1 && f2 == o.f2 && ms == o.ms; } };

static std::vector<int16_t> tones(int n, int rate, double hz1, double amp1, double hz2 = 0, double amp2 = 0)
{
    std::vector<int16_t> x((size_t)n);
    for (int j = 0; j < n; ++j) {
        const double t = (double)j / rate;
        x[(size_t)j] = (int16_t)std::lrint((amp1 * std::sin(2.0 * M_PI * hz1 * t + 0.3) + amp2 * std::sin(2.0 * M_PI * hz2 * t + 1.1)) * 32767.0);
    }
    return x;
}

static uint32_t rec(uint32_t a, uint32_t b = 0) { return a | b << 16; }

static std::vector<Ev> run_events(const TonePlan &p, const std::vector<uint32_t> &r, bool flush, size_t cut = 0)
{
    std::vector<Ev> ev;
    ToneMachine m;
    auto emit = [&](int kind, uint32_t f1, uint32_t f2, uint64_t ms) { ev.push_back(Ev{kind, f1, f2, ms}); };
    tone_events(p, 10, 0, r.data(), cut, m, emit);
    tone_events(p, 10, cut, r.data() + cut, r.size() - cut, m, emit);
    if (flush) tone_flush(10, r.size(), m, emit);
    return ev;
}

int main()
{
    ToneOptions def;
    TonePlan p;
    int w, k_lo, f;
    // the grid and its refusals
    CHECK(tone_grid(16000, 512, &w, &k_lo, &f) && w == 512 && k_lo == 10 && f == 64);
    CHECK(tone_grid(8000, 256, &w, &k_lo, &f) && w == 256 && k_lo == 10 && f == 64);
    CHECK(tone_grid(16000, 400, &w, &k_lo, &f) && w == 384 && k_lo == 8 && f == 48);
    CHECK(tone_grid(48000, 2048, &w, &k_lo, &f) && w == 2048 && k_lo == 13 && f == 86);
    CHECK(!tone_grid(16000, 319, &w, &k_lo, &f) && tone_grid(16000, 320, &w, &k_lo, &f) && w == 320);      // 20 ms exactly
    CHECK(!tone_grid(5999, 256, &w, &k_lo, &f) && tone_grid(6000, 256, &w, &k_lo, &f) && f == 86 && !tone_grid(6000, 512, &w, &k_lo, &f));      // (171 bins)
    CHECK(!tone_grid(48000, 8192, &w, &k_lo, &f) && !tone_grid(16000, 0, &w, &k_lo, &f) && !tone_grid(16000, -5, &w, &k_lo, &f));
    CHECK(!tone_grid(16000, 4096, &w, &k_lo, &f));              // 512 bins in 300 .. 2300 Hz: F > 128
    CHECK(tone_grid(6000, 128, &w, &k_lo, &f) && w == 128 && f >= 8);
    // the plan
    CHECK(tone_make_plan(16000, 512, 10, def, &p) && p.W == 512 && p.k_lo == 10 && p.F == 64 && p.half_w == 256.0f && p.bin_hz == 31.25f);
    CHECK(p.on_frames == 6 && p.off_frames == 3 && p.tol_hz == 20 && std::fabs(p.second_ratio - 10.0f) < 1e-5f && p.min_share == 0.7f);
    CHECK(std::fabs(p.min_power - 7.0368742e9f) < 1e4f);
    {
        ToneOptions o = def; o.min_share = 0.0f; CHECK(!tone_make_plan(16000, 512, 10, o, &p));
        o = def; o.min_share = NAN; CHECK(!tone_make_plan(16000, 512, 10, o, &p));
        o = def; o.second_db = 2.9f; CHECK(!tone_make_plan(16000, 512, 10, o, &p));
        o = def; o.second_db = 30.5f; CHECK(!tone_make_plan(16000, 512, 10, o, &p));
        o = def; o.tol_hz = 0; CHECK(!tone_make_plan(16000, 512, 10, o, &p));
        o = def; o.tol_hz = 201; CHECK(!tone_make_plan(16000, 512, 10, o, &p));
        o = def; o.min_tone_ms = 9; CHECK(!tone_make_plan(16000, 512, 10, o, &p));
        o = def; o.min_pause_ms = 5001; CHECK(!tone_make_plan(16000, 512, 10, o, &p));
        o = def; o.min_level_dbfs = -71.0f; CHECK(!tone_make_plan(16000, 512, 10, o, &p));
        o = def; o.min_level_dbfs = INFINITY; CHECK(!tone_make_plan(16000, 512, 10, o, &p));
        CHECK(!tone_make_plan(16000, 512, 0, def, &p));
        o = def; o.min_tone_ms = 5000; o.min_pause_ms = 10; o.tol_hz = 200; o.second_db = 3.0f; o.min_share = 1.0f;
        CHECK(tone_make_plan(16000, 512, 10, o, &p) && p.on_frames == 500 && p.off_frames == 1);
        CHECK(tone_make_plan(16000, 512, 25, def, &p) && p.on_frames == 2 && p.off_frames == 1);
    }
    // frames out of buffers of exactly W samples, tables of exactly 2 F W values
    const int geos[][2] = {{16000, 512}, {8000, 256}, {16000, 400}, {48000, 2048}};
    for (const auto &g : geos) {
        const int rate = g[0];
        CHECK(tone_make_plan(rate, g[1], 10, def, &p));
        std::vector<float> tab((size_t)2 * p.F * p.W);
        tone_make_tables(p.W, p.k_lo, p.F, tab.data());
        CHECK(tab[0] == 1.0f && tab[(size_t)p.F * p.W] == 0.0f);
        std::vector<float> pw((size_t)p.F + 1);
        uint32_t r = 0;
        // a single tone on a bin, midway, a pair, silence, the lowest sample
        const double bin = (double)rate / p.W;
        std::vector<int16_t> x = tones(p.W, rate, (p.k_lo + 20) * bin, 0.25);
        tone_run_host(p, tab.data(), 1, x.data(), (size_t)p.W, &r, pw.data());
        CHECK((r >> 16) == 0 && std::fabs((double)(r & 0xffff) - (p.k_lo + 20) * bin) <= 2.0);
        x = tones(p.W, rate, (p.k_lo + 20.5) * bin, 0.25);
        tone_run_host(p, tab.data(), 1, x.data(), (size_t)p.W, &r, nullptr);
        CHECK((r >> 16) == 0 && std::fabs((double)(r & 0xffff) - (p.k_lo + 20.5) * bin) <= 4.0);
        x = tones(p.W, rate, 480.0, 0.2, 620.0, 0.2);
        tone_run_host(p, tab.data(), 1, x.data(), (size_t)p.W, &r, nullptr);
        CHECK(std::fabs((double)(r & 0xffff) - 480.0) <= 15.0 && std::fabs((double)(r >> 16) - 620.0) <= 15.0);
        x.assign((size_t)p.W, (int16_t)0);
        tone_run_host(p, tab.data(), 1, x.data(), (size_t)p.W, &r, pw.data());
        CHECK(r == 0 && pw[(size_t)p.F] == 0.0f);
        x.assign((size_t)p.W, (int16_t)-32768);
        tone_run_host(p, tab.data(), 1, x.data(), (size_t)p.W, &r, pw.data());
        CHECK(r == 0 && pw[(size_t)p.F] == (float)p.W * 1073741824.0f);
        // the decision's edges
        std::vector<float> q((size_t)p.F + 1, 0.0f);
        q[5] = p.min_power;
        CHECK(tone_decide(p, q.data(), 0.0f) == rec(tone_hz(p, q.data(), 5)) && tone_hz(p, q.data(), 5) != 0);
        q[5] = std::nextafter(p.min_power, 0.0f);
        CHECK(tone_decide(p, q.data(), 0.0f) == 0);
        const float p2 = 1099511627776.0f, p1 = p2 * p.second_ratio;
        q[5] = p1; q[20] = p2;
        CHECK((tone_decide(p, q.data(), 0.0f) >> 16) != 0);         // P2 * ratio == P1: a pair
        q[5] = std::nextafter(p1, INFINITY);
        CHECK((tone_decide(p, q.data(), 0.0f) >> 16) == 0);
        q[20] = 0.0f;
        const float e = 4294967296.0f, need = p.min_share * (e * p.half_w);
        q[5] = need;
        CHECK(tone_decide(p, q.data(), e) != 0);
        q[5] = std::nextafter(need, 0.0f);
        CHECK(tone_decide(p, q.data(), e) == 0);
        q[5] = 1e12f; q[6] = NAN;
        (void)tone_decide(p, q.data(), 0.0f);                       // (no trap, no out-of-range conversion)
        q[5] = INFINITY; q[6] = INFINITY;
        CHECK(tone_decide(p, q.data(), 0.0f) == 0);
        q[6] = 0.0f; q[5] = 1e12f;
        CHECK(tone_decide(p, q.data(), NAN) != 0);
        q[5] = 0.0f; q[0] = 1e12f; q[(size_t)p.F - 1] = 1e12f;      // both grid edges
        const uint32_t both = tone_decide(p, q.data(), 0.0f);
        CHECK((both & 0xffff) == tone_hz(p, q.data(), 0) && (both >> 16) == tone_hz(p, q.data(), p.F - 1));
    }
    // the event machine: on 6, off 3
    CHECK(tone_make_plan(16000, 512, 10, def, &p));
    {
        std::vector<uint32_t> r(8, rec(1100));
        r.insert(r.end(), 4, 0u);
        const std::vector<Ev> want = {{TONE_ON, 1100, 0, 0}, {TONE_OFF, 1100, 0, 80}};
        for (size_t cut = 0; cut <= r.size(); ++cut) CHECK(run_events(p, r, false, cut) == want);
        // a run one frame short gives nothing; a non-matching tonal frame restarts the run with itself
        std::vector<uint32_t> s(5, rec(1100));
        s.push_back(rec(1150));
        s.insert(s.end(), 5, rec(1150));
        s.push_back(0u);
        const std::vector<Ev> got = run_events(p, s, true);
        CHECK(got.size() == 2 && got[0] == (Ev{TONE_ON, 1150, 0, 50}) && got[1] == (Ev{TONE_OFF, 1150, 0, 120}));
        // a step of 50 Hz inside a held tone: OFF, then ON from the frame that ended the hold
        std::vector<uint32_t> t(8, rec(1000));
        t.insert(t.end(), 8, rec(1050));
        const std::vector<Ev> st = run_events(p, t, true);
        CHECK(st.size() == 4 && st[0] == (Ev{TONE_ON, 1000, 0, 0}) && st[1] == (Ev{TONE_OFF, 1000, 0, 80}) && st[2] == (Ev{TONE_ON, 1050, 0, 100}) &&
              st[3] == (Ev{TONE_OFF, 1050, 0, 160}));
        // the event carries the frequencies of the frame that completed the run; drift inside tol of the REFERENCE keeps the run
        std::vector<uint32_t> d = {rec(1000), rec(1010), rec(1020), rec(1015), rec(1005), rec(1018)};
        const std::vector<Ev> dr = run_events(p, d, true);
        CHECK(dr.size() == 2 && dr[0] == (Ev{TONE_ON, 1018, 0, 0}) && dr[1] == (Ev{TONE_OFF, 1018, 0, 60}));
        // a single tone and a pair never match
        std::vector<uint32_t> m(3, rec(480));
        m.insert(m.end(), 6, rec(480, 620));
        const std::vector<Ev> mx = run_events(p, m, true);
        CHECK(mx.size() == 2 && mx[0] == (Ev{TONE_ON, 480, 620, 30}) && mx[1] == (Ev{TONE_OFF, 480, 620, 90}));
        CHECK(run_events(p, {}, true).empty() && run_events(p, {0u, rec(700)}, true).empty());
    }
    CHECK(std::strcmp(tone_name(350, 440, 20), "dial") == 0 && std::strcmp(tone_name(470, 630, 20), "busy") == 0 && std::strcmp(tone_name(425, 0, 1), "cp425") == 0);
    CHECK(std::strcmp(tone_name(1120, 0, 20), "cng") == 0 && tone_name(1121, 0, 20) == nullptr && tone_name(350, 0, 20) == nullptr && tone_name(425, 440, 200) != nullptr);
    CHECK(std::strcmp(tone_name(2100, 0, 5), "ced") == 0 && std::strcmp(tone_name(950, 0, 5), "sit1") == 0 && std::strcmp(tone_name(1400, 0, 5), "sit2") == 0 &&
          std::strcmp(tone_name(1800, 0, 5), "sit3") == 0);
    if (failures) { printf("%d checks FAILED\n", failures); return 1; }
    printf("all checks passed\n");
    return 0;
}
