// Stand-alone check of csrc/quality.h under AddressSanitizer + UBSan (tests/test_quality_cpu.py builds and runs it):
//   * the record of a hop from heap frames of exactly H samples (nothing behind the hop may be read), against a re-statement with
//     explicit loops, for random samples, zeros, a stuck value, the lowest sample throughout and alternating full scale, H = 80, 160, 480;
//   * clip runs at their edges: below and at clip_run_min, across samples 63 | 64, up to H - 1, L - 1 against L, -L, across a hop boundary;
//   * the machine on hand-derived sequences: ON at the first clipped frame, OFF exactly after the hold, a dropout one frame short, a
//     report interval a flush cuts short, a sequence cut at arbitrary points against the uncut run;
//   * option validation at its borders and the plan's frame counts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>
#include "quality.h"

using namespace aprilx;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Want { uint64_t sumsq; int64_t sum; int mn, mx; unsigned count, run; };
static Want restate(const std::vector<int16_t> &x, int L)
{
    Want w{0, 0, 32767, -32768, 0, 0};
    for (size_t i = 0; i < x.size(); ++i) {
        const int64_t v = x[i];
        w.sumsq += (uint64_t)(v * v); w.sum += v;
        if (v < w.mn) w.mn = (int)v;
        if (v > w.mx) w.mx = (int)v;
        w.count += (v >= L || v <= -L) ? 1u : 0u;
    }
    for (size_t i = 0; i < x.size(); ++i) {          // the longest run, by trying every start
        unsigned n = 0;
        while (i + n < x.size() && (x[i + n] >= L || x[i + n] <= -L)) ++n;
        if (n > w.run) w.run = n;
    }
    return w;
}

static std::vector<uint32_t> record_of(const std::vector<int16_t> &x, int L)
{
    std::unique_ptr<int16_t[]> heap(new int16_t[x.size()]);           // exactly the samples the record may read
    memcpy(heap.get(), x.data(), x.size() * sizeof(int16_t));
    std::vector<uint32_t> w(kQualityWords, 0xdeadbeefu);
    quality_frame(heap.get(), (int)x.size(), L, w.data());
    return w;
}

static void check_record(const std::vector<int16_t> &x, int L)
{
    const std::vector<uint32_t> w = record_of(x, L);
    const Want want = restate(x, L);
    CHECK(((uint64_t)w[0] | (uint64_t)w[1] << 32) == want.sumsq);
    CHECK((int32_t)w[2] == (int32_t)want.sum);
    CHECK((int16_t)(w[3] & 0xffffu) == want.mn && (int16_t)(w[3] >> 16) == want.mx);
    CHECK((w[4] & 0xffffu) == want.count && (w[4] >> 16) == want.run);
    CHECK(w[5] == (want.mn == want.mx ? 1u : 0u) && w[6] == 0u && w[7] == 0u);
}

static void records()
{
    std::mt19937 rng(7);
    for (int H : {80, 160, 480, 1, 63, 64, 65}) {
        std::vector<int16_t> x((size_t)H);
        for (int trial = 0; trial < 8; ++trial) {
            for (auto &v : x) v = (int16_t)(int)(rng() % 65536u - 32768u);
            for (int L : {32767, 32124, 1024}) check_record(x, L);
        }
        for (auto &v : x) v = (int16_t)((int)(rng() % 5u) - 2) * 16383;      // many clipped samples at L = 16383
        check_record(x, 16383);
        check_record(std::vector<int16_t>((size_t)H, 0), 32767);
        check_record(std::vector<int16_t>((size_t)H, 1234), 32767);
        check_record(std::vector<int16_t>((size_t)H, -32768), 32767);
        const std::vector<uint32_t> w = record_of(std::vector<int16_t>((size_t)H, -32768), 32767);
        CHECK(((uint64_t)w[0] | (uint64_t)w[1] << 32) == (uint64_t)H << 30 && w[3] == 0x80008000u && w[5] == 1u);
        for (int i = 0; i < H; ++i) x[(size_t)i] = (i & 1) ? -32767 : 32767;
        check_record(x, 32767);
    }
}

static void pair_of(int H, int L, int at, int n, int value, unsigned *count, unsigned *run)
{
    std::vector<int16_t> x((size_t)H, 0);
    for (int i = at; i < at + n; ++i) x[(size_t)i] = (int16_t)value;
    const std::vector<uint32_t> w = record_of(x, L);
    *count = w[4] & 0xffffu; *run = w[4] >> 16;
}

static void runs()
{
    const int L = 32124;
    for (int H : {80, 160, 480}) {
        unsigned c, r;
        pair_of(H, L, 5, 2, L, &c, &r); CHECK(c == 2 && r == 2);
        pair_of(H, L, 5, 3, L, &c, &r); CHECK(c == 3 && r == 3);
        pair_of(H, L, 61, 6, L, &c, &r); CHECK(c == 6 && r == 6);            // across samples 63 | 64
        pair_of(H, L, H - 2, 2, L, &c, &r); CHECK(c == 2 && r == 2);         // up to H - 1
        pair_of(H, L, 0, H, 32767, &c, &r); CHECK((int)c == H && (int)r == H);
        pair_of(H, L, 5, 3, L - 1, &c, &r); CHECK(c == 0 && r == 0);
        pair_of(H, L, 5, 3, -L, &c, &r); CHECK(c == 3 && r == 3);
        pair_of(H, L, 5, 3, -L + 1, &c, &r); CHECK(c == 0 && r == 0);
        // five clipped samples across the hop boundary: two shorter runs
        std::vector<int16_t> pcm((size_t)(2 * H), 0);
        for (int i = H - 3; i < H + 2; ++i) pcm[(size_t)i] = (int16_t)L;
        std::vector<uint32_t> w((size_t)(2 * kQualityWords));
        quality_run_host(H, L, 2, pcm.data(), (size_t)H, w.data());
        CHECK(w[4] == (3u | 3u << 16) && w[kQualityWords + 4] == (2u | 2u << 16));
    }
}

// records of a sequence: 'c' a frame with a run of three at full scale, 'd' zeros, 's' stuck at 77, '.' live and unclipped
static std::vector<uint32_t> synth(const char *spec, int H = 160)
{
    const size_t n = strlen(spec);
    std::vector<uint32_t> rec(n * kQualityWords);
    for (size_t i = 0; i < n; ++i) {
        std::vector<int16_t> x((size_t)H);
        for (int k = 0; k < H; ++k) x[(size_t)k] = (int16_t)((k * 37 + (int)i * 11) % 1999 - 999);
        if (spec[i] == 'c') { x[7] = x[8] = x[9] = 32767; }
        else if (spec[i] == 'd') std::fill(x.begin(), x.end(), (int16_t)0);
        else if (spec[i] == 's') std::fill(x.begin(), x.end(), (int16_t)77);
        quality_frame(x.data(), H, 32767, &rec[i * kQualityWords]);
    }
    return rec;
}

static QualityPlan plan_of(uint32_t hold_ms, uint32_t dropout_ms, uint32_t report_ms, uint32_t run_min = 3)
{
    QualityOptions o; o.clip_hold_ms = hold_ms; o.dropout_ms = dropout_ms; o.report_ms = report_ms; o.clip_run_min = run_min;
    QualityPlan p;
    CHECK(quality_make_plan(16000, 512, 10, o, &p));
    return p;
}

static std::vector<QualityEvent> events_of(const QualityPlan &p, const char *spec, uint64_t t0, bool flush, const std::vector<size_t> &cuts = {})
{
    const std::vector<uint32_t> rec = synth(spec);
    const size_t n = strlen(spec);
    std::vector<QualityEvent> out;
    auto emit = [&](const QualityEvent &e) { out.push_back(e); };
    QualityMachine m;
    size_t a = 0;
    for (size_t k = 0; k <= cuts.size(); ++k) {
        const size_t b = k < cuts.size() ? cuts[k] : n;
        std::unique_ptr<uint32_t[]> heap(new uint32_t[(b - a) * kQualityWords + 1]);      // exactly the records of the piece
        memcpy(heap.get(), rec.data() + a * kQualityWords, (b - a) * kQualityWords * sizeof(uint32_t));
        quality_events(p, 10, t0 + a, heap.get(), b - a, m, emit);
        a = b;
    }
    if (flush) {
        quality_flush(p, 10, t0 + n, m, emit);
        QualityMachine fresh;
        CHECK(memcmp(&m, &fresh, sizeof m) == 0);
    }
    return out;
}

static bool is(const QualityEvent &e, int kind, uint64_t ms) { return e.kind == kind && e.time_ms == ms; }

static void machine()
{
    {   // hold of 10 frames
        const QualityPlan p = plan_of(100, 200, 0);
        auto ev = events_of(p, "..c..........", 0, false);
        CHECK(ev.size() == 2 && is(ev[0], QUALITY_CLIPPING_ON, 20) && is(ev[1], QUALITY_CLIPPING_OFF, 30));
        ev = events_of(p, "..c.........", 0, false);
        CHECK(ev.size() == 1 && is(ev[0], QUALITY_CLIPPING_ON, 20));
        ev = events_of(p, "..c.........", 0, true);
        CHECK(ev.size() == 2 && is(ev[1], QUALITY_CLIPPING_OFF, 120));             // closed by the flush at frames_seen
    }
    {   // dropout of 20 frames
        const QualityPlan p = plan_of(100, 200, 0);
        auto ev = events_of(p, "..ddddddddddddddddddd..", 0, false);              // nineteen
        CHECK(ev.empty());
        ev = events_of(p, "..ddddddddddssssssssss.", 0, false, {7, 21});          // twenty, of two kinds
        CHECK(ev.size() == 2 && is(ev[0], QUALITY_DROPOUT_ON, 20) && is(ev[1], QUALITY_DROPOUT_OFF, 220));
    }
    {   // reports of 10 frames; the flush cuts the third short
        const QualityPlan p = plan_of(150, 20, 100);
        const char *spec = "..........cc......dd...";
        const auto ev = events_of(p, spec, 0, true, {4, 10, 19});
        const auto whole = events_of(p, spec, 0, true);
        CHECK(ev.size() == whole.size() && ev.size() == 7);
        for (size_t i = 0; i < ev.size() && i < whole.size(); ++i) CHECK(memcmp(&ev[i], &whole[i], sizeof ev[i]) == 0);
        if (ev.size() == 7) {
            CHECK(is(ev[0], QUALITY_REPORT, 0) && ev[0].frames == 10 && ev[0].clipped_frames == 0 && ev[0].hop == 160);
            CHECK(is(ev[1], QUALITY_CLIPPING_ON, 100) && is(ev[2], QUALITY_DROPOUT_ON, 180));
            CHECK(is(ev[3], QUALITY_REPORT, 100) && ev[3].frames == 10 && ev[3].clipped_frames == 2 && ev[3].dead_frames == 2 && ev[3].clip_samples == 6 && ev[3].max == 32767);
            CHECK(is(ev[4], QUALITY_DROPOUT_OFF, 200) && is(ev[5], QUALITY_CLIPPING_OFF, 230));
            CHECK(is(ev[6], QUALITY_REPORT, 200) && ev[6].frames == 3 && ev[6].quiet_sumsq > 0 && ev[6].quiet_sumsq <= ev[6].loud_sumsq);
        }
        const auto dead = events_of(p, "ssssssssss", 50, false);
        CHECK(dead.size() == 2 && is(dead[0], QUALITY_DROPOUT_ON, 500) && is(dead[1], QUALITY_REPORT, 500) && dead[1].quiet_sumsq == 0 &&
              dead[1].loud_sumsq == 160ull * 77 * 77 && dead[1].sum == 160 * 77 * 10 && dead[1].min == 77 && dead[1].max == 77);
    }
}

static void options()
{
    auto ok = [](uint32_t level, uint32_t run, uint32_t hold, uint32_t drop, uint32_t rep) {
        QualityOptions o; o.clip_level = level; o.clip_run_min = run; o.clip_hold_ms = hold; o.dropout_ms = drop; o.report_ms = rep;
        return quality_options_valid(o);
    };
    CHECK(ok(32767, 3, 1000, 200, 1000) && ok(1024, 1, 100, 20, 0) && ok(32767, 64, 60000, 60000, 60000) && ok(32124, 3, 1000, 200, 100));
    CHECK(!ok(1023, 3, 1000, 200, 1000) && !ok(32768, 3, 1000, 200, 1000) && !ok(32767, 0, 1000, 200, 1000) && !ok(32767, 65, 1000, 200, 1000));
    CHECK(!ok(32767, 3, 99, 200, 1000) && !ok(32767, 3, 60001, 200, 1000) && !ok(32767, 3, 1000, 19, 1000) && !ok(32767, 3, 1000, 60001, 1000));
    CHECK(!ok(32767, 3, 1000, 200, 99) && !ok(32767, 3, 1000, 200, 60001) && !ok(32767, 3, 1000, 200, 1));
    QualityOptions o; QualityPlan p;
    CHECK(quality_make_plan(16000, 512, 10, o, &p) && p.hop == 160 && p.hold_frames == 100 && p.dropout_frames == 20 && p.report_frames == 100);
    CHECK(quality_make_plan(8000, 256, 10, o, &p) && p.hop == 80);
    CHECK(quality_make_plan(48000, 2048, 10, o, &p) && p.hop == 480);
    o.dropout_ms = 20; o.report_ms = 0;
    CHECK(quality_make_plan(16000, 512, 30, o, &p) && p.hop == 480 && p.dropout_frames == 1 && p.report_frames == 0 && p.hold_frames == 33);
    CHECK(!quality_make_plan(16000, 100, 10, o, &p) && !quality_make_plan(0, 512, 10, o, &p) && !quality_make_plan(16000, 512, 0, o, &p));
    CHECK(!quality_make_plan(48000, 1 << 20, 1000, o, &p));                        // a hop beyond the 16-bit halves
}

int main()
{
    records();
    runs();
    machine();
    options();
    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    printf("all checks passed\n");
    return 0;
}
