// Stand-alone check of csrc/vad.h under AddressSanitizer + UBSan (tests/test_vad_cpu.py builds and runs it):
//   * hand-derived cases on a one-bin band with integer energies (the literal bytes of tests/golden/vad_cases.py);
//   * the band reduction from heap rows of exactly nbins floats, for bands with empty and unequal chains, against a re-statement
//     that walks the sixteen chains and the four folds with explicit indices;
//   * a sequence cut at arbitrary points and carried through the state against the uncut run;
//   * option validation at its borders, the plan from a small mel table, events from bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <utility>
#include <vector>
#include "vad.h"

using namespace aprilx;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static VadPlan one_bin(int onset, int hang, float min_energy = -100.0f)
{
    VadPlan p; p.b0 = 0; p.b1 = 1; p.inv_nb = 1.0f; p.thr_on = 2.0f; p.thr_off = 1.0f; p.min_energy = min_energy; p.onset_frames = onset; p.hangover_frames = hang;
    return p;
}

static std::vector<int> bytes_of(const VadPlan &p, const std::vector<float> &e, VadState *end = nullptr)
{
    VadState v;
    std::vector<uint8_t> b(e.size());
    std::vector<float> en(e.size());
    std::unique_ptr<float[]> rows(new float[e.size()]);           // exactly the floats the run may read
    for (size_t i = 0; i < e.size(); ++i) rows[i] = e[i];
    vad_run_host(p, (int)e.size(), rows.get(), 1, v, b.data(), en.data());
    for (size_t i = 0; i < e.size(); ++i) CHECK(en[i] == e[i]);
    if (end) *end = v;
    return std::vector<int>(b.begin(), b.end());
}

static void hand_cases()
{
    typedef std::vector<int> B;
    CHECK(bytes_of(one_bin(2, 2), {0, 8, 8}) == (B{0, 0, 2}));                                   // d == thr_on is not above it
    CHECK(bytes_of(one_bin(2, 2), {0, 16, 16, -17, 1}) == (B{0, 2, 3, 1, 0}));                   // d == thr_off; hangover reached
    CHECK(bytes_of(one_bin(3, 2), {0, 16, 16, 16}) == (B{0, 2, 2, 3}));                          // onset reached
    CHECK(bytes_of(one_bin(3, 2), {0, 16, 16, -13, 22}) == (B{0, 2, 2, 0, 2}));                  // one short
    CHECK(bytes_of(one_bin(2, 2), {0, 16, 16, -17, 17, -11, 1}) == (B{0, 2, 3, 1, 3, 1, 0}));    // hangover one short, then reached
    CHECK(bytes_of(one_bin(1, 1, -4.0f), {-10, 4}) == (B{0, 0}));                                // raised to min_energy
    CHECK(bytes_of(one_bin(1, 1), {16, 16}) == (B{0, 0}));                                       // first frame after a reset
    // s = 0 for 32 frames, then 8 (e = 32 once, then 8): speech until the 9th sub-window has overwritten the first
    std::vector<float> e(32, 0.0f);
    e.push_back(32.0f);
    for (int i = 0; i < 256; ++i) e.push_back(8.0f);
    B want(32, 0);
    for (int i = 0; i < 256; ++i) want.push_back(3);
    want.push_back(0);
    VadState v;
    CHECK(bytes_of(one_bin(1, 1), e, &v) == want);
    CHECK(v.pos == 1 && v.cnt == 1 && v.hist[0] == 8.0f && v.cur == 8.0f && v.st == 0 && v.first == 0);
}

static float band_restated(const VadPlan &p, const float *x)
{
    float c[16];
    for (int l = 0; l < 16; ++l) { c[l] = 0.0f; for (int k = 0; p.b0 + l + 16 * k < p.b1; ++k) c[l] = c[l] + x[p.b0 + l + 16 * k]; }
    for (int m = 8; m >= 1; m /= 2) { float t[16]; for (int l = 0; l < 16; ++l) t[l] = c[l] + c[l ^ m]; memcpy(c, t, sizeof c); }
    for (int l = 1; l < 16; ++l) CHECK(memcmp(&c[l], &c[0], 4) == 0);          // every lane holds the same bits
    return c[0] * p.inv_nb;
}

static void bands_and_cuts()
{
    std::mt19937 rng(16);
    std::normal_distribution<float> nd(-8.0f, 4.0f);
    const int nbins = 80;
    for (int nb : {1, 15, 16, 17, 54, 80}) {
        VadPlan p; p.b0 = (int)(rng() % (unsigned)(nbins - nb + 1)); p.b1 = p.b0 + nb; p.inv_nb = 1.0f / (float)nb;
        p.thr_on = 5.0f * kVadDbToLn; p.thr_off = 3.0f * kVadDbToLn; p.min_energy = -12.0f; p.onset_frames = 3; p.hangover_frames = 9;
        const int n = 400;
        std::unique_ptr<float[]> rows(new float[(size_t)n * nbins]);
        for (int i = 0; i < n; ++i) { const float lift = (i / 25) % 2 ? 6.0f : 0.0f; for (int j = 0; j < nbins; ++j) rows[(size_t)i * nbins + j] = nd(rng) + lift; }
        for (int i = 0; i < n; ++i) { const float a = vad_band_energy(p, &rows[(size_t)i * nbins]), b = band_restated(p, &rows[(size_t)i * nbins]); CHECK(memcmp(&a, &b, 4) == 0); }
        VadState whole; std::vector<uint8_t> wb((size_t)n);
        vad_run_host(p, n, rows.get(), nbins, whole, wb.data(), nullptr);
        int speech = 0; for (uint8_t x : wb) speech += x & 1;
        CHECK(speech > 0 && speech < n);
        VadState cut; std::vector<uint8_t> cb((size_t)n);
        for (int at = 0; at < n;) {
            const int len = std::min(n - at, 1 + (int)(rng() % 70u));
            vad_run_host(p, len, &rows[(size_t)at * nbins], nbins, cut, cb.data() + at, nullptr);
            at += len;
        }
        CHECK(wb == cb && memcmp(&whole, &cut, sizeof whole) == 0);
        vad_run_host(p, 0, nullptr, nbins, cut, nullptr, nullptr);               // a run of no rows reads nothing
        CHECK(memcmp(&whole, &cut, sizeof whole) == 0);
    }
}

static void options_plan_events()
{
    VadOptions o;
    CHECK(vad_options_valid(o, 16000) && !vad_options_valid(o, 7999) && vad_options_valid(o, 8000));
    VadOptions q = o; q.band_lo_hz = -1.0f; CHECK(!vad_options_valid(q, 16000));
    q = o; q.band_lo_hz = 4000.0f; CHECK(!vad_options_valid(q, 16000));
    q = o; q.offset_db = 0.0f; CHECK(!vad_options_valid(q, 16000));
    q = o; q.offset_db = 5.0f; CHECK(vad_options_valid(q, 16000)); q.offset_db = 5.5f; CHECK(!vad_options_valid(q, 16000));
    q = o; q.onset_db = 60.0f; CHECK(vad_options_valid(q, 16000)); q.onset_db = 60.5f; CHECK(!vad_options_valid(q, 16000));
    q = o; q.onset_ms = 9; CHECK(!vad_options_valid(q, 16000)); q.onset_ms = 1001; CHECK(!vad_options_valid(q, 16000));
    q = o; q.hangover_ms = 9; CHECK(!vad_options_valid(q, 16000)); q.hangover_ms = 10001; CHECK(!vad_options_valid(q, 16000));
    q = o; q.min_energy = __builtin_nanf(""); CHECK(!vad_options_valid(q, 16000));
    q = o; q.onset_db = __builtin_inff(); CHECK(!vad_options_valid(q, 16000));
    // peaks at fft bins 4, 8, ..., 32 of 64 at 6400 Hz: 200, 400, ..., 1600 Hz; the last row has two equal maxima (the first counts)
    const int nbins = 8, nfft = 64;
    std::unique_ptr<float[]> mel(new float[nbins * nfft]());
    for (int b = 0; b < nbins; ++b) for (int k = 4 * (b + 1) - 3; k <= 4 * (b + 1) + 3; ++k) mel[b * nfft + k] = 1.0f - (float)abs(k - 4 * (b + 1)) / 4.0f;
    mel[(nbins - 1) * nfft + 4 * nbins + 1] = 1.0f;
    VadPlan p;
    q = o; q.band_lo_hz = 201.0f; q.band_hi_hz = 1600.0f; q.onset_ms = 55; q.hangover_ms = 19;
    CHECK(vad_make_plan(mel.get(), nbins, nfft, 6400, 10, q, &p) && p.b0 == 1 && p.b1 == 8 && p.onset_frames == 5 && p.hangover_frames == 1);
    CHECK(p.inv_nb == 1.0f / 7.0f && p.thr_on == 5.0f * 0.23025851f && p.thr_off == 3.0f * 0.23025851f);
    q.band_lo_hz = 210.0f; q.band_hi_hz = 390.0f;
    CHECK(!vad_make_plan(mel.get(), nbins, nfft, 6400, 10, q, &p));
    // events
    VadPlan e = one_bin(2, 3);
    const uint8_t data[8] = {0, 2, 3, 3, 1, 1, 0, 0};
    std::vector<std::pair<int, uint64_t>> got;
    int last = vad_events(e, 10, 100, data, 8, 0, [&](int k, uint64_t ms) { got.emplace_back(k, ms); });
    CHECK(last == 0 && got.size() == 2 && got[0] == std::make_pair(1, (uint64_t)1010) && got[1] == std::make_pair(2, (uint64_t)1040));
    got.clear();
    last = vad_events(e, 10, 100, data, 4, 0, [&](int k, uint64_t ms) { got.emplace_back(k, ms); });
    CHECK(last == 1 && got.size() == 1);
    last = vad_events(e, 10, 104, nullptr, 0, last, [&](int k, uint64_t ms) { got.emplace_back(k, ms); });
    CHECK(last == 1 && got.size() == 1);
}

int main()
{
    hand_cases();
    bands_and_cuts();
    options_plan_events();
    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    printf("all checks passed\n");
    return 0;
}
