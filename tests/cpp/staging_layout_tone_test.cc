// csrc/staging_layout.h with its sixth array, the tone descriptors, as a stand-alone program under AddressSanitizer + UBSan
// (tests/test_tone_cpu.py builds and runs it).  The oracle for calls WITHOUT tone descriptors is the five-array layout, restated below
// from its own rules (each array 16-byte aligned behind what precedes it; the upload ends with the last array the call uses; 8 units
// per array for the first four always, for the fifth once it has elements): offsets, upload length and capacities must be equal for the
// count sets tests/cpp/staging_layout_test.cc walks.  Calls WITH tone descriptors are held against what the layout promises: the sixth
// array 16-byte aligned behind the fifth, nothing in front of it moved, the upload ending where it ends, inside the buffer.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include "staging_layout.h"

using namespace aprilx;

static int fails = 0;
static long checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { if (fails < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// ---- the five-array layout
struct Five {
    size_t raw = 0, off[5] = {0, 0, 0, 0, 0}, bytes = 0, pcm_units = 0, units = 0;
    size_t cap[5] = {0, 0, 0, 0, 0}, cap_pcm = 0, cap_units = 0;
    bool regrew = false;
    void call(const size_t n[5], const size_t el[5], size_t n_pcm, size_t n_in, size_t n_raw)
    {
        auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
        raw = up16((n_pcm + n_in) * 2);
        size_t end = raw + n_raw;
        for (int i = 0; i < 5; ++i) {
            off[i] = up16(end);
            end = off[i] + n[i] * el[i];
            if (i == 0 || n[i]) bytes = end;
        }
        pcm_units = n_pcm + n_in + (n[2] ? (n_raw + 1) / 2 + 8 : 0);
        units = pcm_units;
        for (int i = 0; i < 5; ++i) if (i < 4 || n[i]) units += 8 + (n[i] * el[i] + 1) / 2;
        regrew = pcm_units > cap_pcm;
        for (int i = 0; i < 5; ++i) regrew = regrew || n[i] > cap[i];
        if (regrew) {
            cap[0] = std::max({n[0] * 2, cap[0], (size_t)1024});
            cap_pcm = std::max({pcm_units * 2, cap_pcm, (size_t)1 << 16});
            for (int i = 1; i < 5; ++i) cap[i] = std::max({n[i] * 2, cap[i], n[i] ? (size_t)256 : (size_t)0});
            cap_units = cap_pcm;
            for (int i = 0; i < 5; ++i) if (i < 4 || cap[i]) cap_units += 8 + (cap[i] * el[i] + 1) / 2;
        }
    }
};

struct Six {
    StagingCaps caps; size_t units = 0; bool regrew = false; StagingLayout lay; StagingCounts cnt;
    void call(const size_t n[5], size_t n_tn, const size_t el[6], size_t n_pcm, size_t n_in, size_t n_raw)
    {
        cnt = StagingCounts();
        cnt.n_pcm = n_pcm; cnt.n_in = n_in; cnt.n_raw = n_raw;
        cnt.n[ST_FRAMES] = n[0]; cnt.n[ST_RS] = n[1]; cnt.n[ST_DC] = n[2]; cnt.n[ST_VD] = n[3]; cnt.n[ST_DT] = n[4]; cnt.n[ST_TN] = n_tn;
        StagingSizes s{};
        s[ST_FRAMES] = el[0]; s[ST_RS] = el[1]; s[ST_DC] = el[2]; s[ST_VD] = el[3]; s[ST_DT] = el[4]; s[ST_TN] = el[5];
        lay = staging_layout(cnt, s);
        regrew = !caps.holds(cnt, lay);
        if (regrew) { caps.grow(cnt, lay); units = caps.units(s); }
    }
};

static void same(const Five &o, const Six &n)
{
    CHECK(o.raw == n.lay.raw && o.off[0] == n.lay.off[ST_FRAMES] && o.off[1] == n.lay.off[ST_RS] && o.off[2] == n.lay.off[ST_DC] && o.off[3] == n.lay.off[ST_VD] && o.off[4] == n.lay.off[ST_DT]);
    CHECK(o.bytes == n.lay.bytes && o.pcm_units == n.lay.pcm_units && o.units == n.lay.units);
    CHECK(o.regrew == n.regrew && o.cap_units == n.units);
    CHECK(o.cap[0] == n.caps.n[ST_FRAMES] && o.cap_pcm == n.caps.pcm_units && o.cap[1] == n.caps.n[ST_RS] && o.cap[2] == n.caps.n[ST_DC] && o.cap[3] == n.caps.n[ST_VD] && o.cap[4] == n.caps.n[ST_DT]);
    CHECK(n.caps.n[ST_TN] == 0);
}

int main()
{
    const size_t sizes[][6] = {{12, 64, 24, 48, 64, 64}, {16, 56, 20, 44, 40, 72}, {13, 6, 2, 10, 7, 5}};
    const size_t pcm[] = {400, 401, 65535, 70001};
    const size_t in[] = {0, 1, 882, 883};
    const size_t raw[] = {0, 1, 15, 16, 17};
    const size_t frames[] = {1, 3};
    const size_t descs[] = {0, 1, 5};
    for (const auto &el : sizes) {
        for (size_t n_pcm : pcm) for (size_t n_in : in) for (size_t n_raw : raw) for (size_t n_frames : frames)
            for (size_t n_rs : descs) for (size_t n_dc : descs) for (size_t n_vd : descs) for (size_t n_dt : descs) {
                const size_t n[5] = {n_frames, n_rs, n_dc, n_vd, n_dt};
                const size_t use_in = n_rs ? n_in : 0, use_raw = n_dc ? n_raw : 0;
                Five o; Six s;
                o.call(n, el, n_pcm, use_in, use_raw);
                s.call(n, 0, el, n_pcm, use_in, use_raw);
                same(o, s);
                for (size_t n_tn : {(size_t)1, (size_t)5}) {
                    Six t;
                    t.call(n, n_tn, el, n_pcm, use_in, use_raw);
                    CHECK(t.lay.raw == s.lay.raw && t.lay.off[ST_FRAMES] == s.lay.off[ST_FRAMES] && t.lay.off[ST_RS] == s.lay.off[ST_RS] && t.lay.off[ST_DC] == s.lay.off[ST_DC] && t.lay.off[ST_VD] == s.lay.off[ST_VD] && t.lay.off[ST_DT] == s.lay.off[ST_DT]);
                    const size_t end5 = t.lay.off[ST_DT] + n_dt * el[4];
                    CHECK(t.lay.off[ST_TN] % 16 == 0 && t.lay.off[ST_TN] >= end5 && t.lay.off[ST_TN] < end5 + 16);
                    CHECK(t.lay.bytes == t.lay.off[ST_TN] + n_tn * el[5]);
                    CHECK(t.lay.pcm_units == s.lay.pcm_units && t.lay.units > s.lay.units);
                    CHECK(t.lay.bytes <= t.lay.units * 2 && t.lay.bytes <= t.units * 2);
                    CHECK(t.regrew && t.caps.n[ST_TN] == 256 && t.caps.holds(t.cnt, t.lay) && t.units > s.units);
                    CHECK(t.caps.n[ST_FRAMES] == s.caps.n[ST_FRAMES] && t.caps.pcm_units == s.caps.pcm_units && t.caps.n[ST_RS] == s.caps.n[ST_RS] && t.caps.n[ST_DC] == s.caps.n[ST_DC] &&
                          t.caps.n[ST_VD] == s.caps.n[ST_VD] && t.caps.n[ST_DT] == s.caps.n[ST_DT]);
                }
            }
        // one pair of buffers through a sequence of calls in which tone passes come and go: a call without one uploads what the
        // five-array layout uploads, from the same offsets
        Six s; Five o;
        unsigned seed = 4321u;
        auto rnd = [&seed](unsigned m) { seed = seed * 1664525u + 1013904223u; return (size_t)((seed >> 8) % m); };
        int tone_calls = 0, tone_regrows = 0;
        for (int i = 0; i < 4000; ++i) {
            const unsigned scale = 1u << rnd(12);
            const size_t n[5] = {1 + rnd(3u * scale), rnd(2) ? rnd(scale) : 0, rnd(2) ? rnd(scale) : 0, rnd(2) ? rnd(scale) : 0, rnd(2) ? rnd(scale) : 0};
            const size_t n_tn = rnd(2) ? 1 + rnd(scale) : 0;
            const size_t n_pcm = 1 + rnd(400u * scale), n_in = n[1] ? rnd(900u * scale) : 0, n_raw = n[2] ? rnd(1700u * scale) : 0;
            const StagingCaps before = s.caps;
            s.call(n, n_tn, el, n_pcm, n_in, n_raw);
            o.call(n, el, n_pcm, n_in, n_raw);
            CHECK(o.raw == s.lay.raw && o.off[0] == s.lay.off[ST_FRAMES] && o.off[1] == s.lay.off[ST_RS] && o.off[2] == s.lay.off[ST_DC] && o.off[3] == s.lay.off[ST_VD] && o.off[4] == s.lay.off[ST_DT]);
            CHECK(s.lay.bytes <= s.units * 2 && s.caps.holds(s.cnt, s.lay));
            if (!n_tn) CHECK(o.bytes == s.lay.bytes);
            else {
                ++tone_calls; tone_regrows += s.regrew && n_tn > before.n[ST_TN];
                CHECK(s.lay.off[ST_TN] % 16 == 0 && s.lay.off[ST_TN] >= o.off[4] + n[4] * el[4] && s.lay.bytes == s.lay.off[ST_TN] + n_tn * el[5]);
                CHECK(s.caps.n[ST_TN] >= std::max(before.n[ST_TN], n_tn));
            }
        }
        CHECK(tone_calls > 1000 && tone_regrows > 2);
    }
    if (fails) { printf("%d of %ld checks FAILED\n", fails, checks); return 1; }
    printf("all checks passed (%ld)\n", checks);
    return 0;
}
