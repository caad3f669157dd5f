// Stand-alone check of csrc/staging_layout.h under AddressSanitizer + UBSan (tests/test_staging_layout_cpu.py builds and runs it).
// The oracle is the text Engine::fbank() held before the layout was stated once: its five offset formulas, its upload-length
// expression, its regrow condition, its five capacity updates and its capacity expression, restated literally below (with the
// descriptor sizes as constants, since the descriptor structs live in a HIP header).  Every field must be equal for all eight on/off
// combinations of the three passes, on counts that break every alignment, and along sequences of calls that grow the buffers.
// The old text knew no DTMF array: every comparison with it is a call with n_dt = 0, which must give what it always gave.  Calls with
// n_dt > 0 are held against what the layout promises instead: the array 16-byte aligned behind the VAD array, the upload ending where it
// ends, inside a buffer of `units`, and a regrow exactly when a count exceeds its capacity.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "staging_layout.h"

using namespace aprilx;

static int fails = 0;
static long checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { if (fails < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// the descriptor sizes of one sweep, under the names the old text used through sizeof()
static size_t S_FbankFrameDesc, S_ResampleDesc, S_DecodeDesc, S_VadDesc, S_DtmfDesc;

// ---- the old text: members ...
struct Old {
    int desc_cap_ = 0; size_t pcm_cap_ = 0, rs_cap_ = 0, dc_cap_ = 0, vd_cap_ = 0;
    size_t units = 0;                 // what the last regrow allocated
    // ... what one call computed
    bool regrew = false;
    size_t woff = 0, doff = 0, roff = 0, coff = 0, voff = 0, bytes = 0;

    void call(int n_frames, size_t n_pcm, int rs_n_, size_t rs_n_in_, int dc_n_, size_t dc_n_raw_, int vad_n_)
    {
        const int n_rs = n_frames > 0 ? std::max(rs_n_, 0) : 0;
        const size_t n_in = n_rs ? rs_n_in_ : 0;
        const int n_dc = n_frames > 0 ? std::max(dc_n_, 0) : 0;
        const size_t n_raw = n_dc ? dc_n_raw_ : 0;
        const size_t raw_units = n_dc ? (n_raw + 1) / 2 + 8 : 0;      // the raw region in int16 units, with its alignment
        const int n_vd = n_frames > 0 ? std::max(vad_n_, 0) : 0;
        regrew = false;
        if (n_frames > desc_cap_ || n_pcm + n_in + raw_units > pcm_cap_ || (size_t)n_rs > rs_cap_ || (size_t)n_dc > dc_cap_ || (size_t)n_vd > vd_cap_) {
            regrew = true;
            desc_cap_ = std::max({n_frames * 2, desc_cap_, 1024});
            pcm_cap_ = std::max({(n_pcm + n_in + raw_units) * 2, pcm_cap_, (size_t)1 << 16});
            rs_cap_ = std::max({(size_t)n_rs * 2, rs_cap_, n_rs ? (size_t)256 : (size_t)0});
            dc_cap_ = std::max({(size_t)n_dc * 2, dc_cap_, n_dc ? (size_t)256 : (size_t)0});
            vd_cap_ = std::max({(size_t)n_vd * 2, vd_cap_, n_vd ? (size_t)256 : (size_t)0});
            units = pcm_cap_ + 8 + ((size_t)desc_cap_ * S_FbankFrameDesc + 1) / 2 + 8 + rs_cap_ * S_ResampleDesc / 2
                    + 8 + dc_cap_ * S_DecodeDesc / 2 + 8 + vd_cap_ * S_VadDesc / 2;
        }
        woff = ((n_pcm + n_in) * sizeof(int16_t) + 15) / 16 * 16;          // byte offset of the raw region (empty without formatted sessions)
        doff = (woff + n_raw + 15) / 16 * 16;                              // ... of the descriptors
        roff = (doff + (size_t)n_frames * S_FbankFrameDesc + 15) / 16 * 16;      // ... of the resample descriptors
        coff = (roff + (size_t)n_rs * S_ResampleDesc + 15) / 16 * 16;            // ... and of the decode descriptors
        voff = (coff + (size_t)n_dc * S_DecodeDesc + 15) / 16 * 16;              // ... and of the VAD descriptors
        bytes = n_vd ? voff + (size_t)n_vd * S_VadDesc : n_dc ? coff + (size_t)n_dc * S_DecodeDesc
                     : (n_rs ? roff + (size_t)n_rs * S_ResampleDesc : doff + (size_t)n_frames * S_FbankFrameDesc);
    }
};

// ---- the new text, as Engine::fbank() uses it
struct New {
    StagingCaps caps; size_t units = 0; bool regrew = false; StagingLayout lay; StagingCounts cnt;
    void call(int n_frames, size_t n_pcm, int n_rs, size_t n_in, int n_dc, size_t n_raw, int n_vd, int n_dt = 0)
    {
        n_rs = std::max(n_rs, 0); n_dc = std::max(n_dc, 0); n_vd = std::max(n_vd, 0); n_dt = std::max(n_dt, 0);
        cnt = StagingCounts();
        cnt.n_pcm = n_pcm; cnt.n_in = n_rs ? n_in : 0; cnt.n_raw = n_dc ? n_raw : 0;
        cnt.n[ST_FRAMES] = (size_t)n_frames; cnt.n[ST_RS] = (size_t)n_rs; cnt.n[ST_DC] = (size_t)n_dc; cnt.n[ST_VD] = (size_t)n_vd; cnt.n[ST_DT] = (size_t)n_dt;
        const StagingSizes el{S_FbankFrameDesc, S_ResampleDesc, S_DecodeDesc, S_VadDesc, S_DtmfDesc};
        lay = staging_layout(cnt, el);
        regrew = !caps.holds(cnt, lay);
        if (regrew) { caps.grow(cnt, lay); units = caps.units(el); }
    }
};

static void compare(const Old &o, const New &n)
{
    CHECK(o.woff == n.lay.raw); CHECK(o.doff == n.lay.off[ST_FRAMES]); CHECK(o.roff == n.lay.off[ST_RS]); CHECK(o.coff == n.lay.off[ST_DC]); CHECK(o.voff == n.lay.off[ST_VD]);
    CHECK(o.bytes == n.lay.bytes);
    CHECK(o.regrew == n.regrew); CHECK(o.units == n.units);
    CHECK((size_t)o.desc_cap_ == n.caps.n[ST_FRAMES]); CHECK(o.pcm_cap_ == n.caps.pcm_units); CHECK(o.rs_cap_ == n.caps.n[ST_RS]); CHECK(o.dc_cap_ == n.caps.n[ST_DC]); CHECK(o.vd_cap_ == n.caps.n[ST_VD]);
    CHECK(n.lay.bytes <= n.units * 2);                  // the upload fits the buffers
    CHECK(n.lay.raw % 16 == 0 && n.lay.off[ST_FRAMES] % 16 == 0 && n.lay.off[ST_RS] % 16 == 0 && n.lay.off[ST_DC] % 16 == 0 && n.lay.off[ST_VD] % 16 == 0);
}

// a call with DTMF descriptors, `before` the capacities it met
static void check_dt(const New &n, const StagingCaps &before)
{
    const StagingCounts &c = n.cnt;
    CHECK(c.n[ST_DT] > 0);
    CHECK(n.lay.off[ST_DT] % 16 == 0 && n.lay.off[ST_DT] >= n.lay.off[ST_VD] + c.n[ST_VD] * S_VadDesc && n.lay.off[ST_DT] < n.lay.off[ST_VD] + c.n[ST_VD] * S_VadDesc + 16);
    CHECK(n.lay.bytes == n.lay.off[ST_DT] + c.n[ST_DT] * S_DtmfDesc);
    CHECK(n.lay.bytes <= n.lay.units * 2);              // a buffer of exactly these counts holds the upload ...
    CHECK(n.lay.bytes <= n.units * 2);                  // ... and so do the buffers as they are after the call
    const bool exceeds = c.n[ST_FRAMES] > before.n[ST_FRAMES] || n.lay.pcm_units > before.pcm_units || c.n[ST_RS] > before.n[ST_RS] || c.n[ST_DC] > before.n[ST_DC] ||
                         c.n[ST_VD] > before.n[ST_VD] || c.n[ST_DT] > before.n[ST_DT];
    CHECK(n.regrew == exceeds);
    CHECK(n.caps.holds(c, n.lay));
    if (!n.regrew)
        CHECK(n.caps.n[ST_FRAMES] == before.n[ST_FRAMES] && n.caps.pcm_units == before.pcm_units && n.caps.n[ST_RS] == before.n[ST_RS] && n.caps.n[ST_DC] == before.n[ST_DC] &&
              n.caps.n[ST_VD] == before.n[ST_VD] && n.caps.n[ST_DT] == before.n[ST_DT]);
    else
        CHECK(n.caps.n[ST_FRAMES] >= before.n[ST_FRAMES] && n.caps.pcm_units >= before.pcm_units && n.caps.n[ST_RS] >= before.n[ST_RS] && n.caps.n[ST_DC] >= before.n[ST_DC] &&
              n.caps.n[ST_VD] >= before.n[ST_VD] && n.caps.n[ST_DT] >= std::max(before.n[ST_DT], c.n[ST_DT]));
}

int main()
{
    const size_t sizes[][5] = {{12, 64, 24, 48, 64}, {16, 56, 20, 44, 40}, {13, 6, 2, 10, 7}};      // (even sizes as the structs have them, and sizes that divide nothing)
    const size_t pcm[] = {400, 401, 65535, 70001};
    const size_t in[] = {0, 1, 882, 883};
    const size_t raw[] = {0, 1, 15, 16, 17};
    const int frames[] = {1, 3};
    const int descs[] = {0, 1, 5};
    for (const auto &sz : sizes) {
        S_FbankFrameDesc = sz[0]; S_ResampleDesc = sz[1]; S_DecodeDesc = sz[2]; S_VadDesc = sz[3]; S_DtmfDesc = sz[4];
        // every call on fresh buffers: all eight on/off combinations are among the descriptor counts {0, 1, 5}^3
        for (size_t n_pcm : pcm) for (size_t n_in : in) for (size_t n_raw : raw) for (int n_frames : frames)
            for (int n_rs : descs) for (int n_dc : descs) for (int n_vd : descs) {
                Old o; New n;
                o.call(n_frames, n_pcm, n_rs, n_in, n_dc, n_raw, n_vd);
                n.call(n_frames, n_pcm, n_rs, n_in, n_dc, n_raw, n_vd);
                compare(o, n);
                CHECK(((n_pcm + (n_rs ? n_in : 0)) & 1) == 0 || n.lay.raw != (n_pcm + (n_rs ? n_in : 0)) * 2);      // (odd sample counts do leave a gap)
                for (int n_dt : {1, 5}) {                // the same call with DTMF descriptors: nothing in front of them moves
                    New d;
                    d.call(n_frames, n_pcm, n_rs, n_in, n_dc, n_raw, n_vd, n_dt);
                    check_dt(d, StagingCaps());
                    CHECK(d.lay.raw == n.lay.raw && d.lay.off[ST_FRAMES] == n.lay.off[ST_FRAMES] && d.lay.off[ST_RS] == n.lay.off[ST_RS] && d.lay.off[ST_DC] == n.lay.off[ST_DC] && d.lay.off[ST_VD] == n.lay.off[ST_VD]);
                    CHECK(d.lay.pcm_units == n.lay.pcm_units && d.caps.n[ST_DT] == 256 && d.units > n.units);
                }
            }
        // one pair of buffers through a sequence of calls: passes come and go, counts cross the floors and the doubled capacities
        Old o; New n;
        unsigned s = 12345u;
        auto rnd = [&s](unsigned m) { s = s * 1664525u + 1013904223u; return (s >> 8) % m; };
        int regrows = 0;
        for (int i = 0; i < 4000; ++i) {
            const int scale = 1 << rnd(12);
            const int n_frames = 1 + (int)rnd(3u * (unsigned)scale);
            const size_t n_pcm = 1 + rnd(400u * (unsigned)scale);
            const int n_rs = rnd(2) ? (int)rnd((unsigned)scale) : 0, n_dc = rnd(2) ? (int)rnd((unsigned)scale) : 0, n_vd = rnd(2) ? (int)rnd((unsigned)scale) : 0;
            const size_t n_in = rnd(900u * (unsigned)scale), n_raw = rnd(1700u * (unsigned)scale);
            o.call(n_frames, n_pcm, n_rs, n_in, n_dc, n_raw, n_vd);
            n.call(n_frames, n_pcm, n_rs, n_in, n_dc, n_raw, n_vd);
            compare(o, n);
            regrows += o.regrew;
        }
        CHECK(regrows > 5);
        // the same sweep with DTMF passes that come and go; calls without one must still upload what the old text uploaded
        New d; Old od;
        int dt_regrows = 0, dt_calls = 0;
        for (int i = 0; i < 4000; ++i) {
            const int scale = 1 << rnd(12);
            const int n_frames = 1 + (int)rnd(3u * (unsigned)scale);
            const size_t n_pcm = 1 + rnd(400u * (unsigned)scale);
            const int n_rs = rnd(2) ? (int)rnd((unsigned)scale) : 0, n_dc = rnd(2) ? (int)rnd((unsigned)scale) : 0, n_vd = rnd(2) ? (int)rnd((unsigned)scale) : 0;
            const int n_dt = rnd(2) ? 1 + (int)rnd((unsigned)scale) : 0;
            const size_t n_in = rnd(900u * (unsigned)scale), n_raw = rnd(1700u * (unsigned)scale);
            const StagingCaps before = d.caps;
            d.call(n_frames, n_pcm, n_rs, n_in, n_dc, n_raw, n_vd, n_dt);
            if (n_dt) { check_dt(d, before); ++dt_calls; dt_regrows += d.regrew && (size_t)n_dt > before.n[ST_DT]; }
            else {
                od.call(n_frames, n_pcm, n_rs, n_in, n_dc, n_raw, n_vd);
                CHECK(od.woff == d.lay.raw && od.doff == d.lay.off[ST_FRAMES] && od.roff == d.lay.off[ST_RS] && od.coff == d.lay.off[ST_DC] && od.voff == d.lay.off[ST_VD] && od.bytes == d.lay.bytes);
                CHECK(d.lay.bytes <= d.units * 2);
            }
        }
        CHECK(dt_calls > 1000 && dt_regrows > 2);
    }
    if (fails) { printf("%d of %ld checks FAILED\n", fails, checks); return 1; }
    printf("all checks passed (%ld)\n", checks);
    return 0;
}
