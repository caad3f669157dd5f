// Tone events per session (include/aprilx_engine.h "Tones"): ON / OFF events for sustained single tones and tone
// pairs -- call-progress tones, fax CNG / CED, the beep of an answering machine, the segments of a special-information tone -- from the
// model-rate samples the filterbank reads.  This is the contract in plain C++ -- kernels_tone.hip is the device half and gives the same
// bits -- : the accepted options, the plan derived from them, the tables, steps 1-7 over an array of frames, and the events that follow
// from the records.  Header-only on purpose, as dtmf.h is: the scheduler harness builds session.cc without further files, and
// tests/cpp/tone_test.cc builds it alone under the sanitizers.
//
// All arithmetic is fp32, never contracted (-ffp-contract=off), in exactly the order written; division and square root are correctly
// rounded.  The frame is the filterbank's own; the detector reads its first W = 64 * floor(fft_size / 64) samples x[0 .. W) (int16).
// The grid is the DFT bins k_lo .. k_hi of length W: k_lo = ceil(300 W / rate), k_hi = min(floor(2300 W / rate), W / 2 - 1),
// F = k_hi - k_lo + 1.  Tables T[2F][W]: row k cos(2 pi m / W), row F + k sin(2 pi m / W) with the integer m = ((k_lo + k) j) mod W,
// computed in double and rounded once.  Per real frame:
//   1  per table row 64 chains a[l] = 0.0f + float(x[l]) * T[l] + float(x[l + 64]) * T[l + 64] + ... (multiply then add, increasing
//      index), then a[l] = a[l] + a[l ^ m] for m = 32, 16, 8, 4, 2, 1 (IEEE addition commutes: every lane holds the same bits);
//      re = a[0] of row k, im = a[0] of row F + k;  P[k] = re * re + im * im
//   2  E = float(sum x[j]^2), the sum exact in 64-bit integers;  half_w = 0.5f * float(W)
//   3  p = first maximum of P[0..F), P1 = P[p];  !(P1 >= min_power) -> the record is (0, 0)
//   4  q = first maximum over the bins with |k - p| >= 3, P2 = P[q];  dual = !(P2 * second_ratio < P1)
//   5  S = the fp32 sum, from 0.0f in increasing bin order, of P over {p-1, p, p+1} and for a pair also {q-1, q, q+1}, each clipped to
//      the grid (disjoint: the lower group first);  S < min_share * (E * half_w) -> the record is (0, 0)
//   6  the frequency of a component at bin c, l and r its neighbours' powers (0 outside the grid):
//        r >= l: s = sqrtf(r / P[c]), d = s / (1.0f + s);  else s = sqrtf(l / P[c]), d = -(s / (1.0f + s))
//        hz = int((float(k_lo + c) + d) * bin_hz + 0.5f), bin_hz = float(rate) / float(W)
//      (a value that is no number inside 1 .. 65535 -- it takes a NaN or an infinity among the powers -- makes the record (0, 0))
//   7  the record: two uint16, (hz, 0) for a single tone, the two values in ascending order for a pair.  No state on the device.
// Written so that NaN and exact ties fall the same way everywhere.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define APRILX_TONE_HD __host__ __device__
#else
#define APRILX_TONE_HD
#endif

namespace aprilx {

constexpr int kToneLanes = 64, kToneMaxW = 4096, kToneMinF = 8, kToneMaxF = 128, kToneGuard = 3;

// the option values (the public AprilxToneOptions without its size and flags)
struct ToneOptions {
    float min_level_dbfs = -40.0f, second_db = 10.0f, min_share = 0.7f;
    uint32_t tol_hz = 20, min_tone_ms = 60, min_pause_ms = 30;
};
// what the kernel and the event machine need of them, 48 bytes (the layout of the public AprilxTonePlan)
struct TonePlan {
    int32_t W = 0, k_lo = 0, F = 0;
    float half_w = 0, min_power = 0, second_ratio = 0, min_share = 0, bin_hz = 0;
    int32_t tol_hz = 0, on_frames = 1, off_frames = 1, reserved = 0;
};
static_assert(sizeof(TonePlan) == 48, "layout shared with the device and the C ABI");
// the host's event machine, integers only: held (0 idle, 1 a tone is on) with its reference h1, h2; the candidate's reference c1, c2
// and the length of the current run (idle: matching frames; held: frames that do not match)
struct ToneMachine { int32_t held = 0, h1 = 0, h2 = 0, c1 = 0, c2 = 0, run = 0; };

enum : int { TONE_ON = 1, TONE_OFF = 2 };

inline bool tone_options_valid(const ToneOptions &o)
{
    auto in = [](float v, float lo, float hi) { return std::isfinite(v) && v >= lo && v <= hi; };
    if (!in(o.min_level_dbfs, -70.0f, 0.0f) || !in(o.second_db, 3.0f, 30.0f)) return false;
    if (!(std::isfinite(o.min_share) && o.min_share > 0.0f && o.min_share <= 1.0f)) return false;
    return o.tol_hz >= 1u && o.tol_hz <= 200u && o.min_tone_ms >= 10u && o.min_tone_ms <= 5000u && o.min_pause_ms >= 10u && o.min_pause_ms <= 5000u;
}

// W, k_lo and F of a model; false when the model is refused: a window shorter than 20 ms, a rate below 6000 Hz, a window beyond
// kToneMaxW, or a grid of fewer than 8 or more than 128 bins
inline bool tone_grid(int rate, int fft_size, int *w_out, int *k_lo_out, int *f_out)
{
    if (rate < 6000 || fft_size < kToneLanes) return false;
    const int64_t w = (int64_t)kToneLanes * (fft_size / kToneLanes);
    if (w * 1000 < (int64_t)20 * rate || w > kToneMaxW) return false;
    const int64_t k_lo = (300 * w + rate - 1) / rate;
    int64_t k_hi = 2300 * w / rate;
    if (k_hi > w / 2 - 1) k_hi = w / 2 - 1;
    const int64_t f = k_hi - k_lo + 1;
    if (f < kToneMinF || f > kToneMaxF) return false;
    *w_out = (int)w; *k_lo_out = (int)k_lo; *f_out = (int)f;
    return true;
}

// The plan, derived once in double and rounded once.  False: options out of range, or a refused model.
inline bool tone_make_plan(int rate, int fft_size, int shift_ms, const ToneOptions &o, TonePlan *out)
{
    int w, k_lo, f;
    if (shift_ms <= 0 || !tone_options_valid(o) || !tone_grid(rate, fft_size, &w, &k_lo, &f)) return false;
    TonePlan p;
    p.W = w; p.k_lo = k_lo; p.F = f;
    p.half_w = 0.5f * (float)w;
    const double amp = 32768.0 * std::pow(10.0, (double)o.min_level_dbfs / 20.0) * (double)w / 2.0;
    p.min_power = (float)(amp * amp);
    p.second_ratio = (float)std::pow(10.0, (double)o.second_db / 10.0);
    p.min_share = o.min_share;
    p.bin_hz = (float)rate / (float)w;
    p.tol_hz = (int32_t)o.tol_hz;
    p.on_frames = (int32_t)(o.min_tone_ms / (uint32_t)shift_ms); if (p.on_frames < 1) p.on_frames = 1;
    p.off_frames = (int32_t)(o.min_pause_ms / (uint32_t)shift_ms); if (p.off_frames < 1) p.off_frames = 1;
    *out = p;
    return true;
}

// the tables [2F][W]
inline void tone_make_tables(int w, int k_lo, int f, float *out)
{
    for (int k = 0; k < f; ++k)
        for (int j = 0; j < w; ++j) {
            const int64_t m = ((int64_t)(k_lo + k) * (int64_t)j) % (int64_t)w;
            const double a = 2.0 * 3.14159265358979323846 * (double)m / (double)w;
            out[(size_t)k * (size_t)w + (size_t)j] = (float)std::cos(a);
            out[(size_t)(f + k) * (size_t)w + (size_t)j] = (float)std::sin(a);
        }
}

// step 6 for the component at bin c; 0: no frequency
APRILX_TONE_HD inline uint32_t tone_hz(const TonePlan &p, const float *P, int c)
{
    const float l = c > 0 ? P[c - 1] : 0.0f, r = c + 1 < p.F ? P[c + 1] : 0.0f;
    float d;
    if (r >= l) { const float q = r / P[c]; const float s = sqrtf(q); const float u = 1.0f + s; d = s / u; }
    else { const float q = l / P[c]; const float s = sqrtf(q); const float u = 1.0f + s; const float v = s / u; d = -v; }
    const float k = (float)(p.k_lo + c) + d;
    const float h = k * p.bin_hz;
    const float v = h + 0.5f;
    return v >= 1.0f && v < 65536.0f ? (uint32_t)(int)v : 0u;
}

// steps 3-7 on the F powers and the energy; returns the record as lo | hi << 16 (the two uint16 in memory order)
APRILX_TONE_HD inline uint32_t tone_decide(const TonePlan &p, const float *P, float E)
{
    int a = 0;
    for (int i = 1; i < p.F; ++i) if (P[i] > P[a]) a = i;
    const float p1 = P[a];
    if (!(p1 >= p.min_power)) return 0u;
    int b = -1;
    for (int i = 0; i < p.F; ++i) {
        if (i > a - kToneGuard && i < a + kToneGuard) continue;
        if (b < 0 || P[i] > P[b]) b = i;
    }
    bool dual = false;
    if (b >= 0) { const float t = P[b] * p.second_ratio; dual = !(t < p1); }
    const int lo = dual && b < a ? b : a, hi = dual ? (b < a ? a : b) : -1;
    float s = 0.0f;
    for (int i = lo - 1; i <= lo + 1; ++i) if (i >= 0 && i < p.F) s = s + P[i];
    if (dual) for (int i = hi - 1; i <= hi + 1; ++i) if (i >= 0 && i < p.F) s = s + P[i];
    const float eh = E * p.half_w;
    const float need = p.min_share * eh;
    if (s < need) return 0u;
    const uint32_t f1 = tone_hz(p, P, lo);
    if (!f1) return 0u;
    if (!dual) return f1;
    const uint32_t f2 = tone_hz(p, P, hi);
    if (!f2) return 0u;
    return f1 <= f2 ? f1 | f2 << 16 : f2 | f1 << 16;
}

// steps 1 and 2 of one frame: P[0..F) and E into out (F + 1 values)
inline void tone_powers(const TonePlan &p, const float *tables, const int16_t *x, float *out)
{
    float c[kToneLanes], t[kToneLanes], sum[2];
    for (int k = 0; k < p.F; ++k) {
        for (int part = 0; part < 2; ++part) {
            const float *T = tables + (size_t)(part * p.F + k) * (size_t)p.W;
            for (int l = 0; l < kToneLanes; ++l) {
                c[l] = 0.0f;
                for (int j = l; j < p.W; j += kToneLanes) { const float m = (float)x[j] * T[j]; c[l] = c[l] + m; }
            }
            for (int m = kToneLanes / 2; m >= 1; m >>= 1) {
                for (int l = 0; l < kToneLanes; ++l) t[l] = c[l] + c[l ^ m];
                for (int l = 0; l < kToneLanes; ++l) c[l] = t[l];
            }
            sum[part] = c[0];
        }
        const float rr = sum[0] * sum[0], ii = sum[1] * sum[1];
        out[k] = rr + ii;
    }
    int64_t e = 0;
    for (int j = 0; j < p.W; ++j) e += (int64_t)x[j] * (int64_t)x[j];
    out[p.F] = (float)e;
}

// n frames (frame i at frames + i * ld, W samples read of each) through steps 1-7; records_out [n] (lo | hi << 16); powers_out (may be
// null) receives [n][F + 1]
inline void tone_run_host(const TonePlan &p, const float *tables, int n, const int16_t *frames, size_t ld, uint32_t *records_out, float *powers_out)
{
    float q[kToneMaxF + 1];
    for (int i = 0; i < n; ++i) {
        tone_powers(p, tables, frames + (size_t)i * ld, q);
        if (powers_out) for (int k = 0; k <= p.F; ++k) powers_out[(size_t)i * (size_t)(p.F + 1) + (size_t)k] = q[k];
        records_out[i] = tone_decide(p, q, q[p.F]);
    }
}

// two tonal records match: both single or both pairs, and each frequency within tol_hz
inline bool tone_match(int32_t a1, int32_t a2, int32_t b1, int32_t b2, int32_t tol)
{
    if ((a2 != 0) != (b2 != 0)) return false;
    const int32_t d1 = a1 > b1 ? a1 - b1 : b1 - a1, d2 = a2 > b2 ? a2 - b2 : b2 - a2;
    return d1 <= tol && d2 <= tol;
}

// Events from the records of consecutive real frames: record i is frame t0 + i of the session.
//   idle: a tonal frame opens a candidate run with its record as the reference; on_frames consecutive frames that match the reference
//         -> ON(f1, f2) with the frequencies of the frame that completed the run (they become the held reference) at
//         (t - on_frames + 1) * shift_ms; a tonal frame that does not match restarts the run with itself
//   held: off_frames consecutive frames that do not match the held reference -> OFF(f1, f2) at (t - off_frames + 1) * shift_ms; the
//         frame that ended the hold starts the next candidate
// emit(kind, f1, f2, time_ms) once per event, in order.
template <class Emit> inline void tone_events(const TonePlan &p, int shift_ms, uint64_t t0, const uint32_t *records, size_t n, ToneMachine &m, Emit emit)
{
    for (size_t i = 0; i < n; ++i) {
        const int32_t f1 = (int32_t)(records[i] & 0xffffu), f2 = (int32_t)(records[i] >> 16);
        const bool tonal = f1 != 0;
        const int64_t t = (int64_t)(t0 + i);
        if (m.held) {
            m.run = tonal && tone_match(f1, f2, m.h1, m.h2, p.tol_hz) ? 0 : m.run + 1;
            if (m.run < p.off_frames) continue;
            emit((int)TONE_OFF, (uint32_t)m.h1, (uint32_t)m.h2, (uint64_t)((t - p.off_frames + 1) * shift_ms));
            m = ToneMachine();
        }
        if (!tonal) { m.c1 = m.c2 = m.run = 0; continue; }
        if (m.run > 0 && tone_match(f1, f2, m.c1, m.c2, p.tol_hz)) m.run += 1;
        else { m.c1 = f1; m.c2 = f2; m.run = 1; }
        if (m.run >= p.on_frames) {
            emit((int)TONE_ON, (uint32_t)f1, (uint32_t)f2, (uint64_t)((t - p.on_frames + 1) * shift_ms));
            m = ToneMachine();
            m.held = 1; m.h1 = f1; m.h2 = f2;
        }
    }
}
// a completed flush at frame `frames_seen`: a held tone is closed there, and the machine starts afresh
template <class Emit> inline void tone_flush(int shift_ms, uint64_t frames_seen, ToneMachine &m, Emit emit)
{
    if (m.held) emit((int)TONE_OFF, (uint32_t)m.h1, (uint32_t)m.h2, frames_seen * (uint64_t)shift_ms);
    m = ToneMachine();
}

// the names of the table in include/aprilx_engine.h: the first entry all of whose frequencies lie within tol_hz, or null
struct ToneName { const char *name; uint32_t f1, f2; };
constexpr ToneName kToneNames[] = {{"dial", 350, 440}, {"busy", 480, 620}, {"cp425", 425, 0}, {"cng", 1100, 0}, {"ced", 2100, 0},
                                   {"sit1", 950, 0}, {"sit2", 1400, 0}, {"sit3", 1800, 0}};
inline const char *tone_name(uint32_t f1, uint32_t f2, uint32_t tol)
{
    for (const ToneName &e : kToneNames)
        if (tone_match((int32_t)(f1 & 0xffffu), (int32_t)(f2 & 0xffffu), (int32_t)e.f1, (int32_t)e.f2, (int32_t)(tol > 65535u ? 65535u : tol))) return e.name;
    return nullptr;
}

}  // namespace aprilx
