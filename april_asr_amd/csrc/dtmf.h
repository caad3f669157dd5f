// DTMF digits per session (include/aprilx_engine.h "DTMF"): key-down / key-up events from the model-rate samples
// the filterbank reads.  This is the contract in plain C++ -- kernels_dtmf.hip is the device half and gives the same bits -- : the
// accepted options, the plan derived from them, the tables, steps 1-5 over an array of frames, and the events that follow from the
// bytes.  Header-only on purpose: the scheduler harness (tests/sched_harness) builds session.cc without further files, and
// tests/cpp/dtmf_test.cc builds it alone under the sanitizers.
//
// All arithmetic is fp32, never contracted (-ffp-contract=off), in exactly the order written.  The frame is the filterbank's own; the
// detector reads its first Wd samples x[0 .. Wd) (int16), Wd = min(fft_size, 64 * (rate / 4000)): 16 ms in whole 64-sample steps.
// Tables T[16][Wd]: rows 0..7 cos(2 pi f_k j / rate), rows 8..15 sin(...), f = 697 770 852 941 | 1209 1336 1477 1633, computed in
// double and rounded once.  Per real frame:
//   1  per table row 64 chains a[l] = 0.0f + float(x[l]) * T[l] + float(x[l + 64]) * T[l + 64] + ... (indices below Wd, multiply then
//      add, increasing index), then a[l] = a[l] + a[l ^ m] for m = 32, 16, 8, 4, 2, 1 (IEEE addition commutes: every lane holds the same
//      bits);  re = a[0] of row k, im = a[0] of row 8 + k;  P[k] = re * re + im * im
//   2  E = float(sum x[j]^2), the sum exact in 64-bit integers
//   3  r = first maximum of P[0..4), c = first maximum of P[4..8), pr = P[r], pc = P[4 + c]
//   4  code = 1 + 4 r + c when all of
//        pr >= min_power, pc >= min_power;  !(pc > pr * twist_hi), !(pr > pc * twist_lo);
//        !(P[i] * rel_peak > pr) for every other row i, !(P[4 + i] * rel_peak > pc) for every other column i;
//        !((pr + pc) < min_share * (E * half_w))
//      hold, else 0  (written so that NaN and exact ties fall the same way everywhere)
//   5  one byte per frame: the code.  No state on the device.
// The digits are "123A456B789C*0#D"[code - 1].
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define APRILX_DTMF_HD __host__ __device__
#else
#define APRILX_DTMF_HD
#endif

namespace aprilx {

constexpr int kDtmfLanes = 64, kDtmfRows = 16, kDtmfMaxW = 4096;
constexpr int kDtmfHz[8] = {697, 770, 852, 941, 1209, 1336, 1477, 1633};
constexpr char kDtmfDigits[17] = "123A456B789C*0#D";

// the option values (the public AprilxDtmfOptions without its size and flags)
struct DtmfOptions {
    float min_level_dbfs = -40.0f, twist_hi_db = 4.0f, twist_lo_db = 8.0f, rel_peak_db = 8.0f, min_share = 0.6f;
    uint32_t min_tone_ms = 20, min_pause_ms = 20;
};
// what the kernel and the event machine need of them, 40 bytes (the layout of the public AprilxDtmfPlan)
struct DtmfPlan {
    int32_t Wd = 0;
    float half_w = 0, min_power = 0, twist_hi = 0, twist_lo = 0, rel_peak = 0, min_share = 0;
    int32_t on_frames = 1, off_frames = 1, reserved = 0;
};
static_assert(sizeof(DtmfPlan) == 40, "layout shared with the device and the C ABI");
// the host's event machine, integers only: the held code (0: idle), the candidate code and the length of the current run
struct DtmfMachine { int32_t held = 0, cand = 0, run = 0; };

enum : int { DTMF_DOWN = 1, DTMF_UP = 2 };

inline bool dtmf_options_valid(const DtmfOptions &o)
{
    auto in = [](float v, float lo, float hi) { return std::isfinite(v) && v >= lo && v <= hi; };
    if (!in(o.min_level_dbfs, -70.0f, 0.0f) || !in(o.twist_hi_db, 0.0f, 20.0f) || !in(o.twist_lo_db, 0.0f, 20.0f) || !in(o.rel_peak_db, 3.0f, 30.0f)) return false;
    if (!(std::isfinite(o.min_share) && o.min_share > 0.0f && o.min_share <= 1.0f)) return false;
    return o.min_tone_ms >= 10u && o.min_tone_ms <= 1000u && o.min_pause_ms >= 10u && o.min_pause_ms <= 1000u;
}

// Wd of a model, or 0 when the model is refused: a window shorter than 12 ms, a rate below 4000 Hz, or a window beyond kDtmfMaxW
inline int dtmf_window(int rate, int fft_size)
{
    if (rate < 4000 || fft_size <= 0) return 0;
    const int64_t w16 = (int64_t)64 * (rate / 4000);          // 64 * floor(0.016 * rate / 64)
    const int64_t wd = w16 < fft_size ? w16 : fft_size;
    if (wd * 1000 < (int64_t)12 * rate || wd > kDtmfMaxW) return 0;
    return (int)wd;
}

// The plan, derived once in double and rounded once.  False: options out of range, or a refused model.
inline bool dtmf_make_plan(int rate, int fft_size, int shift_ms, const DtmfOptions &o, DtmfPlan *out)
{
    const int wd = dtmf_window(rate, fft_size);
    if (!wd || shift_ms <= 0 || !dtmf_options_valid(o)) return false;
    DtmfPlan p;
    p.Wd = wd;
    p.half_w = 0.5f * (float)wd;
    const double amp = 32768.0 * std::pow(10.0, (double)o.min_level_dbfs / 20.0) * (double)wd / 2.0;
    p.min_power = (float)(amp * amp);
    p.twist_hi = (float)std::pow(10.0, (double)o.twist_hi_db / 10.0);
    p.twist_lo = (float)std::pow(10.0, (double)o.twist_lo_db / 10.0);
    p.rel_peak = (float)std::pow(10.0, (double)o.rel_peak_db / 10.0);
    p.min_share = o.min_share;
    p.on_frames = (int32_t)(o.min_tone_ms / (uint32_t)shift_ms); if (p.on_frames < 1) p.on_frames = 1;
    p.off_frames = (int32_t)(o.min_pause_ms / (uint32_t)shift_ms); if (p.off_frames < 1) p.off_frames = 1;
    *out = p;
    return true;
}

// the tables [16][Wd]
inline void dtmf_make_tables(int rate, int wd, float *out)
{
    for (int k = 0; k < 8; ++k)
        for (int j = 0; j < wd; ++j) {
            const double w = 2.0 * 3.14159265358979323846 * (double)kDtmfHz[k] * (double)j / (double)rate;
            out[(size_t)k * (size_t)wd + (size_t)j] = (float)std::cos(w);
            out[(size_t)(8 + k) * (size_t)wd + (size_t)j] = (float)std::sin(w);
        }
}

// steps 3 and 4 on the eight powers and the energy; returns the code
APRILX_DTMF_HD inline int dtmf_decide(const DtmfPlan &p, const float *P, float E)
{
    int r = 0, c = 0;
    for (int i = 1; i < 4; ++i) { if (P[i] > P[r]) r = i; if (P[4 + i] > P[4 + c]) c = i; }
    const float pr = P[r], pc = P[4 + c];
    bool ok = pr >= p.min_power && pc >= p.min_power;
    ok = ok && !(pc > pr * p.twist_hi) && !(pr > pc * p.twist_lo);
    for (int i = 0; i < 4; ++i) {
        if (i != r) ok = ok && !(P[i] * p.rel_peak > pr);
        if (i != c) ok = ok && !(P[4 + i] * p.rel_peak > pc);
    }
    ok = ok && !((pr + pc) < p.min_share * (E * p.half_w));
    return ok ? 1 + 4 * r + c : 0;
}

// steps 1 and 2 of one frame: P[0..8) and E into out9
inline void dtmf_powers(const DtmfPlan &p, const float *tables, const int16_t *x, float *out9)
{
    float a[kDtmfRows], c[kDtmfLanes], t[kDtmfLanes];
    for (int row = 0; row < kDtmfRows; ++row) {
        const float *T = tables + (size_t)row * (size_t)p.Wd;
        for (int l = 0; l < kDtmfLanes; ++l) {
            c[l] = 0.0f;
            for (int j = l; j < p.Wd; j += kDtmfLanes) { const float m = (float)x[j] * T[j]; c[l] = c[l] + m; }
        }
        for (int m = kDtmfLanes / 2; m >= 1; m >>= 1) {
            for (int l = 0; l < kDtmfLanes; ++l) t[l] = c[l] + c[l ^ m];
            for (int l = 0; l < kDtmfLanes; ++l) c[l] = t[l];
        }
        a[row] = c[0];
    }
    for (int k = 0; k < 8; ++k) { const float rr = a[k] * a[k], ii = a[8 + k] * a[8 + k]; out9[k] = rr + ii; }
    int64_t e = 0;
    for (int j = 0; j < p.Wd; ++j) e += (int64_t)x[j] * (int64_t)x[j];
    out9[8] = (float)e;
}

// n frames (frame i at frames + i * ld, Wd samples read of each) through steps 1-5; powers_out (may be null) receives [n][9]
inline void dtmf_run_host(const DtmfPlan &p, const float *tables, int n, const int16_t *frames, size_t ld, uint8_t *codes_out, float *powers_out)
{
    for (int i = 0; i < n; ++i) {
        float q[9];
        dtmf_powers(p, tables, frames + (size_t)i * ld, q);
        if (powers_out) for (int k = 0; k < 9; ++k) powers_out[(size_t)i * 9 + (size_t)k] = q[k];
        codes_out[i] = (uint8_t)dtmf_decide(p, q, q[8]);
    }
}

// Events from the codes of consecutive real frames: byte i is frame t0 + i of the session.
//   idle: the same non-zero code in on_frames consecutive frames -> DOWN(digit) at (t - on_frames + 1) * shift_ms
//   held: off_frames consecutive frames whose code differs from the held one -> UP(digit) at (t - off_frames + 1) * shift_ms; the
//         frame that ended the hold starts the next candidate run
// emit(kind, digit, time_ms) once per event, in order.
template <class Emit> inline void dtmf_events(const DtmfPlan &p, int shift_ms, uint64_t t0, const uint8_t *codes, size_t n, DtmfMachine &m, Emit emit)
{
    for (size_t i = 0; i < n; ++i) {
        const int32_t c = codes[i] <= 16 ? (int32_t)codes[i] : 0;
        const int64_t t = (int64_t)(t0 + i);
        if (m.held) {
            m.run = c != m.held ? m.run + 1 : 0;
            if (m.run < p.off_frames) continue;
            emit((int)DTMF_UP, kDtmfDigits[m.held - 1], (uint64_t)((t - p.off_frames + 1) * shift_ms));
            m = DtmfMachine();
        }
        if (c != m.cand) { m.cand = c; m.run = c ? 1 : 0; }
        else if (c) m.run += 1;
        if (c && m.run >= p.on_frames) {
            emit((int)DTMF_DOWN, kDtmfDigits[c - 1], (uint64_t)((t - p.on_frames + 1) * shift_ms));
            m.held = c; m.cand = 0; m.run = 0;
        }
    }
}
// a completed flush at frame `frames_seen`: a held digit is closed there, and the machine starts afresh
template <class Emit> inline void dtmf_flush(int shift_ms, uint64_t frames_seen, DtmfMachine &m, Emit emit)
{
    if (m.held) emit((int)DTMF_UP, kDtmfDigits[m.held - 1], frames_seen * (uint64_t)shift_ms);
    m = DtmfMachine();
}

}  // namespace aprilx
