// Voice activity per session (include/aprilx_engine.h "voice activity"): speech start / end events from the
// log-mel rows the filterbank has just written.  This is the host half of the contract, in plain C++ -- kernels_vad.hip is the device
// half and gives the same bits -- : the accepted options, the plan derived from them, steps 1-9 over an array of rows, and the events
// that follow from the bytes.  Header-only on purpose: the scheduler harness (tests/sched_harness) builds session.cc without further
// files, and tests/cpp/vad_test.cc builds it alone under the sanitizers.
//
// All arithmetic is fp32, never contracted (-ffp-contract=off), in exactly the order written.  min and max are the comparisons
//   vmin(a, b) = b < a ? b : a        vmax(a, b) = a < b ? b : a
// so that the sign of a zero is pinned too.  Per real frame x[0 .. nbins), in frame order:
//   1  sixteen chains p[l] = 0.0f + x[b0 + l] + x[b0 + l + 16] + ... (indices below b1), then p[l] = p[l] + p[l ^ m] for m = 8, 4, 2, 1
//      (IEEE addition commutes: every lane holds the same bits);  e = p[0] * inv_nb
//   2  e = vmax(e, min_energy)
//   3  first frame after a reset: s = e;  else t = e - s; t = 0.25f * t; s = s + t
//   4  cur = vmin(cur, s); cnt += 1
//   5  n = cur; n = vmin(n, hist[i]) for i = 0 .. 7;  d = s - n
//   6  raw = d > (st ? thr_off : thr_on)              (the st from before this frame)
//   7  cnt == 32: hist[pos] = cur; pos = (pos + 1) & 7; cur = +inf; cnt = 0
//   8  silence: run = raw ? run + 1 : 0; run >= onset_frames: st = 1, run = 0
//      speech:  run = raw ? 0 : run + 1; run >= hangover_frames: st = 0, run = 0
//   9  byte = st | raw << 1
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace aprilx {

constexpr float kVadAlpha = 0.25f;
constexpr int kVadSubFrames = 32, kVadSubWindows = 8, kVadLanes = 16;
constexpr float kVadDbToLn = 0.23025851f;                  // ln(10) / 10 as the nearest fp32: dB of power -> natural log units

// the option values (the public AprilxVadOptions without its size and flags)
struct VadOptions {
    float band_lo_hz = 200.0f, band_hi_hz = 4000.0f, onset_db = 5.0f, offset_db = 3.0f;
    uint32_t onset_ms = 50, hangover_ms = 300;
    float min_energy = -12.0f;
};
// what the kernel needs of them, 32 bytes (the layout of the public AprilxVadPlan)
struct VadPlan {
    int32_t b0 = 0, b1 = 0;                                // the band: mel bins [b0, b1)
    float inv_nb = 0, thr_on = 0, thr_off = 0, min_energy = 0;
    int32_t onset_frames = 1, hangover_frames = 1;
};
// a session's detector state, 64 bytes (the layout of the public AprilxVadState)
struct VadState {
    float s = 0, cur = INFINITY, hist[kVadSubWindows] = {INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY};
    int32_t cnt = 0, pos = 0, st = 0, run = 0, first = 1, reserved = 0;
};
static_assert(sizeof(VadPlan) == 32 && sizeof(VadState) == 64, "layouts shared with the device and the C ABI");

enum : int { VAD_SPEECH_START = 1, VAD_SPEECH_END = 2 };

inline float vmin(float a, float b) { return b < a ? b : a; }
inline float vmax(float a, float b) { return a < b ? b : a; }

inline bool vad_options_valid(const VadOptions &o, int sample_rate)
{
    if (!(std::isfinite(o.band_lo_hz) && std::isfinite(o.band_hi_hz) && o.band_lo_hz >= 0.0f && o.band_lo_hz < o.band_hi_hz
          && (double)o.band_hi_hz <= 0.5 * (double)sample_rate)) return false;
    if (!(std::isfinite(o.onset_db) && std::isfinite(o.offset_db) && o.offset_db > 0.0f && o.offset_db <= o.onset_db && o.onset_db <= 60.0f)) return false;
    if (o.onset_ms < 10u || o.onset_ms > 1000u || o.hangover_ms < 10u || o.hangover_ms > 10000u) return false;
    return std::isfinite(o.min_energy);
}

// The plan, derived once: the band is the mel bins whose peak -- argmax_k mel[b][k], first maximum, times rate / padded with
// padded = 2 nfft_bins, in double -- lies in [lo, hi].  False: options out of range, or a band without a bin.
inline bool vad_make_plan(const float *mel, int nbins, int nfft_bins, int sample_rate, int shift_ms, const VadOptions &o, VadPlan *out)
{
    if (!mel || nbins <= 0 || nfft_bins <= 0 || sample_rate <= 0 || shift_ms <= 0 || !vad_options_valid(o, sample_rate)) return false;
    int b0 = -1, b1 = -1;
    for (int b = 0; b < nbins; ++b) {
        int k = 0;
        for (int i = 1; i < nfft_bins; ++i) if (mel[(size_t)b * nfft_bins + i] > mel[(size_t)b * nfft_bins + k]) k = i;
        const double hz = (double)k * (double)sample_rate / (2.0 * (double)nfft_bins);
        if (hz < (double)o.band_lo_hz || hz > (double)o.band_hi_hz) { if (b0 >= 0) break; continue; }
        if (b0 < 0) b0 = b;
        b1 = b + 1;
    }
    if (b0 < 0) return false;
    VadPlan p;
    p.b0 = b0; p.b1 = b1;
    p.inv_nb = 1.0f / (float)(b1 - b0);
    p.thr_on = o.onset_db * kVadDbToLn; p.thr_off = o.offset_db * kVadDbToLn;
    p.min_energy = o.min_energy;
    p.onset_frames = (int32_t)(o.onset_ms / (uint32_t)shift_ms); if (p.onset_frames < 1) p.onset_frames = 1;
    p.hangover_frames = (int32_t)(o.hangover_ms / (uint32_t)shift_ms); if (p.hangover_frames < 1) p.hangover_frames = 1;
    *out = p;
    return true;
}

// step 1
inline float vad_band_energy(const VadPlan &p, const float *x)
{
    float c[kVadLanes], t[kVadLanes];
    for (int l = 0; l < kVadLanes; ++l) {
        c[l] = 0.0f;
        for (int i = p.b0 + l; i < p.b1; i += kVadLanes) c[l] = c[l] + x[i];
    }
    for (int m = kVadLanes / 2; m >= 1; m >>= 1) {
        for (int l = 0; l < kVadLanes; ++l) t[l] = c[l] + c[l ^ m];
        for (int l = 0; l < kVadLanes; ++l) c[l] = t[l];
    }
    return c[0] * p.inv_nb;
}

// steps 2-9 on the energy of step 1; returns the byte
inline uint8_t vad_step(const VadPlan &p, VadState &v, float e)
{
    e = vmax(e, p.min_energy);
    if (v.first) { v.s = e; v.first = 0; }
    else { float t = e - v.s; t = kVadAlpha * t; v.s = v.s + t; }
    v.cur = vmin(v.cur, v.s); v.cnt += 1;
    float n = v.cur;
    for (int i = 0; i < kVadSubWindows; ++i) n = vmin(n, v.hist[i]);
    const float d = v.s - n;
    const int raw = d > (v.st ? p.thr_off : p.thr_on) ? 1 : 0;
    if (v.cnt == kVadSubFrames) { v.hist[v.pos] = v.cur; v.pos = (v.pos + 1) & (kVadSubWindows - 1); v.cur = INFINITY; v.cnt = 0; }
    if (!v.st) { v.run = raw ? v.run + 1 : 0; if (v.run >= p.onset_frames) { v.st = 1; v.run = 0; } }
    else { v.run = raw ? 0 : v.run + 1; if (v.run >= p.hangover_frames) { v.st = 0; v.run = 0; } }
    return (uint8_t)(v.st | raw << 1);
}

// n rows of `ld` floats through steps 1-9; energy_out (may be null) receives step 1's e of every row
inline void vad_run_host(const VadPlan &p, int n, const float *rows, size_t ld, VadState &v, uint8_t *bytes_out, float *energy_out)
{
    for (int i = 0; i < n; ++i) {
        const float e = vad_band_energy(p, rows + (size_t)i * ld);
        if (energy_out) energy_out[i] = e;
        bytes_out[i] = vad_step(p, v, e);
    }
}

// Events from bit 0 of consecutive bytes: byte i is real frame t0 + i of the session, `last` the bit of frame t0 - 1 (0 after a reset).
// 0 -> 1 at frame t: SPEECH_START at (t - onset_frames + 1) * shift_ms; 1 -> 0: SPEECH_END at (t - hangover_frames + 1) * shift_ms.
// Returns the last bit; emit(kind, time_ms) once per event, in order.
template <class Emit> inline int vad_events(const VadPlan &p, int shift_ms, uint64_t t0, const uint8_t *bytes, size_t n, int last, Emit emit)
{
    for (size_t i = 0; i < n; ++i) {
        const int st = bytes[i] & 1;
        const int64_t t = (int64_t)(t0 + i);
        if (st && !last) emit((int)VAD_SPEECH_START, (uint64_t)((t - p.onset_frames + 1) * shift_ms));
        else if (!st && last) emit((int)VAD_SPEECH_END, (uint64_t)((t - p.hangover_frames + 1) * shift_ms));
        last = st;
    }
    return last;
}

}  // namespace aprilx
