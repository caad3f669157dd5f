// Line quality per session (include/aprilx_engine.h "line quality"): level, clipping and dropout figures from the
// model-rate int16 samples the filterbank reads.  This is the host half of the contract, in plain C++ -- kernels_quality.hip is the
// device half and gives the same bits -- : the accepted options, the plan derived from them, the record of one frame, and the machine
// that turns consecutive records into reports and ON / OFF events.  Header-only on purpose: the scheduler harness (tests/sched_harness)
// builds session.cc without further files, and tests/cpp/quality_test.cc builds it alone under the sanitizers.
//
// Real frame t of a session owns the hop x[0 .. H), the first H = frame shift samples of the frame the filterbank reads for t: hops do
// not overlap, so sums over frames are sums over the audio.  The record of a frame is eight little-endian uint32, all integer arithmetic
// (the order of the reduction is free, every bit is pinned):
//   w0, w1  sumsq = sum of x * x, unsigned 64-bit, low word then high word
//   w2      sum of x, int32 two's complement
//   w3      (uint16)min(x) | (uint16)max(x) << 16
//   w4      clip_count | clip_run << 16: the samples with x >= L or x <= -L, and the longest run of consecutive such samples INSIDE the hop
//   w5      1 if min == max (a dead frame: digital silence or a stuck value), else 0
//   w6, w7  0
#pragma once
#include <cstddef>
#include <cstdint>

namespace aprilx {

constexpr int kQualityWords = 8;                           // uint32 per record
constexpr int kQualityMaxHop = 32767;                      // clip_count and clip_run are 16-bit halves; |sum| stays below 2^30

// the option values (the public AprilxQualityOptions without its size and flags)
struct QualityOptions {
    uint32_t clip_level = 32767, clip_run_min = 3, clip_hold_ms = 1000, dropout_ms = 200, report_ms = 1000;
};
// what kernel and machine need of them, 24 bytes (the layout of the public AprilxQualityPlan)
struct QualityPlan {
    int32_t hop = 0;                                       // H
    int32_t clip_level = 32767, clip_run_min = 3;
    int32_t hold_frames = 1, dropout_frames = 1;
    int32_t report_frames = 0;                             // 0: no reports
};
enum : int { QUALITY_REPORT = 1, QUALITY_CLIPPING_ON = 2, QUALITY_CLIPPING_OFF = 3, QUALITY_DROPOUT_ON = 4, QUALITY_DROPOUT_OFF = 5 };
// an event as the handler sees it, 80 bytes (the layout of the public AprilxQualityEvent); everything behind time_ms is a report's
struct QualityEvent {
    int32_t kind = 0;
    uint32_t frames = 0;
    uint64_t time_ms = 0;
    int64_t sum = 0;
    uint64_t sumsq = 0;
    int32_t min = 0, max = 0;
    uint64_t clip_samples = 0;
    uint32_t clipped_frames = 0, dead_frames = 0;
    uint64_t quiet_sumsq = 0, loud_sumsq = 0;              // smallest frame sumsq among the live frames (0: none), largest of all frames
    uint32_t hop = 0, reserved = 0;
};
// the machine between records, 88 bytes (the layout of the public AprilxQualityMachine): all zero at the start and after a flush
struct QualityMachine {
    int32_t clipping = 0, dropout = 0;                     // what is on
    int32_t quiet_run = 0;                                 // consecutive unclipped frames while clipping is on
    int32_t dead_run = 0;                                  // consecutive dead frames
    uint32_t frames = 0;                                   // the open interval, as a report's fields
    int32_t have_live = 0;
    uint64_t first_frame = 0;
    int64_t sum = 0;
    uint64_t sumsq = 0;
    int32_t min = 0, max = 0;
    uint64_t clip_samples = 0;
    uint32_t clipped_frames = 0, dead_frames = 0;
    uint64_t quiet_sumsq = 0, loud_sumsq = 0;
};
static_assert(sizeof(QualityPlan) == 24 && sizeof(QualityEvent) == 80 && sizeof(QualityMachine) == 88, "layouts shared with the device and the C ABI");

inline bool quality_options_valid(const QualityOptions &o)
{
    if (o.clip_level < 1024u || o.clip_level > 32767u) return false;
    if (o.clip_run_min < 1u || o.clip_run_min > 64u) return false;
    if (o.clip_hold_ms < 100u || o.clip_hold_ms > 60000u) return false;
    if (o.dropout_ms < 20u || o.dropout_ms > 60000u) return false;
    return o.report_ms == 0u || (o.report_ms >= 100u && o.report_ms <= 60000u);
}

// The plan, derived once: H = shift_ms * sample_rate / 1000, the durations in frames (ms / shift_ms, at least 1).  False: options out of
// range, or a model whose hop is empty, longer than its frame, or longer than kQualityMaxHop.
inline bool quality_make_plan(int sample_rate, int frame_samples, int shift_ms, const QualityOptions &o, QualityPlan *out)
{
    if (sample_rate <= 0 || shift_ms <= 0 || frame_samples <= 0 || !quality_options_valid(o)) return false;
    const int64_t hop = (int64_t)shift_ms * (int64_t)sample_rate / 1000;
    if (hop < 1 || hop > (int64_t)frame_samples || hop > (int64_t)kQualityMaxHop) return false;
    auto frames = [&](uint32_t ms) { const uint32_t f = ms / (uint32_t)shift_ms; return (int32_t)(f < 1u ? 1u : f); };
    QualityPlan p;
    p.hop = (int32_t)hop; p.clip_level = (int32_t)o.clip_level; p.clip_run_min = (int32_t)o.clip_run_min;
    p.hold_frames = frames(o.clip_hold_ms); p.dropout_frames = frames(o.dropout_ms);
    p.report_frames = o.report_ms ? frames(o.report_ms) : 0;
    *out = p;
    return true;
}

// the record of one hop x[0 .. H), clip level L
inline void quality_frame(const int16_t *x, int H, int L, uint32_t *w)
{
    uint64_t sumsq = 0;
    int32_t sum = 0, mn = 32767, mx = -32768;
    uint32_t count = 0, run = 0, best = 0;
    for (int i = 0; i < H; ++i) {
        const int32_t v = (int32_t)x[i];
        sumsq += (uint64_t)(uint32_t)(v * v);              // (at most 2^30)
        sum += v;
        if (v < mn) mn = v;
        if (v > mx) mx = v;
        if (v >= L || v <= -L) { ++count; ++run; if (run > best) best = run; }
        else run = 0;
    }
    w[0] = (uint32_t)(sumsq & 0xffffffffu); w[1] = (uint32_t)(sumsq >> 32);
    w[2] = (uint32_t)sum;
    w[3] = (uint32_t)(uint16_t)mn | (uint32_t)(uint16_t)mx << 16;
    w[4] = (count & 0xffffu) | best << 16;
    w[5] = mn == mx ? 1u : 0u;
    w[6] = 0u; w[7] = 0u;
}

// n hops, hop i at frames + i * ld, into records_out [n][8]
inline void quality_run_host(int H, int L, int n, const int16_t *frames, size_t ld, uint32_t *records_out)
{
    for (int i = 0; i < n; ++i) quality_frame(frames + (size_t)i * ld, H, L, records_out + (size_t)i * kQualityWords);
}

// the open interval as a report; emit(const QualityEvent &)
template <class Emit> inline void quality_close_interval(const QualityPlan &p, int shift_ms, QualityMachine &m, Emit emit)
{
    if (m.frames) {
        QualityEvent e;
        e.kind = QUALITY_REPORT; e.frames = m.frames; e.time_ms = m.first_frame * (uint64_t)shift_ms;
        e.sum = m.sum; e.sumsq = m.sumsq; e.min = m.min; e.max = m.max;
        e.clip_samples = m.clip_samples; e.clipped_frames = m.clipped_frames; e.dead_frames = m.dead_frames;
        e.quiet_sumsq = m.have_live ? m.quiet_sumsq : 0; e.loud_sumsq = m.loud_sumsq; e.hop = (uint32_t)p.hop;
        emit(e);
    }
    m.frames = 0; m.have_live = 0; m.first_frame = 0; m.sum = 0; m.sumsq = 0; m.min = 0; m.max = 0;
    m.clip_samples = 0; m.clipped_frames = 0; m.dead_frames = 0; m.quiet_sumsq = 0; m.loud_sumsq = 0;
}

// Events from consecutive records: record i is real frame t0 + i of the session.  Per frame, in this order:
//   CLIPPING   a frame is clipped when clip_run >= clip_run_min.  Off: a clipped frame gives CLIPPING_ON at t * shift_ms.  On: the
//              hold_frames-th consecutive unclipped frame gives CLIPPING_OFF at the time of the first of them.
//   DROPOUT    off: the dropout_frames-th consecutive dead frame gives DROPOUT_ON at the time of the first of them.  On: a live frame
//              gives DROPOUT_OFF at t * shift_ms.
//   REPORT     the frame joins the open interval (the first one starts at the machine's first frame); the report_frames-th frame closes
//              it with a REPORT at the time of its first frame.  report_frames == 0: no interval is kept.
template <class Emit> inline void quality_events(const QualityPlan &p, int shift_ms, uint64_t t0, const uint32_t *records, size_t n, QualityMachine &m, Emit emit)
{
    auto simple = [&](int kind, uint64_t frame) {
        QualityEvent e;
        e.kind = kind; e.time_ms = frame * (uint64_t)shift_ms; e.hop = (uint32_t)p.hop;
        emit(e);
    };
    for (size_t i = 0; i < n; ++i) {
        const uint32_t *w = records + i * kQualityWords;
        const uint64_t t = t0 + i;
        const uint64_t sumsq = (uint64_t)w[0] | (uint64_t)w[1] << 32;
        const int32_t mn = (int32_t)(int16_t)(uint16_t)(w[3] & 0xffffu), mx = (int32_t)(int16_t)(uint16_t)(w[3] >> 16);
        const uint32_t count = w[4] & 0xffffu, run = w[4] >> 16;
        const bool clipped = run >= (uint32_t)p.clip_run_min, dead = (w[5] & 1u) != 0;
        if (!m.clipping) {
            if (clipped) { m.clipping = 1; m.quiet_run = 0; simple(QUALITY_CLIPPING_ON, t); }
        } else if (clipped) {
            m.quiet_run = 0;
        } else if (++m.quiet_run >= p.hold_frames) {
            simple(QUALITY_CLIPPING_OFF, t + 1 - (uint64_t)m.quiet_run);
            m.clipping = 0; m.quiet_run = 0;
        }
        if (dead) {
            if (!m.dropout) {
                if (++m.dead_run >= p.dropout_frames) { m.dropout = 1; simple(QUALITY_DROPOUT_ON, t + 1 - (uint64_t)m.dead_run); m.dead_run = 0; }
            }
        } else {
            if (m.dropout) { m.dropout = 0; simple(QUALITY_DROPOUT_OFF, t); }
            m.dead_run = 0;
        }
        if (p.report_frames > 0) {
            if (!m.frames) { m.first_frame = t; m.min = mn; m.max = mx; m.loud_sumsq = sumsq; }
            m.frames += 1;
            m.sum += (int64_t)(int32_t)w[2]; m.sumsq += sumsq;
            if (mn < m.min) m.min = mn;
            if (mx > m.max) m.max = mx;
            m.clip_samples += count; m.clipped_frames += clipped ? 1u : 0u; m.dead_frames += dead ? 1u : 0u;
            if (sumsq > m.loud_sumsq) m.loud_sumsq = sumsq;
            if (!dead) { if (!m.have_live || sumsq < m.quiet_sumsq) m.quiet_sumsq = sumsq; m.have_live = 1; }
            if (m.frames >= (uint32_t)p.report_frames) quality_close_interval(p, shift_ms, m, emit);
        }
    }
}

// A flush completed behind frame t - 1: the OFF event of anything that is on, at t * shift_ms, then the open interval as a short report;
// the machine starts afresh.
template <class Emit> inline void quality_flush(const QualityPlan &p, int shift_ms, uint64_t t, QualityMachine &m, Emit emit)
{
    auto simple = [&](int kind) {
        QualityEvent e;
        e.kind = kind; e.time_ms = t * (uint64_t)shift_ms; e.hop = (uint32_t)p.hop;
        emit(e);
    };
    if (m.clipping) simple(QUALITY_CLIPPING_OFF);
    if (m.dropout) simple(QUALITY_DROPOUT_OFF);
    quality_close_interval(p, shift_ms, m, emit);
    m = QualityMachine();
}

}  // namespace aprilx
