// The layout of the ONE staging buffer of an Engine::fbank() call (pinned host buffer and its device twin, one host-to-device copy per
// call), stated once: the PCM windows (model-rate regions, then the input-rate spans of resampled sessions), then (16-byte aligned) the
// raw bytes of formatted sessions, then the descriptor arrays of THIS call, each 16-byte aligned right behind what precedes it, in one
// fixed order: frames, resample, decode, VAD, DTMF, tones, line quality.  Everything a pass sends to the device is in here; the upload ends with the last
// array the call uses.  Pure arithmetic, no HIP: tests/cpp/staging_layout_test.cc holds it against the formulas it replaced.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>

namespace aprilx {

// The descriptor arrays in buffer order: offsets, upload length and capacity all follow from walking this list.  The frames array is
// part of every call; the others are the passes', empty in a call without that pass.
enum StagingArray { ST_FRAMES = 0, ST_RS, ST_DC, ST_VD, ST_DT, ST_TN, ST_QA, ST_COUNT };      // frames, resample, decode, VAD, DTMF, tones, line quality
typedef std::array<size_t, ST_COUNT> StagingPer;      // one value per array
typedef StagingPer StagingSizes;                      // bytes per descriptor

struct StagingCounts {
    size_t n_pcm = 0, n_in = 0;        // int16 samples: model-rate windows, input-rate spans
    size_t n_raw = 0;                  // raw bytes of formatted sessions
    StagingPer n{};                    // descriptors per array
};

struct StagingLayout {
    size_t raw = 0;                    // byte offset of the raw region
    StagingPer off{};                  // ... and of the descriptor arrays
    size_t bytes = 0;                  // upload length: up to the end of the last array the call uses
    size_t pcm_units = 0;              // the three sample regions in int16 units, the raw region with its alignment
    size_t units = 0;                  // capacity (int16 units) of a buffer that holds exactly these counts
};

// capacity in int16 units of a buffer with room for `pcm_units` of samples and raw bytes and `n` elements per array: per array 8 units for
// its alignment, then its bytes.  The first four keep those 8 units when they are empty (buffers without DTMF, tones and line quality stay the size they always
// had); an array behind them gets room only once it has elements.
inline size_t staging_units(size_t pcm_units, const StagingPer &n, const StagingSizes &el)
{
    size_t units = pcm_units;
    for (size_t i = 0; i < ST_COUNT; ++i)
        if (i < 4 || n[i]) units += 8 + (n[i] * el[i] + 1) / 2;
    return units;
}

inline StagingLayout staging_layout(const StagingCounts &n, const StagingSizes &el)
{
    auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    StagingLayout l;
    l.raw = up16((n.n_pcm + n.n_in) * 2);                  // (empty without formatted sessions)
    size_t end = l.raw + n.n_raw;
    for (size_t i = 0; i < ST_COUNT; ++i) {
        l.off[i] = up16(end);
        end = l.off[i] + n.n[i] * el[i];
        if (i == ST_FRAMES || n.n[i]) l.bytes = end;
    }
    l.pcm_units = n.n_pcm + n.n_in + (n.n[ST_DC] ? (n.n_raw + 1) / 2 + 8 : 0);
    l.units = staging_units(l.pcm_units, n.n, el);
    return l;
}

// What the buffers have room for.  They only grow: to twice what the call needs, never below a floor (the descriptor arrays of a pass
// have none until a call carries that pass).
struct StagingCaps {
    size_t pcm_units = 0;
    StagingPer n{};                    // elements per array
    bool holds(const StagingCounts &c, const StagingLayout &l) const
    {
        bool ok = l.pcm_units <= pcm_units;
        for (size_t i = 0; i < ST_COUNT; ++i) ok = ok && c.n[i] <= n[i];
        return ok;
    }
    void grow(const StagingCounts &c, const StagingLayout &l)
    {
        pcm_units = std::max({l.pcm_units * 2, pcm_units, (size_t)1 << 16});
        for (size_t i = 0; i < ST_COUNT; ++i) n[i] = std::max({c.n[i] * 2, n[i], i == ST_FRAMES ? (size_t)1024 : c.n[i] ? (size_t)256 : (size_t)0});
    }
    size_t units(const StagingSizes &el) const { return staging_units(pcm_units, n, el); }
};

}  // namespace aprilx
