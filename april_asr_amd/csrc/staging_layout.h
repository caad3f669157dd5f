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

struct StagingCounts {
    size_t n_pcm = 0, n_in = 0;        // int16 samples: model-rate windows, input-rate spans
    size_t n_raw = 0;                  // raw bytes of formatted sessions
    size_t n_frames = 0, n_rs = 0, n_dc = 0, n_vd = 0, n_dt = 0, n_tn = 0, n_qa = 0;      // descriptors: frames, resample, decode, VAD, DTMF, tones, line quality
};
struct StagingSizes { size_t frame = 0, rs = 0, dc = 0, vd = 0, dt = 0, tn = 0, qa = 0; };      // bytes per descriptor

struct StagingLayout {
    size_t raw = 0, frames = 0, rs = 0, dc = 0, vd = 0, dt = 0, tn = 0, qa = 0;      // byte offsets of the raw region and of the seven descriptor arrays
    size_t bytes = 0;                  // upload length: up to the end of the last array the call uses
    size_t pcm_units = 0;              // the three sample regions in int16 units, the raw region with its alignment
    size_t units = 0;                  // capacity (int16 units) of a buffer that holds exactly these counts
};

// The descriptor arrays in buffer order, each as {elements, bytes per element}: offsets, upload length and capacity all follow from
// walking this list.  The frames array is part of every call; the others are the passes', empty in a call without that pass.
struct StagingArray { size_t n, el; };
typedef std::array<StagingArray, 7> StagingArrays;
inline StagingArrays staging_arrays(size_t frames, size_t rs, size_t dc, size_t vd, size_t dt, size_t tn, size_t qa, const StagingSizes &el)
{
    return {{{frames, el.frame}, {rs, el.rs}, {dc, el.dc}, {vd, el.vd}, {dt, el.dt}, {tn, el.tn}, {qa, el.qa}}};
}

// capacity in int16 units of a buffer with room for `pcm_units` of samples and raw bytes and the given arrays: per array 8 units for
// its alignment, then its bytes.  The first four keep those 8 units when they are empty (buffers without DTMF, tones and line quality stay the size they always
// had); an array behind them gets room only once it has elements.
inline size_t staging_units(size_t pcm_units, const StagingArrays &arrays)
{
    size_t units = pcm_units;
    for (size_t i = 0; i < arrays.size(); ++i)
        if (i < 4 || arrays[i].n) units += 8 + (arrays[i].n * arrays[i].el + 1) / 2;
    return units;
}

inline StagingLayout staging_layout(const StagingCounts &n, const StagingSizes &el)
{
    auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    StagingLayout l;
    l.raw = up16((n.n_pcm + n.n_in) * 2);                  // (empty without formatted sessions)
    const StagingArrays arrays = staging_arrays(n.n_frames, n.n_rs, n.n_dc, n.n_vd, n.n_dt, n.n_tn, n.n_qa, el);
    size_t *const offset[] = {&l.frames, &l.rs, &l.dc, &l.vd, &l.dt, &l.tn, &l.qa};
    size_t end = l.raw + n.n_raw;
    for (size_t i = 0; i < arrays.size(); ++i) {
        *offset[i] = up16(end);
        end = *offset[i] + arrays[i].n * arrays[i].el;
        if (i == 0 || arrays[i].n) l.bytes = end;
    }
    l.pcm_units = n.n_pcm + n.n_in + (n.n_dc ? (n.n_raw + 1) / 2 + 8 : 0);
    l.units = staging_units(l.pcm_units, arrays);
    return l;
}

// What the buffers have room for.  They only grow: to twice what the call needs, never below a floor (the descriptor arrays of a pass
// have none until a call carries that pass).
struct StagingCaps {
    size_t frames = 0, pcm_units = 0, rs = 0, dc = 0, vd = 0, dt = 0, tn = 0, qa = 0;
    bool holds(const StagingCounts &n, const StagingLayout &l) const
    {
        return n.n_frames <= frames && l.pcm_units <= pcm_units && n.n_rs <= rs && n.n_dc <= dc && n.n_vd <= vd && n.n_dt <= dt && n.n_tn <= tn && n.n_qa <= qa;
    }
    void grow(const StagingCounts &n, const StagingLayout &l)
    {
        auto pass = [](size_t need, size_t &cap) { cap = std::max({need * 2, cap, need ? (size_t)256 : (size_t)0}); };
        frames = std::max({n.n_frames * 2, frames, (size_t)1024});
        pcm_units = std::max({l.pcm_units * 2, pcm_units, (size_t)1 << 16});
        pass(n.n_rs, rs); pass(n.n_dc, dc); pass(n.n_vd, vd); pass(n.n_dt, dt); pass(n.n_tn, tn); pass(n.n_qa, qa);
    }
    size_t units(const StagingSizes &el) const { return staging_units(pcm_units, staging_arrays(frames, rs, dc, vd, dt, tn, qa, el)); }
};

}  // namespace aprilx
