// The layout of the ONE staging buffer of an Engine::fbank() call (pinned host buffer and its device twin, one host-to-device copy per
// call), stated once: the PCM windows (model-rate regions, then the input-rate spans of resampled sessions), then (16-byte aligned) the
// raw bytes of formatted sessions, then (16-byte aligned each, right behind the samples of THIS call) the frame descriptors, the
// resample descriptors, the decode descriptors and the VAD descriptors.  Pure arithmetic, no HIP: tests/cpp/staging_layout_test.cc
// holds it against the formulas it replaced.
#pragma once
#include <algorithm>
#include <cstddef>

namespace aprilx {

struct StagingCounts {
    size_t n_pcm = 0, n_in = 0;        // int16 samples: model-rate windows, input-rate spans
    size_t n_raw = 0;                  // raw bytes of formatted sessions
    size_t n_frames = 0, n_rs = 0, n_dc = 0, n_vd = 0;      // descriptors: frames, resample, decode, VAD
};
struct StagingSizes { size_t frame = 0, rs = 0, dc = 0, vd = 0; };      // bytes per descriptor

struct StagingLayout {
    size_t raw = 0, frames = 0, rs = 0, dc = 0, vd = 0;      // byte offsets of the raw region and of the four descriptor arrays
    size_t bytes = 0;                  // upload length: up to the end of the last array the call uses
    size_t pcm_units = 0;              // the three sample regions in int16 units, the raw region with its alignment
    size_t units = 0;                  // capacity (int16 units) of a buffer that holds exactly these counts
};

// capacity in int16 units of a buffer with room for `pcm_units` of samples and raw bytes and the given numbers of descriptors
inline size_t staging_units(size_t pcm_units, size_t frames, size_t rs, size_t dc, size_t vd, const StagingSizes &el)
{
    return pcm_units + 8 + (frames * el.frame + 1) / 2 + 8 + rs * el.rs / 2 + 8 + dc * el.dc / 2 + 8 + vd * el.vd / 2;
}

inline StagingLayout staging_layout(const StagingCounts &n, const StagingSizes &el)
{
    auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    StagingLayout l;
    l.raw = up16((n.n_pcm + n.n_in) * 2);                  // (empty without formatted sessions)
    l.frames = up16(l.raw + n.n_raw);
    l.rs = up16(l.frames + n.n_frames * el.frame);
    l.dc = up16(l.rs + n.n_rs * el.rs);
    l.vd = up16(l.dc + n.n_dc * el.dc);
    l.bytes = n.n_vd ? l.vd + n.n_vd * el.vd : n.n_dc ? l.dc + n.n_dc * el.dc : n.n_rs ? l.rs + n.n_rs * el.rs : l.frames + n.n_frames * el.frame;
    l.pcm_units = n.n_pcm + n.n_in + (n.n_dc ? (n.n_raw + 1) / 2 + 8 : 0);
    l.units = staging_units(l.pcm_units, n.n_frames, n.n_rs, n.n_dc, n.n_vd, el);
    return l;
}

// What the buffers have room for.  They only grow: to twice what the call needs, never below a floor (the descriptor arrays of a pass
// have none until a call carries that pass).
struct StagingCaps {
    size_t frames = 0, pcm_units = 0, rs = 0, dc = 0, vd = 0;
    bool holds(const StagingCounts &n, const StagingLayout &l) const
    {
        return n.n_frames <= frames && l.pcm_units <= pcm_units && n.n_rs <= rs && n.n_dc <= dc && n.n_vd <= vd;
    }
    void grow(const StagingCounts &n, const StagingLayout &l)
    {
        frames = std::max({n.n_frames * 2, frames, (size_t)1024});
        pcm_units = std::max({l.pcm_units * 2, pcm_units, (size_t)1 << 16});
        rs = std::max({n.n_rs * 2, rs, n.n_rs ? (size_t)256 : (size_t)0});
        dc = std::max({n.n_dc * 2, dc, n.n_dc ? (size_t)256 : (size_t)0});
        vd = std::max({n.n_vd * 2, vd, n.n_vd ? (size_t)256 : (size_t)0});
    }
    size_t units(const StagingSizes &el) const { return staging_units(pcm_units, frames, rs, dc, vd, el); }
};

}  // namespace aprilx
