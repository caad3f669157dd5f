// Input formats (include/aprilx_engine.h "input format"): sessions that are fed G.711, float32 or interleaved
// multi-channel audio.  A format decodes to ONE int16 sample per audio frame, and everything behind the decode sees exactly those
// samples.  This is the host half of the contract, in plain C++ -- kernels_decode.hip is the device half -- and the raw-byte queue
// of such a session.  Header-only on purpose: the scheduler harness (tests/sched_harness) builds session.cc without further files,
// and tests/cpp/input_format_test.cc builds it alone under the sanitizers.
//
//   S16    little-endian int16, identity
//   MULAW  u = ~b & 0xFF; mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84; value = u & 0x80 ? -mag : mag
//   ALAW   a = b ^ 0x55; e = (a >> 4) & 7; m = a & 15; mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
//          value = a & 0x80 ? mag : -mag
//   F32    little-endian binary32: y = x * 32768 in fp32, NaN -> 0, clamped to [-32768, 32767], rounded half to even
//   channel >= 0 selects that channel of the frame; channel -1 is the downmix of the frame's C decoded integer values with sum S:
//          floor((2 S + C) / (2 C)), rounding half towards +infinity
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace aprilx {

enum : uint32_t { ENC_S16 = 0, ENC_MULAW = 1, ENC_ALAW = 2, ENC_F32 = 3, ENC_COUNT = 4 };
constexpr uint32_t kMaxInputChannels = 8;

// frame_bytes == 0: no format (the session takes mono PCM16 through the path it always took)
struct InputFormat {
    uint32_t encoding = ENC_S16, channels = 1;
    int32_t channel = 0;
    uint32_t frame_bytes = 0;
    explicit operator bool() const { return frame_bytes != 0; }
};

inline uint32_t encoding_bytes(uint32_t enc) { return enc == ENC_S16 ? 2u : (enc == ENC_F32 ? 4u : 1u); }
inline bool input_format_valid(uint32_t enc, uint32_t channels, int32_t channel)
{
    return enc < ENC_COUNT && channels >= 1 && channels <= kMaxInputChannels && channel >= -1 && channel < (int32_t)channels;
}
inline bool input_format_default(uint32_t enc, uint32_t channels, int32_t channel) { return enc == ENC_S16 && channels == 1 && channel == 0; }

inline int32_t decode_mulaw(uint32_t b)
{
    const uint32_t u = ~b & 0xFFu;
    const int32_t mag = (int32_t)(((((u & 15u) << 3) + 0x84u) << ((u >> 4) & 7u)) - 0x84u);
    return (u & 0x80u) ? -mag : mag;
}
inline int32_t decode_alaw(uint32_t b)
{
    const uint32_t a = (b ^ 0x55u) & 0xFFu, e = (a >> 4) & 7u, m = a & 15u;
    const int32_t mag = (int32_t)(e == 0 ? (m << 4) + 8u : ((m << 4) + 0x108u) << (e - 1u));
    return (a & 0x80u) ? mag : -mag;
}
inline int32_t decode_f32(float x)
{
    float y = x * 32768.0f;
    if (y != y) return 0;
    y = y < -32768.0f ? -32768.0f : (y > 32767.0f ? 32767.0f : y);
    return (int32_t)std::nearbyintf(y);                 // round half to even (the default rounding mode)
}
// one channel's value of a frame that starts at `p` (any alignment)
inline int32_t decode_value(uint32_t enc, const uint8_t *p, uint32_t ch)
{
    switch (enc) {
    case ENC_MULAW: return decode_mulaw(p[ch]);
    case ENC_ALAW: return decode_alaw(p[ch]);
    case ENC_F32: { float x; memcpy(&x, p + 4 * (size_t)ch, 4); return decode_f32(x); }
    default: return (int16_t)((uint32_t)p[2 * (size_t)ch] | ((uint32_t)p[2 * (size_t)ch + 1] << 8));
    }
}
inline int32_t downmix(int32_t sum, int32_t channels)
{
    const int32_t n = 2 * sum + channels, d = 2 * channels;
    return n >= 0 ? n / d : -((-n + d - 1) / d);        // floor
}
inline int16_t decode_frame(const InputFormat &f, const uint8_t *p)
{
    if (f.channel >= 0) return (int16_t)decode_value(f.encoding, p, (uint32_t)f.channel);
    int32_t s = 0;
    for (uint32_t c = 0; c < f.channels; ++c) s += decode_value(f.encoding, p, c);
    return (int16_t)downmix(s, (int32_t)f.channels);
}

// The queued and unconsumed audio of a session with a format: raw bytes, one frame of `fbytes` bytes per stream position.  The
// same two parts as the int16 queue of FrameBook: `bytes` (owned), then `ext` (a buffer a blocked caller lends for one tick).
struct RawFifo {
    size_t fbytes = 1;
    std::vector<uint8_t> bytes;
    const uint8_t *ext = nullptr; size_t ext_cnt = 0;      // (frames)
    typedef std::vector<std::pair<const uint8_t *, size_t>> Parts;      // (pointer, bytes)
    size_t own() const { return bytes.size() / fbytes; }
    size_t count() const { return own() + ext_cnt; }
    void append(const uint8_t *p, size_t frames) { bytes.insert(bytes.end(), p, p + frames * fbytes); }
    void absorb()                                          // ext -> bytes (positions stay valid)
    {
        if (!ext) return;
        append(ext, ext_cnt);
        ext = nullptr; ext_cnt = 0;
    }
    void drop(size_t frames) { bytes.erase(bytes.begin(), bytes.begin() + (long)(frames * fbytes)); }     // (frames <= own())
    // end of a tick: frames before `keep` (an index into bytes ++ ext) are consumed.  True: everything owned was consumed, the queue
    // is now the lent buffer's tail and starts at `keep`; false: the lent buffer was appended, nothing was dropped
    bool settle(size_t keep)
    {
        if (!ext) return false;
        if (keep < own()) { absorb(); return false; }
        const size_t skip = keep - own();
        bytes.assign(ext + skip * fbytes, ext + ext_cnt * fbytes);
        ext = nullptr; ext_cnt = 0;
        return true;
    }
    void clear() { bytes.clear(); ext = nullptr; ext_cnt = 0; }
    void span(size_t l0, size_t l1, Parts &parts) const    // frames [l0, l1) of bytes ++ ext (l0 < l1) as at most two parts
    {
        const size_t n = own();
        if (l0 < n) parts.emplace_back(bytes.data() + l0 * fbytes, ((l1 < n ? l1 : n) - l0) * fbytes);
        if (l1 > n) { const size_t a = l0 > n ? l0 : n; parts.emplace_back(ext + (a - n) * fbytes, (l1 - a) * fbytes); }
    }
};

}  // namespace aprilx
