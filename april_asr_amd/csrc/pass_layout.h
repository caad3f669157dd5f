// The block a front-end pass's frame observers write (Engine::fbank() returns it, Scheduler::harvest() reads it), stated once: one part
// per observer in one fixed order -- voice activity, DTMF, tones, line quality --, each a record per frame of that observer's runs in the
// pass, each part at its alignment behind the last part that HAS records (a part without records moves nothing behind it).  A run's
// out_off / off counts records from the start of its observer's part.  Pure arithmetic, no HIP: tests/cpp/pass_layout_test.cc holds it
// against the three formulas it replaced.
#pragma once
#include <array>
#include <cstddef>
#include "quality.h"

namespace aprilx {

enum Observer { OBS_VAD = 0, OBS_DTMF = 1, OBS_TONE = 2, OBS_QUALITY = 3, OBS_COUNT = 4 };      // in block order

// bytes per record and alignment of every part: a VAD and a DTMF byte, a tone record of one word, a quality record of kQualityWords words
struct PassPart { size_t record, align; };
constexpr PassPart kPassParts[OBS_COUNT] = {{1, 1}, {1, 1}, {4, 4}, {(size_t)kQualityWords * 4, 16}};

typedef std::array<size_t, OBS_COUNT> PassFrames;      // frames (= records) per observer in one pass

struct PassLayout {
    size_t at[OBS_COUNT] = {0, 0, 0, 0};       // byte offset of every part
    size_t bytes = 0;                          // the block's length: the end of the last part with records
    size_t record_at(int o, size_t off) const { return at[o] + off * kPassParts[o].record; }      // byte offset of record `off` of observer o
};

inline PassLayout pass_layout(const PassFrames &frames)
{
    PassLayout l;
    for (int o = 0; o < OBS_COUNT; ++o) {
        l.at[o] = (l.bytes + kPassParts[o].align - 1) / kPassParts[o].align * kPassParts[o].align;
        if (frames[(size_t)o]) l.bytes = l.at[o] + frames[(size_t)o] * kPassParts[o].record;
    }
    return l;
}

}  // namespace aprilx
