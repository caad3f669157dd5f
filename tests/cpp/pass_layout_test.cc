// Stand-alone check of csrc/pass_layout.h under AddressSanitizer + UBSan (tests/test_pass_layout_cpu.py builds and runs it).
// The oracle is the text that computed the layout of a pass's output block before it was stated once -- in three places that had to
// agree byte for byte --, frozen literally below: FrontPass::quality_at_of(), the head of Engine::fbank(), the tail of
// Scheduler::cut_frames().  pass_layout() must equal all three for every combination of VAD and DTMF frames in
// {0, 1, 2, 3, 4, 5, 15, 16, 17, 1000} and tone and quality frames in {0, 1, 5}; and the parts must be aligned, must not overlap, and
// the block must end with its last non-empty part.
#include <cstdio>
#include <cstdlib>
#include "pass_layout.h"

using namespace aprilx;

static int fails = 0;
static long checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { if (fails < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static const int kWords = 8;      // kQualityWords when the text was frozen

// ---- the old text: FrontPass::quality_at_of
static size_t old_quality_at_of(size_t vad_bytes, size_t dtmf_bytes, size_t tone_bytes)
{
    const size_t end = tone_bytes ? (vad_bytes + dtmf_bytes + 3) / 4 * 4 + tone_bytes : vad_bytes + dtmf_bytes;
    return (end + 15) / 16 * 16;
}

// ---- the old text: the head of Engine::fbank(), from a pass that carries descriptors of every observer with frames (a pass's byte
// counts were frames x record size)
struct OldEngine {
    size_t vd_frames = 0, dt_frames = 0, tn_at = 0, tn_end = 0, qa_at = 0, out_bytes = 0;
    void call(size_t vad_bytes, size_t dtmf_bytes, size_t tone_bytes, size_t quality_bytes)
    {
        const int n_vd = vad_bytes ? 1 : 0, n_dt = dtmf_bytes ? 1 : 0, n_tn = tone_bytes ? 1 : 0, n_qa = quality_bytes ? 1 : 0;
        vd_frames = n_vd ? vad_bytes : 0;
        dt_frames = n_dt ? dtmf_bytes : 0;
        tn_at = (vd_frames + dt_frames + 3) / 4 * 4;
        const size_t tn_frames = n_tn ? tone_bytes / 4 : 0;
        tn_end = n_tn ? tn_at + tn_frames * 4 : vd_frames + dt_frames;
        qa_at = old_quality_at_of(vd_frames, dt_frames, tn_frames * 4);
        const size_t qa_frames = n_qa ? quality_bytes / (kWords * 4) : 0;
        out_bytes = n_qa ? qa_at + qa_frames * kWords * 4 : tn_end;
    }
};

// ---- the old text: the tail of Scheduler::cut_frames()
struct OldScheduler {
    size_t dtmf_at = 0, tone_at = 0, quality_at = 0;
    void call(int32_t vad_frames, int32_t dtmf_frames, int32_t tone_frames)
    {
        dtmf_at = (size_t)vad_frames;
        tone_at = ((size_t)vad_frames + (size_t)dtmf_frames + 3) / 4 * 4;
        quality_at = old_quality_at_of((size_t)vad_frames, (size_t)dtmf_frames, (size_t)tone_frames * 4);
    }
};

int main()
{
    CHECK(kQualityWords == kWords);
    CHECK(kPassParts[OBS_VAD].record == 1 && kPassParts[OBS_DTMF].record == 1 && kPassParts[OBS_TONE].record == 4 && kPassParts[OBS_QUALITY].record == (size_t)kWords * 4);
    const size_t bytes1[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 1000};
    const size_t records[] = {0, 1, 5};
    for (size_t vad : bytes1) for (size_t dtmf : bytes1) for (size_t tone : records) for (size_t quality : records) {
        const PassFrames f = {{vad, dtmf, tone, quality}};
        const PassLayout l = pass_layout(f);
        OldEngine e;
        e.call(vad, dtmf, tone * 4, quality * kWords * 4);
        OldScheduler s;
        s.call((int32_t)vad, (int32_t)dtmf, (int32_t)tone);
        // the engine: VAD bytes at 0, DTMF bytes behind them, tone records at tn_at, quality records at qa_at, out_bytes in all
        CHECK(l.at[OBS_VAD] == 0 && l.at[OBS_DTMF] == e.vd_frames && l.at[OBS_TONE] == e.tn_at && l.at[OBS_QUALITY] == e.qa_at && l.bytes == e.out_bytes);
        // the scheduler
        CHECK(l.at[OBS_DTMF] == s.dtmf_at && l.at[OBS_TONE] == s.tone_at && l.at[OBS_QUALITY] == s.quality_at);
        CHECK(l.at[OBS_QUALITY] == old_quality_at_of(vad, dtmf, tone * 4));
        // a record's place
        CHECK(l.record_at(OBS_VAD, 3) == 3 && l.record_at(OBS_DTMF, 3) == s.dtmf_at + 3 && l.record_at(OBS_TONE, 3) == s.tone_at + 12 &&
              l.record_at(OBS_QUALITY, 3) == s.quality_at + 3 * (size_t)kWords * 4);
        // alignment
        if (tone) CHECK(l.at[OBS_TONE] % 4 == 0);
        CHECK(l.at[OBS_QUALITY] % 16 == 0);
        // no two non-empty parts overlap (the parts are in block order: each starts at or behind the end of the one before it), and the
        // block ends with the last non-empty part
        size_t end = 0;
        for (int o = 0; o < OBS_COUNT; ++o) {
            if (!f[(size_t)o]) continue;
            CHECK(l.at[o] >= end);
            end = l.at[o] + f[(size_t)o] * kPassParts[o].record;
        }
        CHECK(l.bytes == end);
    }
    if (fails) { printf("%d of %ld checks FAILED\n", fails, checks); return 1; }
    printf("all checks passed (%ld)\n", checks);
    return 0;
}
