// C ABI of the input format (include/aprilx_engine.h "input format"): sessions that are fed G.711, float32 or
// interleaved multi-channel audio, the byte-counted feed calls, and the decode contract (input_format.h) for tests.  Kept apart from
// april_api.cc, as resample_api.cc is: the scheduler harness (tests/sched_harness) builds april_api.cc host-only against a fake engine.
#include <cstring>
#include <vector>
#include "../../include/april_api.h"
#include "../../include/aprilx_engine.h"
#include "common.h"
#include "session.h"
#include "api_handles.h"

using namespace aprilx;

#include "group_feed.h"

namespace {
// the public struct as the runtime's: false on a wrong size or a value out of range; the default {S16, 1, 0} is "no format"
bool to_format(const AprilxInputFormat *f, InputFormat *out)
{
    *out = InputFormat();
    if (!f) return true;
    if (f->size != sizeof(AprilxInputFormat) || !input_format_valid(f->encoding, f->channels, f->channel)) return false;
    if (input_format_default(f->encoding, f->channels, f->channel)) return true;
    out->encoding = f->encoding; out->channels = f->channels; out->channel = f->channel;
    out->frame_bytes = f->channels * encoding_bytes(f->encoding);
    return true;
}

size_t frame_bytes_of(const Session &s) { return s.frame_bytes ? s.frame_bytes : sizeof(int16_t); }
}  // namespace

extern "C" {

int aprilx_session_set_input_format(AprilASRSession session, const AprilxInputFormat *format)
{
    InputFormat f;
    if (!session || !to_format(format, &f)) return -1;
    Session *s = &session->s;
    return s->sched->set_input_format(s, f) ? 0 : -1;
}

int aprilx_session_input_format(AprilASRSession session, AprilxInputFormat *out)
{
    if (!session || !out) return -1;
    const InputFormat &f = session->s.fb.fmt;
    out->size = (uint32_t)sizeof(AprilxInputFormat);
    out->encoding = f ? f.encoding : (uint32_t)APRILX_ENC_S16; out->channels = f ? f.channels : 1u; out->channel = f ? f.channel : 0;
    return f ? 1 : 0;
}

int aprilx_session_feed_bytes(AprilASRSession session, const void *data, size_t bytes)
{
    if (!session || (bytes && !data)) return -1;
    Session *s = &session->s;
    const short *p = static_cast<const short *>(data);
    if (!s->sched->submit(1, &s, &p, &bytes, false, s->sync_mode, /*borrow=*/s->sync_mode, /*bytes=*/true)) return -1;
    if (s->sync_mode) s->sched->deliver_sync_events(s);
    return 0;
}

int aprilx_feed_many_bytes(size_t n, AprilASRSession *sessions, const void *const *data, const size_t *byte_counts, int depth)
{
    if (n && (!sessions || !data || !byte_counts)) return -1;
    // (a session's format only changes while it is idle, by the thread that feeds it: read here without the schedulers' locks, so
    // that a partial frame is found before anything is queued on any GPU)
    for (size_t i = 0; i < n; ++i) if (!sessions[i] || byte_counts[i] % frame_bytes_of(sessions[i]->s) || (byte_counts[i] && !data[i])) return -1;
    // depth 0: aprilx_feed_many (the buffers are lent until every session is idle again); depth >= 1: aprilx_feed_many_pipelined
    const short *const *pcm = reinterpret_cast<const short *const *>(data);
    bool ok;
    if (depth <= 0) ok = feed_groups(n, sessions, pcm, byte_counts, /*borrow=*/true, /*bytes=*/true, [](SchedGroup &g) { g.sched->wait_idle_many(g.ss.data(), (int)g.ss.size()); });
    else ok = feed_groups(n, sessions, pcm, byte_counts, /*borrow=*/false, /*bytes=*/true, [&](SchedGroup &g) { g.sched->wait_backlog(g.ss.data(), (int)g.ss.size(), (uint64_t)(depth - 1)); });
    return ok ? 0 : -1;
}

int64_t aprilx_decode_host(const AprilxInputFormat *format, const void *data, size_t bytes, int16_t *out, size_t cap)
{
    if (!format || format->size != sizeof(AprilxInputFormat) || !input_format_valid(format->encoding, format->channels, format->channel)) return -1;
    InputFormat f;
    f.encoding = format->encoding; f.channels = format->channels; f.channel = format->channel;
    f.frame_bytes = format->channels * encoding_bytes(format->encoding);
    if (bytes % f.frame_bytes || (bytes && !data)) return -1;
    const size_t n = bytes / f.frame_bytes;
    if (cap < n || (n && !out)) return -1;
    const uint8_t *p = static_cast<const uint8_t *>(data);
    for (size_t i = 0; i < n; ++i) out[i] = decode_frame(f, p + i * f.frame_bytes);
    return (int64_t)n;
}

int64_t aprilx_decode(AprilASRModel model, const AprilxInputFormat *format, const void *data, size_t bytes, int16_t *out, size_t cap)
{
    if (!model || model->m.engines.empty() || !format || format->size != sizeof(AprilxInputFormat)
        || !input_format_valid(format->encoding, format->channels, format->channel)) return -1;
    const size_t fb = format->channels * encoding_bytes(format->encoding);
    if (bytes % fb || (bytes && !data)) return -1;
    const size_t n = bytes / fb;
    if (cap < n || (n && !out) || n > ((size_t)1 << 30)) return -1;
    model->m.engines[0]->debug_decode(format->encoding, format->channels, format->channel, data, n, out);
    return (int64_t)n;
}

int aprilx_model_decode_stats(AprilASRModel model, int device_index, uint64_t *launches, uint64_t *frames, double *ms)
{
    if (!model || device_index < 0 || device_index >= (int)model->m.engines.size() || !launches || !frames || !ms) return -1;
    const Engine *e = model->m.engines[(size_t)device_index];
    e->decode_counts(launches, frames);
    *ms = e->timing(Engine::T_DECODE).ms;
    return 0;
}

}  // extern "C"
