// C ABI of the line-quality observer (include/aprilx_engine.h "Line quality"): the per-session observer, the host
// statement of its contract (quality.h) for tests and for users without a GPU, and the kernel alone on given frames.  Kept apart from
// april_api.cc, as tone_api.cc is: the scheduler harness (tests/sched_harness) builds april_api.cc host-only against a fake engine.
#include <cstddef>
#include <cstring>
#include <vector>
#include "../../include/april_api.h"
#include "../../include/aprilx_engine.h"
#include "common.h"
#include "session.h"
#include "api_handles.h"

using namespace aprilx;

static_assert(sizeof(AprilxQualityPlan) == sizeof(QualityPlan) && sizeof(AprilxQualityMachine) == sizeof(QualityMachine) &&
              sizeof(AprilxQualityEvent) == sizeof(QualityEvent), "the public structs are the runtime's");
static_assert(offsetof(AprilxQualityEvent, quiet_sumsq) == offsetof(QualityEvent, quiet_sumsq) && offsetof(AprilxQualityEvent, hop) == offsetof(QualityEvent, hop) &&
              offsetof(AprilxQualityMachine, quiet_sumsq) == offsetof(QualityMachine, quiet_sumsq), "... field for field");
static_assert((int)APRILX_QUALITY_REPORT == (int)QUALITY_REPORT && (int)APRILX_QUALITY_CLIPPING_ON == (int)QUALITY_CLIPPING_ON &&
              (int)APRILX_QUALITY_CLIPPING_OFF == (int)QUALITY_CLIPPING_OFF && (int)APRILX_QUALITY_DROPOUT_ON == (int)QUALITY_DROPOUT_ON &&
              (int)APRILX_QUALITY_DROPOUT_OFF == (int)QUALITY_DROPOUT_OFF, "the public kinds are the runtime's");

namespace {
// the public struct as the runtime's: false on a wrong size or non-zero flags (the ranges are quality_make_plan's)
bool to_options(const AprilxQualityOptions *o, QualityOptions *out)
{
    if (!o || o->size != sizeof(AprilxQualityOptions) || o->flags != 0) return false;
    out->clip_level = o->clip_level; out->clip_run_min = o->clip_run_min; out->clip_hold_ms = o->clip_hold_ms;
    out->dropout_ms = o->dropout_ms; out->report_ms = o->report_ms;
    return true;
}
bool model_plan(const Model &m, const QualityOptions &o, QualityPlan *plan)
{
    // (the hop the engine walks is the filterbank's: a model whose shift in samples is not shift_ms * rate / 1000 is refused)
    return quality_make_plan(m.host.params.sample_rate, m.ftab.padded, m.host.params.frame_shift_ms, o, plan) && plan->hop == m.ftab.shift;
}
// a plan somebody hands in: what the machine counts with
bool plan_usable(const AprilxQualityPlan *p)
{
    return p && p->hop >= 1 && p->hop <= kQualityMaxHop && p->clip_level >= 1024 && p->clip_level <= 32767 && p->clip_run_min >= 1 && p->clip_run_min <= 64 &&
           p->hold_frames >= 1 && p->dropout_frames >= 1 && p->report_frames >= 0;
}
}  // namespace

extern "C" {

int aprilx_session_set_quality(AprilASRSession session, const AprilxQualityOptions *options, AprilxQualityHandler handler, void *userdata)
{
    if (!session) return -1;
    Session *s = &session->s;
    if (!options) return s->sched->set_quality(s, nullptr, nullptr, nullptr, nullptr) ? 0 : -1;
    QualityOptions o; QualityPlan plan;
    if (!handler || !to_options(options, &o) || !model_plan(*s->model, o, &plan)) return -1;
    return s->sched->set_quality(s, &o, &plan, handler, userdata) ? 0 : -1;
}

int aprilx_session_quality(AprilASRSession session, AprilxQualityOptions *options_out, AprilxQualityInfo *out)
{
    if (!session) return -1;
    Session *s = &session->s;
    s->sched->wait_idle(s);
    if (options_out) {
        const QualityOptions &o = s->quality.opt;
        *options_out = AprilxQualityOptions{(uint32_t)sizeof(AprilxQualityOptions), 0u, o.clip_level, o.clip_run_min, o.clip_hold_ms, o.dropout_ms, o.report_ms};
    }
    if (out) {
        memset(out, 0, sizeof *out);
        out->frames_seen = s->real_frames;
        if (s->quality.on) {
            const QualityPlan &p = s->quality.plan;
            out->hop = p.hop; out->hold_frames = p.hold_frames; out->dropout_frames = p.dropout_frames; out->report_frames = p.report_frames;
            out->clipping = (uint32_t)s->quality.m.clipping; out->dropout = (uint32_t)s->quality.m.dropout;
            out->frames = s->quality.frames; out->clipped_frames = s->quality.clipped; out->dead_frames = s->quality.dead;
            out->clip_samples = s->quality.clip_samples; out->reports = s->quality.reports;
        }
    }
    return s->quality.on ? 1 : 0;
}

int aprilx_quality_plan(int sample_rate, int frame_samples, int frame_shift_ms, const AprilxQualityOptions *options, AprilxQualityPlan *plan_out)
{
    QualityOptions o; QualityPlan plan;
    if (!plan_out || !to_options(options, &o) || !quality_make_plan(sample_rate, frame_samples, frame_shift_ms, o, &plan)) return -1;
    memcpy(plan_out, &plan, sizeof plan);
    return 0;
}

int aprilx_quality_host(int hop, int clip_level, int n, const int16_t *frames, size_t ld, uint32_t *records_out)
{
    if (hop < 1 || hop > kQualityMaxHop || clip_level < 1024 || clip_level > 32767 || n < 0 || (n && (!frames || !records_out || ld < (size_t)hop))) return -1;
    quality_run_host(hop, clip_level, n, frames, ld, records_out);
    return 0;
}

int aprilx_quality_events_host(const AprilxQualityPlan *plan, int frame_shift_ms, uint64_t t0, const uint32_t *records, size_t n, int flush,
                               AprilxQualityMachine *machine, AprilxQualityEvent *events_out, int cap)
{
    if (!plan_usable(plan) || frame_shift_ms <= 0 || (n && !records) || !machine || cap < 0 || (cap && !events_out)) return -1;
    if (machine->clipping < 0 || machine->clipping > 1 || machine->dropout < 0 || machine->dropout > 1 || machine->quiet_run < 0 || machine->dead_run < 0) return -1;
    QualityPlan p; QualityMachine m;
    memcpy(&p, plan, sizeof p); memcpy(&m, machine, sizeof m);
    int cnt = 0;
    auto emit = [&](const QualityEvent &e) {
        if (cnt < cap) memcpy(&events_out[cnt], &e, sizeof e);
        ++cnt;
    };
    quality_events(p, frame_shift_ms, t0, records, n, m, emit);
    if (flush) quality_flush(p, frame_shift_ms, t0 + n, m, emit);
    memcpy(machine, &m, sizeof m);
    return cnt;
}

int aprilx_run_quality(AprilASRModel model, const int32_t *clip_levels, int n_runs, const int32_t *n, const int16_t *frames, uint32_t *records_out)
{
    if (!model || model->m.engines.empty() || n_runs <= 0 || n_runs > 4096 || !clip_levels || !n || !frames || !records_out) return -1;
    const int hop = model->m.ftab.shift, padded = model->m.ftab.padded;
    if (hop < 1 || hop > padded || hop > kQualityMaxHop) return -1;
    int64_t total = 0;
    for (int r = 0; r < n_runs; ++r) {
        if (clip_levels[r] < 1024 || clip_levels[r] > 32767 || n[r] <= 0 || n[r] > (1 << 20)) return -1;
        total += n[r];
    }
    if (total * (int64_t)padded >= ((int64_t)1 << 31)) return -1;      // (FbankFrameDesc::pcm_off is 32 bits)
    model->m.engines[0]->debug_quality(hop, n_runs, clip_levels, n, frames, records_out);
    return 0;
}

int aprilx_model_quality_stats(AprilASRModel model, int device_index, uint64_t *launches, uint64_t *frames, double *ms)
{
    if (!model || device_index < 0 || device_index >= (int)model->m.engines.size() || !launches || !frames || !ms) return -1;
    const Engine *e = model->m.engines[(size_t)device_index];
    e->observer_counts(OBS_QUALITY, launches, frames);
    *ms = e->timing(Engine::T_QUALITY).ms;
    return 0;
}

}  // extern "C"
