// C ABI of tone detection (include/aprilx_engine.h "Tones"): the per-session detector, the host statement of its
// contract (tone.h) for tests and for users without a GPU, and the kernel alone on given frames.  Kept apart from april_api.cc, as
// dtmf_api.cc is: the scheduler harness (tests/sched_harness) builds april_api.cc host-only against a fake engine.
#include <cstring>
#include <vector>
#include "../../include/april_api.h"
#include "../../include/aprilx_engine.h"
#include "common.h"
#include "session.h"
#include "api_handles.h"

using namespace aprilx;

static_assert(sizeof(AprilxTonePlan) == sizeof(TonePlan) && sizeof(AprilxToneMachine) == sizeof(ToneMachine), "the public structs are the runtime's");
static_assert((int)APRILX_TONE_ON == (int)TONE_ON && (int)APRILX_TONE_OFF == (int)TONE_OFF, "the public kinds are the runtime's");

namespace {
// the public struct as the runtime's: false on a wrong size or non-zero flags (the ranges are tone_make_plan's)
bool to_options(const AprilxToneOptions *o, ToneOptions *out)
{
    if (!o || o->size != sizeof(AprilxToneOptions) || o->flags != 0) return false;
    out->min_level_dbfs = o->min_level_dbfs; out->second_db = o->second_db; out->min_share = o->min_share;
    out->tol_hz = o->tol_hz; out->min_tone_ms = o->min_tone_ms; out->min_pause_ms = o->min_pause_ms;
    return true;
}
bool model_plan(const Model &m, const ToneOptions &o, TonePlan *plan)
{
    return tone_make_plan(m.host.params.sample_rate, m.ftab.padded, m.host.params.frame_shift_ms, o, plan);
}
// a plan somebody hands in: what the loops below index with
bool plan_usable(const AprilxTonePlan *p)
{
    return p && p->W >= kToneLanes && p->W <= kToneMaxW && p->W % kToneLanes == 0 && p->F >= 1 && p->F <= kToneMaxF && p->k_lo >= 0 && p->on_frames >= 1 &&
           p->off_frames >= 1 && p->tol_hz >= 0;
}
// records cross the ABI as [n][2] uint16 (any alignment); inside they are lo | hi << 16
void put_records(const std::vector<uint32_t> &r, uint16_t *out)
{
    for (size_t i = 0; i < r.size(); ++i) { out[2 * i] = (uint16_t)(r[i] & 0xffffu); out[2 * i + 1] = (uint16_t)(r[i] >> 16); }
}
}  // namespace

extern "C" {

int aprilx_session_set_tones(AprilASRSession session, const AprilxToneOptions *options, AprilxToneHandler handler, void *userdata)
{
    if (!session) return -1;
    Session *s = &session->s;
    if (!options) return s->sched->set_tones(s, nullptr, nullptr, nullptr, nullptr) ? 0 : -1;
    ToneOptions o; TonePlan plan;
    if (!handler || !to_options(options, &o) || !model_plan(*s->model, o, &plan)) return -1;
    return s->sched->set_tones(s, &o, &plan, handler, userdata) ? 0 : -1;
}

int aprilx_session_tones(AprilASRSession session, AprilxToneOptions *options_out, AprilxToneInfo *out)
{
    if (!session) return -1;
    Session *s = &session->s;
    s->sched->wait_idle(s);
    if (options_out) {
        const ToneOptions &o = s->tones.opt;
        *options_out = AprilxToneOptions{(uint32_t)sizeof(AprilxToneOptions), o.min_level_dbfs, o.second_db, o.min_share, o.tol_hz, o.min_tone_ms, o.min_pause_ms, 0u};
    }
    if (out) {
        memset(out, 0, sizeof *out);
        out->frames_seen = s->real_frames;
        if (s->tones.on) {
            const TonePlan &p = s->tones.plan;
            out->W = p.W; out->k_lo = p.k_lo; out->F = p.F; out->on_frames = p.on_frames; out->off_frames = p.off_frames;
            if (s->tones.m.held) { out->held_f1 = (uint32_t)s->tones.m.h1; out->held_f2 = (uint32_t)s->tones.m.h2; }
            out->tonal_frames = s->tones.tonal; out->tones = s->tones.tones;
        }
    }
    return s->tones.on ? 1 : 0;
}

int aprilx_tone_plan(int sample_rate, int fft_size, int frame_shift_ms, const AprilxToneOptions *options, AprilxTonePlan *plan_out)
{
    ToneOptions o; TonePlan plan;
    if (!plan_out || !to_options(options, &o) || !tone_make_plan(sample_rate, fft_size, frame_shift_ms, o, &plan)) return -1;
    memcpy(plan_out, &plan, sizeof plan);
    return 0;
}

int aprilx_tone_tables(int sample_rate, int fft_size, float *out, size_t cap)
{
    int w, k_lo, f;
    if (!out || !tone_grid(sample_rate, fft_size, &w, &k_lo, &f) || cap < (size_t)2 * (size_t)f * (size_t)w) return -1;
    tone_make_tables(w, k_lo, f, out);
    return 2 * f * w;
}

int aprilx_tone_host(const AprilxTonePlan *plan, const float *tables, int n, const int16_t *frames, size_t ld, uint16_t *records_out, float *powers_out)
{
    if (!plan_usable(plan) || !tables || n < 0 || (n && (!frames || !records_out || ld < (size_t)plan->W))) return -1;
    TonePlan p;
    memcpy(&p, plan, sizeof p);
    std::vector<uint32_t> rec((size_t)n);
    tone_run_host(p, tables, n, frames, ld, rec.data(), powers_out);
    put_records(rec, records_out);
    return 0;
}

int64_t aprilx_tone_decide_host(const AprilxTonePlan *plan, const float *powers)
{
    if (!plan_usable(plan) || !powers) return -1;
    TonePlan p;
    memcpy(&p, plan, sizeof p);
    return (int64_t)tone_decide(p, powers, powers[p.F]);
}

int aprilx_tone_events_host(const AprilxTonePlan *plan, int frame_shift_ms, uint64_t t0, const uint16_t *records, size_t n, int flush, AprilxToneMachine *machine,
                            int32_t *kinds_out, uint32_t *f1_out, uint32_t *f2_out, uint64_t *times_out, int cap)
{
    if (!plan_usable(plan) || frame_shift_ms <= 0 || (n && !records) || !machine || cap < 0 || (cap && (!kinds_out || !f1_out || !f2_out || !times_out))) return -1;
    auto hz = [](int32_t v) { return v >= 0 && v <= 65535; };
    if (machine->held < 0 || machine->held > 1 || !hz(machine->h1) || !hz(machine->h2) || !hz(machine->c1) || !hz(machine->c2) || machine->run < 0) return -1;
    TonePlan p; ToneMachine m;
    memcpy(&p, plan, sizeof p); memcpy(&m, machine, sizeof m);
    std::vector<uint32_t> rec(n);
    for (size_t i = 0; i < n; ++i) rec[i] = (uint32_t)records[2 * i] | (uint32_t)records[2 * i + 1] << 16;
    int cnt = 0;
    auto emit = [&](int kind, uint32_t f1, uint32_t f2, uint64_t ms) {
        if (cnt < cap) { kinds_out[cnt] = kind; f1_out[cnt] = f1; f2_out[cnt] = f2; times_out[cnt] = ms; }
        ++cnt;
    };
    tone_events(p, frame_shift_ms, t0, rec.data(), n, m, emit);
    if (flush) tone_flush(frame_shift_ms, t0 + n, m, emit);
    memcpy(machine, &m, sizeof m);
    return cnt;
}

const char *aprilx_tone_name(uint32_t f1_hz, uint32_t f2_hz, uint32_t tol_hz)
{
    if (f1_hz > 65535u || f2_hz > 65535u) return nullptr;
    return tone_name(f1_hz, f2_hz, tol_hz);
}

int aprilx_run_tones(AprilASRModel model, const AprilxToneOptions *options, int n_runs, const int32_t *n, const int16_t *frames, uint16_t *records_out, float *powers_out)
{
    if (!model || model->m.engines.empty() || n_runs <= 0 || n_runs > 4096 || !options || !n || !frames || !records_out) return -1;
    std::vector<TonePlan> plans((size_t)n_runs);
    int64_t total = 0;
    for (int r = 0; r < n_runs; ++r) {
        ToneOptions o;
        if (!to_options(&options[r], &o) || !model_plan(model->m, o, &plans[(size_t)r]) || n[r] <= 0 || n[r] > (1 << 20)) return -1;
        total += n[r];
    }
    if (total * (int64_t)model->m.ftab.padded >= ((int64_t)1 << 31)) return -1;      // (FbankFrameDesc::pcm_off is 32 bits)
    std::vector<uint32_t> rec((size_t)total);
    model->m.engines[0]->debug_tones(n_runs, plans.data(), n, frames, rec.data(), powers_out);
    put_records(rec, records_out);
    return 0;
}

int aprilx_run_tone_decide(AprilASRModel model, const AprilxToneOptions *options, int n, const float *powers, uint16_t *records_out)
{
    ToneOptions o; TonePlan plan;
    if (!model || model->m.engines.empty() || n <= 0 || n > (1 << 20) || !powers || !records_out || !to_options(options, &o) || !model_plan(model->m, o, &plan)) return -1;
    std::vector<uint32_t> rec((size_t)n);
    model->m.engines[0]->debug_tone_decide(plan, n, powers, rec.data());
    put_records(rec, records_out);
    return 0;
}

int aprilx_model_tone_stats(AprilASRModel model, int device_index, uint64_t *launches, uint64_t *frames, double *ms)
{
    if (!model || device_index < 0 || device_index >= (int)model->m.engines.size() || !launches || !frames || !ms) return -1;
    const Engine *e = model->m.engines[(size_t)device_index];
    e->observer_counts(OBS_TONE, launches, frames);
    *ms = e->timing(Engine::T_TONE).ms;
    return 0;
}

}  // extern "C"
