// C ABI of voice activity (include/aprilx_engine.h "voice activity"): the per-session detector, the host
// statement of its contract (vad.h) for tests and for users without a GPU, and the kernel alone on given rows.  Kept apart from
// april_api.cc, as input_format_api.cc is: the scheduler harness (tests/sched_harness) builds april_api.cc host-only against a fake engine.
#include <cstring>
#include <vector>
#include "../../include/april_api.h"
#include "../../include/aprilx_engine.h"
#include "common.h"
#include "session.h"
#include "api_handles.h"

using namespace aprilx;

static_assert(sizeof(AprilxVadPlan) == sizeof(VadPlan) && sizeof(AprilxVadState) == sizeof(VadState), "the public structs are the runtime's");

namespace {
// the public struct as the runtime's: false on a wrong size or non-zero flags (the ranges are vad_make_plan's)
bool to_options(const AprilxVadOptions *o, VadOptions *out)
{
    if (!o || o->size != sizeof(AprilxVadOptions) || o->flags != 0) return false;
    out->band_lo_hz = o->band_lo_hz; out->band_hi_hz = o->band_hi_hz; out->onset_db = o->onset_db; out->offset_db = o->offset_db;
    out->onset_ms = o->onset_ms; out->hangover_ms = o->hangover_ms; out->min_energy = o->min_energy;
    return true;
}
bool model_plan(const Model &m, const VadOptions &o, VadPlan *plan)
{
    return vad_make_plan(m.ftab.mel.data(), m.ftab.nbins, m.ftab.nfft_bins, m.host.params.sample_rate, m.host.params.frame_shift_ms, o, plan);
}
}  // namespace

extern "C" {

int aprilx_session_set_vad(AprilASRSession session, const AprilxVadOptions *options, AprilxVadHandler handler, void *userdata)
{
    if (!session) return -1;
    Session *s = &session->s;
    if (!options) return s->sched->set_vad(s, nullptr, nullptr, nullptr, nullptr) ? 0 : -1;
    VadOptions o; VadPlan plan;
    if (!handler || !to_options(options, &o) || !model_plan(*s->model, o, &plan)) return -1;
    return s->sched->set_vad(s, &o, &plan, handler, userdata) ? 0 : -1;
}

int aprilx_session_vad(AprilASRSession session, AprilxVadOptions *options_out, AprilxVadInfo *out)
{
    if (!session) return -1;
    Session *s = &session->s;
    s->sched->wait_idle(s);
    if (options_out) {
        const VadOptions &o = s->vad.opt;
        *options_out = AprilxVadOptions{(uint32_t)sizeof(AprilxVadOptions), o.band_lo_hz, o.band_hi_hz, o.onset_db, o.offset_db, o.onset_ms, o.hangover_ms, o.min_energy, 0u};
    }
    if (out) {
        memset(out, 0, sizeof *out);
        out->frames_seen = s->real_frames;
        if (s->vad.on) {
            out->b0 = s->vad.plan.b0; out->b1 = s->vad.plan.b1; out->onset_frames = s->vad.plan.onset_frames; out->hangover_frames = s->vad.plan.hangover_frames;
            out->speech_frames = s->vad.speech; out->in_speech = (uint32_t)s->vad.last; out->segments = s->vad.segments;
        }
    }
    return s->vad.on ? 1 : 0;
}

int aprilx_vad_plan_tables(const float *mel, int nbins, int nfft_bins, int sample_rate, int frame_shift_ms, const AprilxVadOptions *options, AprilxVadPlan *plan_out)
{
    VadOptions o; VadPlan plan;
    if (!plan_out || !to_options(options, &o) || !vad_make_plan(mel, nbins, nfft_bins, sample_rate, frame_shift_ms, o, &plan)) return -1;
    memcpy(plan_out, &plan, sizeof plan);
    return 0;
}

int aprilx_vad_host(const AprilxVadPlan *plan, int n, int nbins, const float *rows, AprilxVadState *state_inout, uint8_t *bytes_out, float *energy_out)
{
    if (!plan || n < 0 || nbins <= 0 || !state_inout || (n && (!rows || !bytes_out)) || plan->b0 < 0 || plan->b0 >= plan->b1 || plan->b1 > nbins) return -1;
    VadPlan p; VadState v;
    memcpy(&p, plan, sizeof p); memcpy(&v, state_inout, sizeof v);
    if (v.pos < 0 || v.pos >= kVadSubWindows) return -1;
    vad_run_host(p, n, rows, (size_t)nbins, v, bytes_out, energy_out);
    memcpy(state_inout, &v, sizeof v);
    return 0;
}

int aprilx_vad_events_host(const AprilxVadPlan *plan, int frame_shift_ms, uint64_t t0, const uint8_t *bytes, size_t n, int32_t *last_bit, int32_t *kinds_out,
                           uint64_t *times_out, int cap)
{
    if (!plan || frame_shift_ms <= 0 || (n && !bytes) || !last_bit || cap < 0 || (cap && (!kinds_out || !times_out))) return -1;
    VadPlan p;
    memcpy(&p, plan, sizeof p);
    int cnt = 0;
    *last_bit = vad_events(p, frame_shift_ms, t0, bytes, n, *last_bit & 1, [&](int kind, uint64_t ms) {
        if (cnt < cap) { kinds_out[cnt] = kind; times_out[cnt] = ms; }
        ++cnt;
    });
    return cnt;
}

int aprilx_run_vad(AprilASRModel model, int n_runs, const AprilxVadOptions *options, const int32_t *n, const int32_t *first_row, const float *rows,
                   AprilxVadState *states_inout, uint8_t *bytes_out, float *energy_out)
{
    if (!model || model->m.engines.empty() || n_runs <= 0 || n_runs > 4096 || !options || !n || !first_row || !rows || !states_inout || !bytes_out) return -1;
    std::vector<VadPlan> plans((size_t)n_runs);
    int R = 0;
    for (int r = 0; r < n_runs; ++r) {
        VadOptions o;
        if (!to_options(&options[r], &o) || !model_plan(model->m, o, &plans[(size_t)r]) || n[r] <= 0 || n[r] > (1 << 20)) return -1;
        if (states_inout[r].pos < 0 || states_inout[r].pos >= kVadSubWindows) return -1;
        R = n[r] > R ? n[r] : R;
    }
    for (int r = 0; r < n_runs; ++r) if (first_row[r] < 0 || first_row[r] >= R) return -1;
    model->m.engines[0]->debug_vad(n_runs, plans.data(), n, first_row, R, rows, reinterpret_cast<VadState *>(states_inout), bytes_out, energy_out);
    return 0;
}

int aprilx_model_vad_stats(AprilASRModel model, int device_index, uint64_t *launches, uint64_t *frames, double *ms)
{
    if (!model || device_index < 0 || device_index >= (int)model->m.engines.size() || !launches || !frames || !ms) return -1;
    const Engine *e = model->m.engines[(size_t)device_index];
    e->observer_counts(OBS_VAD, launches, frames);
    *ms = e->timing(Engine::T_VAD).ms;
    return 0;
}

}  // extern "C"
