// C ABI of DTMF detection (include/aprilx_engine.h "DTMF"): the per-session detector, the host statement of its
// contract (dtmf.h) for tests and for users without a GPU, and the kernel alone on given frames.  Kept apart from april_api.cc, as
// vad_api.cc is: the scheduler harness (tests/sched_harness) builds april_api.cc host-only against a fake engine.
#include <cstring>
#include <vector>
#include "../../include/april_api.h"
#include "../../include/aprilx_engine.h"
#include "common.h"
#include "session.h"
#include "api_handles.h"

using namespace aprilx;

static_assert(sizeof(AprilxDtmfPlan) == sizeof(DtmfPlan) && sizeof(AprilxDtmfMachine) == sizeof(DtmfMachine), "the public structs are the runtime's");

namespace {
// the public struct as the runtime's: false on a wrong size or non-zero flags (the ranges are dtmf_make_plan's)
bool to_options(const AprilxDtmfOptions *o, DtmfOptions *out)
{
    if (!o || o->size != sizeof(AprilxDtmfOptions) || o->flags != 0) return false;
    out->min_level_dbfs = o->min_level_dbfs; out->twist_hi_db = o->twist_hi_db; out->twist_lo_db = o->twist_lo_db; out->rel_peak_db = o->rel_peak_db;
    out->min_share = o->min_share; out->min_tone_ms = o->min_tone_ms; out->min_pause_ms = o->min_pause_ms;
    return true;
}
bool model_plan(const Model &m, const DtmfOptions &o, DtmfPlan *plan)
{
    return dtmf_make_plan(m.host.params.sample_rate, m.ftab.padded, m.host.params.frame_shift_ms, o, plan);
}
// a plan somebody hands in: what the loops below index with
bool plan_usable(const AprilxDtmfPlan *p) { return p && p->Wd > 0 && p->Wd <= kDtmfMaxW && p->on_frames >= 1 && p->off_frames >= 1; }
}  // namespace

extern "C" {

int aprilx_session_set_dtmf(AprilASRSession session, const AprilxDtmfOptions *options, AprilxDtmfHandler handler, void *userdata)
{
    if (!session) return -1;
    Session *s = &session->s;
    if (!options) return s->sched->set_dtmf(s, nullptr, nullptr, nullptr, nullptr) ? 0 : -1;
    DtmfOptions o; DtmfPlan plan;
    if (!handler || !to_options(options, &o) || !model_plan(*s->model, o, &plan)) return -1;
    return s->sched->set_dtmf(s, &o, &plan, handler, userdata) ? 0 : -1;
}

int aprilx_session_dtmf(AprilASRSession session, AprilxDtmfOptions *options_out, AprilxDtmfInfo *out)
{
    if (!session) return -1;
    Session *s = &session->s;
    s->sched->wait_idle(s);
    if (options_out) {
        const DtmfOptions &o = s->dtmf.opt;
        *options_out = AprilxDtmfOptions{(uint32_t)sizeof(AprilxDtmfOptions), o.min_level_dbfs, o.twist_hi_db, o.twist_lo_db, o.rel_peak_db, o.min_share,
                                         o.min_tone_ms, o.min_pause_ms, 0u};
    }
    if (out) {
        memset(out, 0, sizeof *out);
        out->frames_seen = s->real_frames;
        if (s->dtmf.on) {
            out->Wd = s->dtmf.plan.Wd; out->on_frames = s->dtmf.plan.on_frames; out->off_frames = s->dtmf.plan.off_frames;
            out->held = s->dtmf.m.held ? (uint32_t)(unsigned char)kDtmfDigits[s->dtmf.m.held - 1] : 0u;
            out->tone_frames = s->dtmf.tone; out->digits = s->dtmf.digits;
        }
    }
    return s->dtmf.on ? 1 : 0;
}

int aprilx_dtmf_plan(int sample_rate, int fft_size, int frame_shift_ms, const AprilxDtmfOptions *options, AprilxDtmfPlan *plan_out)
{
    DtmfOptions o; DtmfPlan plan;
    if (!plan_out || !to_options(options, &o) || !dtmf_make_plan(sample_rate, fft_size, frame_shift_ms, o, &plan)) return -1;
    memcpy(plan_out, &plan, sizeof plan);
    return 0;
}

int aprilx_dtmf_tables(int sample_rate, int Wd, float *out, size_t cap)
{
    if (sample_rate <= 0 || Wd <= 0 || Wd > kDtmfMaxW || !out || cap < (size_t)kDtmfRows * (size_t)Wd) return -1;
    dtmf_make_tables(sample_rate, Wd, out);
    return kDtmfRows * Wd;
}

int aprilx_dtmf_host(const AprilxDtmfPlan *plan, const float *tables, int n, const int16_t *frames, size_t ld, uint8_t *codes_out, float *powers_out)
{
    if (!plan_usable(plan) || !tables || n < 0 || (n && (!frames || !codes_out || ld < (size_t)plan->Wd))) return -1;
    DtmfPlan p;
    memcpy(&p, plan, sizeof p);
    dtmf_run_host(p, tables, n, frames, ld, codes_out, powers_out);
    return 0;
}

int aprilx_dtmf_decide_host(const AprilxDtmfPlan *plan, const float *powers9)
{
    if (!plan || !powers9) return -1;
    DtmfPlan p;
    memcpy(&p, plan, sizeof p);
    return dtmf_decide(p, powers9, powers9[8]);
}

int aprilx_dtmf_events_host(const AprilxDtmfPlan *plan, int frame_shift_ms, uint64_t t0, const uint8_t *codes, size_t n, int flush, AprilxDtmfMachine *machine,
                            int32_t *kinds_out, char *digits_out, uint64_t *times_out, int cap)
{
    if (!plan_usable(plan) || frame_shift_ms <= 0 || (n && !codes) || !machine || cap < 0 || (cap && (!kinds_out || !digits_out || !times_out))) return -1;
    if (machine->held < 0 || machine->held > 16 || machine->cand < 0 || machine->cand > 16 || machine->run < 0) return -1;
    DtmfPlan p; DtmfMachine m;
    memcpy(&p, plan, sizeof p); memcpy(&m, machine, sizeof m);
    int cnt = 0;
    auto emit = [&](int kind, char digit, uint64_t ms) {
        if (cnt < cap) { kinds_out[cnt] = kind; digits_out[cnt] = digit; times_out[cnt] = ms; }
        ++cnt;
    };
    dtmf_events(p, frame_shift_ms, t0, codes, n, m, emit);
    if (flush) dtmf_flush(frame_shift_ms, t0 + n, m, emit);
    memcpy(machine, &m, sizeof m);
    return cnt;
}

int aprilx_run_dtmf(AprilASRModel model, const AprilxDtmfOptions *options, int n_runs, const int32_t *n, const int16_t *frames, uint8_t *codes_out, float *powers_out)
{
    if (!model || model->m.engines.empty() || n_runs <= 0 || n_runs > 4096 || !options || !n || !frames || !codes_out) return -1;
    std::vector<DtmfPlan> plans((size_t)n_runs);
    int64_t total = 0;
    for (int r = 0; r < n_runs; ++r) {
        DtmfOptions o;
        if (!to_options(&options[r], &o) || !model_plan(model->m, o, &plans[(size_t)r]) || n[r] <= 0 || n[r] > (1 << 20)) return -1;
        total += n[r];
    }
    if (total * (int64_t)model->m.ftab.padded >= ((int64_t)1 << 31)) return -1;      // (FbankFrameDesc::pcm_off is 32 bits)
    model->m.engines[0]->debug_dtmf(n_runs, plans.data(), n, frames, codes_out, powers_out);
    return 0;
}

int aprilx_run_dtmf_decide(AprilASRModel model, const AprilxDtmfOptions *options, int n, const float *powers9, uint8_t *codes_out)
{
    DtmfOptions o; DtmfPlan plan;
    if (!model || model->m.engines.empty() || n <= 0 || n > (1 << 24) || !powers9 || !codes_out || !to_options(options, &o) || !model_plan(model->m, o, &plan)) return -1;
    model->m.engines[0]->debug_dtmf_decide(plan, n, powers9, codes_out);
    return 0;
}

int aprilx_model_dtmf_stats(AprilASRModel model, int device_index, uint64_t *launches, uint64_t *frames, double *ms)
{
    if (!model || device_index < 0 || device_index >= (int)model->m.engines.size() || !launches || !frames || !ms) return -1;
    const Engine *e = model->m.engines[(size_t)device_index];
    e->observer_counts(OBS_DTMF, launches, frames);
    *ms = e->timing(Engine::T_DTMF).ms;
    return 0;
}

}  // extern "C"
