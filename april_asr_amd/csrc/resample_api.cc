// C ABI of the input sample rate (include/aprilx_engine.h "input sample rate"): sessions that receive PCM16 at a rate of their own,
// and the conversion's contract (resample.h) for tests.  Kept apart from april_api.cc: the scheduler harness
// (tests/sched_harness) builds april_api.cc host-only against a fake engine.
#include <cstring>
#include "../../include/april_api.h"
#include "../../include/aprilx_engine.h"
#include "common.h"
#include "session.h"
#include "api_handles.h"

using namespace aprilx;

// ---- input sample rate (the reference takes PCM16 at aam_get_sample_rate() only, april-docs/src/python.md:79)
namespace {
const ResampleSpec *model_resampler(Model &m, uint32_t rate)
{
    std::lock_guard<std::mutex> g(m.mu);
    auto it = m.resamplers.find(rate);
    if (it != m.resamplers.end()) return &it->second;
    ResampleSpec spec;
    if (!resample_build(rate, (uint32_t)m.host.params.sample_rate, &spec)) return nullptr;
    return &(m.resamplers[rate] = std::move(spec));
}
}  // namespace

extern "C" {

int aprilx_session_set_input_rate(AprilASRSession session, uint32_t rate_hz)
{
    if (!session) return -1;
    Session *s = &session->s;
    const uint32_t model_rate = (uint32_t)s->model->host.params.sample_rate;
    const ResampleSpec *spec = nullptr;
    if (rate_hz != model_rate) {
        spec = model_resampler(*s->model, rate_hz);
        if (!spec) return -1;
    }
    return s->sched->set_input_rate(s, spec) ? 0 : -1;
}

uint32_t aprilx_session_input_rate(AprilASRSession session)
{
    if (!session) return 0;
    const Session *s = &session->s;
    const ResampleSpec *r = s->fb.rs;
    return r ? r->in_rate : (uint32_t)s->model->host.params.sample_rate;
}

int aprilx_resampler_taps(uint32_t in_rate, uint32_t out_rate, int32_t *lmk_out, float *taps, size_t cap)
{
    int L, M, K;
    if (!resample_plan(in_rate, out_rate, &L, &M, &K)) return -1;
    if (lmk_out) { lmk_out[0] = L; lmk_out[1] = M; lmk_out[2] = K; }
    const size_t n = (size_t)L * 2 * (size_t)K;
    if (taps && n) {
        if (cap < n) return -1;
        ResampleSpec spec;
        resample_build(in_rate, out_rate, &spec);
        for (int p = 0; p < L; ++p) memcpy(taps + (size_t)p * 2 * K, spec.taps.data() + (size_t)p * spec.ldt, (size_t)2 * K * sizeof(float));
    }
    return 0;
}

int64_t aprilx_resample(AprilASRModel model, uint32_t in_rate, const int16_t *pcm, size_t n, int16_t *out, size_t cap)
{
    if (!model || model->m.engines.empty() || (n && !pcm)) return -1;
    Model &m = model->m;
    const uint32_t model_rate = (uint32_t)m.host.params.sample_rate;
    int L, M, K;
    if (!resample_plan(in_rate, model_rate, &L, &M, &K)) return -1;
    const int64_t n_out = resample_total((int64_t)n, L, M);
    if ((int64_t)n + n_out > (int64_t)1 << 30 || (out == nullptr && n_out) || cap < (size_t)n_out) return -1;
    if (in_rate == model_rate) { if (n) memcpy(out, pcm, n * sizeof(int16_t)); return n_out; }
    const ResampleSpec *spec = model_resampler(m, in_rate);
    if (!spec) return -1;
    m.engines[0]->debug_resample(spec, pcm, n, out);
    return n_out;
}

}  // extern "C"
