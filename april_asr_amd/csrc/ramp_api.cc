// C ABI of the ramp merge (include/aprilx_engine.h): the pure window function and the two counters.  Kept apart
// from april_api.cc, as resample_api.cc, confidence_api.cc and search_options_api.cc are: the scheduler harness (tests/sched_harness)
// builds april_api.cc host-only against a fake engine, and these call engine code that is not inline.
#include <vector>
#include "../../include/april_api.h"
#include "../../include/aprilx_engine.h"
#include "common.h"
#include "session.h"
#include "api_handles.h"

using namespace aprilx;

extern "C" {

int aprilx_ramp_window(int L, int T, int R, int32_t *out, int cap)
{
    if (L <= 0 || T <= 0 || R <= 0 || !out) return -1;
    const std::vector<RampStep> w = ramp_window(L, T, R);
    const int stride = 3 + 2 * R;
    if ((int)w.size() * stride > cap) return -1;
    for (size_t i = 0; i < w.size(); ++i) {
        int32_t *o = out + i * (size_t)stride;
        for (int k = 0; k < stride; ++k) o[k] = -1;
        o[0] = w[i].macro; o[1] = w[i].own; o[2] = (int32_t)w[i].guests.size();
        for (size_t g = 0; g < w[i].guests.size() && (int)g < R; ++g) { o[3 + 2 * g] = w[i].guests[g].first; o[4 + 2 * g] = w[i].guests[g].second; }
    }
    return (int)w.size();
}
int aprilx_model_ramp_stats(AprilASRModel model, int device_index, uint64_t *ramp_hosted, uint64_t *ramp_eligible)
{
    if (!model || device_index < 0 || device_index >= (int)model->m.engines.size() || !ramp_hosted || !ramp_eligible) return -1;
    model->m.engines[(size_t)device_index]->ramp_counts(ramp_hosted, ramp_eligible);
    return 0;
}
int aprilx_model_ramp_stats2(AprilASRModel model, int device_index, uint64_t out[5])
{
    if (!model || device_index < 0 || device_index >= (int)model->m.engines.size() || !out) return -1;
    model->m.engines[(size_t)device_index]->ramp_counts(&out[0], &out[1]);
    model->m.engines[(size_t)device_index]->ramp_defer_counts(&out[2], &out[3], &out[4]);
    return 0;
}

}  // extern "C"
