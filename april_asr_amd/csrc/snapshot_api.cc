// C ABI of session snapshot / restore (include/aprilx_engine.h "session snapshot and restore").  Kept apart from
// april_api.cc, as the detectors' files are: the scheduler harness (tests/sched_harness) builds april_api.cc host-only against a fake
// engine, and these entry points reach Engine members that engine has not.
#include <cstring>
#include <string>
#include <vector>
#include "../../include/april_api.h"
#include "../../include/aprilx_engine.h"
#include "common.h"
#include "snapshot.h"
#include "api_handles.h"

namespace aprilx {
void snapshot_sessions(size_t n, Session *const *ss, std::vector<uint8_t> *out, bool *ok, bool sizes_only);
void restore_sessions(size_t n, Session *const *ss, const void *const *blobs, const size_t *sizes, int *status, std::string *errs);
}
using namespace aprilx;

extern "C" {

int aprilx_snapshot_many(size_t n, AprilASRSession *sessions, void *const *dsts, const size_t *caps, int64_t *sizes_out)
{
    if (!sessions || !sizes_out || (dsts && !caps)) return -1;
    for (size_t i = 0; i < n; ++i) if (!sessions[i]) return -1;
    std::vector<Session *> ss(n); std::vector<std::vector<uint8_t>> blobs(n); std::vector<char> ok(n, 0);
    for (size_t i = 0; i < n; ++i) ss[i] = &sessions[i]->s;
    static_assert(sizeof(bool) == sizeof(char), "ok flags");
    snapshot_sessions(n, ss.data(), blobs.data(), reinterpret_cast<bool *>(ok.data()), /*sizes_only=*/dsts == nullptr);
    int failed = 0;
    for (size_t i = 0; i < n; ++i) {
        sizes_out[i] = -1;
        if (ok[i] && (!dsts || (dsts[i] && caps[i] >= blobs[i].size()))) {
            if (dsts) memcpy(dsts[i], blobs[i].data(), blobs[i].size());
            sizes_out[i] = (int64_t)blobs[i].size();
        } else ++failed;
    }
    return failed;
}

int64_t aprilx_session_snapshot(AprilASRSession session, void *dst, size_t cap)
{
    if (!session) return -1;
    int64_t size = -1;
    void *d = dst;
    aprilx_snapshot_many(1, &session, dst ? &d : nullptr, &cap, &size);
    return size;
}

int aprilx_restore_many(size_t n, AprilASRSession *sessions, const void *const *blobs, const size_t *sizes, int *status_out)
{
    if (!sessions || !blobs || !sizes || !status_out) return -1;
    for (size_t i = 0; i < n; ++i) if (!sessions[i]) return -1;
    std::vector<Session *> ss(n); std::vector<std::string> errs(n);
    for (size_t i = 0; i < n; ++i) ss[i] = &sessions[i]->s;
    restore_sessions(n, ss.data(), blobs, sizes, status_out, errs.data());
    int failed = 0;
    for (size_t i = 0; i < n; ++i) if (status_out[i]) { ++failed; LOGW("aprilx_restore_many: session %zu refused: %s", i, errs[i].c_str()); }
    return failed;
}

int aprilx_session_restore(AprilASRSession session, const void *blob, size_t size, char *err, size_t err_cap)
{
    if (err && err_cap) err[0] = 0;
    if (!session) return -1;
    Session *s = &session->s;
    int status = -1; std::string why;
    restore_sessions(1, &s, &blob, &size, &status, &why);
    if (status && err && err_cap) { strncpy(err, why.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    return status ? -1 : 0;
}

int aprilx_snapshot_info(const void *blob, size_t size, AprilxSnapshotInfo *out)
{
    snap::View v;
    if (!out || !snap::parse(blob, size, &v)) return -1;
    memcpy(out, v.blk[snap::B_INFO], sizeof *out);
    if (out->size != sizeof *out || out->version != snap::kVersion || out->blob_size != (uint64_t)size) return -1;
    return 0;
}

int aprilx_model_snapshot_stats(AprilASRModel model, int device_index, uint64_t *gathers, uint64_t *scatters, double *gather_ms, double *scatter_ms)
{
    if (!model || device_index < 0 || device_index >= (int)model->m.engines.size() || !gathers || !scatters) return -1;
    const Engine *e = model->m.engines[(size_t)device_index];
    e->snapshot_counts(gathers, scatters);
    if (gather_ms) *gather_ms = e->timing(Engine::T_SNAP_GATHER).ms;
    if (scatter_ms) *scatter_ms = e->timing(Engine::T_SNAP_SCATTER).ms;
    return 0;
}

}  // extern "C"
