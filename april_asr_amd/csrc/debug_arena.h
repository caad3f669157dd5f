// Device allocations of one call of a single-launch test entry (gemm_debug_api.cc, conv_debug_api.cc).
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "common.h"

namespace aprilx {

// device allocations of one call, freed together; `bad` latches the first failing HIP call
struct Arena {
    const char *who;                                  // name of the entry, for the log
    std::vector<void *> ptrs;
    bool bad = false;
    explicit Arena(const char *w) : who(w) {}
    bool ok(hipError_t e) { if (e != hipSuccess) { if (!bad) LOGE("%s: HIP: %s", who, hipGetErrorString(e)); bad = true; } return !bad; }
    void *raw(size_t bytes, int fill)
    {
        void *p = nullptr;
        if (bad || !ok(hipMalloc(&p, bytes ? bytes : 4))) return nullptr;
        ptrs.push_back(p);
        ok(hipMemset(p, fill, bytes ? bytes : 4));
        return p;
    }
    // `bytes` of device memory: the first `have` from the host array, the rest zero
    void *upload(const void *host, size_t have, size_t bytes)
    {
        void *p = raw(bytes < have ? have : bytes, 0);
        if (p && have) ok(hipMemcpy(p, host, have, hipMemcpyHostToDevice));
        return p;
    }
    void download(void *host, const void *dev, size_t bytes) { if (host && dev && !bad) ok(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost)); }
    ~Arena() { for (void *p : ptrs) (void)hipFree(p); }
};

}  // namespace aprilx
