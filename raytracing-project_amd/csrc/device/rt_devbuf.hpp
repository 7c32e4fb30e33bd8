// rt_devbuf.hpp — the growable device buffer and the HIP error macro shared
// by the host sides of librtamd (rt_workspace.hpp, rt_render.hip, rt_dist.hip, rt_test_hooks.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "rt.h"
#include "rt_internal.hpp"

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            rtamd::set_last_error(std::string(#expr) + " failed: " + hipGetErrorString(e_));     \
            return RT_ERR_HIP;                                                                   \
        }                                                                                        \
    } while (0)

namespace rtamd {

// Growable device buffer.  SLACK: a growth allocates bytes + bytes / SLACK +
// 256 (the render workspace 8, the distributed frame's buffers 16).
template <int SLACK>
struct DevBufT {
    void* p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= n) return hipSuccess;
        release();
        const size_t want = bytes + bytes / SLACK + 256;
        SetupTimer tm(kSetupAlloc);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) n = want;
        return e;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

}  // namespace rtamd
