// rt_render.hip — librtamd's four utility kernels with their launchers, and the
// device / stream / memcpy part of the C-ABI.  The frame path is rt_frame.hip,
// the batched entry points rt_batch.hip, the workspace they run on
// rt_workspace.hip; the rt_test_* hooks live in rt_test_hooks.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "mt_poly.hpp"
#include "rt_workspace.hpp"

namespace {

__global__ void k_scatter_rows(const double* __restrict__ src, const int32_t* __restrict__ rows, int n_rows, int W,
                               double* __restrict__ dst) {
    const size_t row_len = (size_t)W * 3;
    const size_t total = row_len * n_rows;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / row_len, k = i - r * row_len;
        const int32_t d = rows[r];
        if (d >= 0) dst[(size_t)d * row_len + k] = src[i];
    }
}

__global__ void k_to_rgb8(const double* __restrict__ fb, size_t n, uint8_t* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double v = fb[i];
        double c = (v < 1.0) ? v : 1.0;   // std::min(1.0, v)
        c = (0.0 < c) ? c : 0.0;          // std::max(0.0, .)
        out[i] = (uint8_t)(int)round(c * 255.0);   // round half away from zero (core.h:316)
    }
}

// The frame's op counters: kCounterSlots x kCounterWords partial sums reduced
// on the device and stored straight into page-locked host memory, so that
// rt_frame_end reads 144 B after one event instead of copying 72 KiB through
// the runtime's pageable staging (which waited ~115 us after the last kernel
// before the copy even started: profiles/r04t_api_timeline.txt).
__global__ void __launch_bounds__(64) k_reduce_counters(unsigned long long* __restrict__ slots,
                                                        unsigned long long* __restrict__ out,
                                                        const unsigned int* __restrict__ gtime, int wpg) {
    // block k < kCounterWords sums word k over the slots (8 independent loads
    // per lane); block kCounterWords + g sums paper-mode list group g's wave
    // times (end - start, mod 2^32) over its wpg waves
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= rtamd::kCounterWords) {
        const size_t g = k - rtamd::kCounterWords;
        unsigned v = 0;
        for (int xt = lane; xt < wpg; xt += 64) {
            const unsigned* t = gtime + 2 * (g * wpg + xt);
            v += t[1] - t[0];
        }
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) reinterpret_cast<unsigned int*>(out + rtamd::kCounterWords)[g] = v;
        return;
    }
    // (and leaves the slots zero for the next frame: FrameBuffers::counters_zero)
    unsigned long long v = 0;
#pragma unroll
    for (int sl = lane; sl < rtamd::kCounterSlots; sl += 64) {
        unsigned long long* w = slots + (size_t)sl * rtamd::kCounterWords + k;
        v += *w;
        *w = 0ull;
    }
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) out[k] = v;
}

// dst <- page-locked host src, 16-byte words (+ a byte tail), read by the GPU over PCIe
__global__ void k_host_copy(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16, int tail) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
    if (blockIdx.x == 0 && (int)threadIdx.x < tail)
        reinterpret_cast<unsigned char*>(dst + n16)[threadIdx.x] = reinterpret_cast<const unsigned char*>(src + n16)[threadIdx.x];
}

// blocks of 256 threads for a grid-stride loop over n elements
unsigned stride_blocks(size_t n, size_t most) { return (unsigned)std::max<size_t>(1, std::min<size_t>(most, (n + 255) / 256)); }

}  // namespace

// ------------------------------------------------------------- launchers
hipError_t rtw::launch_reduce_counters(hipStream_t st, unsigned long long* slots, unsigned long long* out,
                                       const unsigned int* gtime, int wpg, int n_groups) {
    hipLaunchKernelGGL(k_reduce_counters, dim3(rtamd::kCounterWords + n_groups), dim3(64), 0, st, slots, out, gtime, wpg);
    return hipGetLastError();
}

hipError_t rtamd::host_copy_async(void* dst, const void* src, size_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15)
        return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st);
    const size_t n16 = n / 16;
    const int tail = (int)(n - n16 * 16);
    hipLaunchKernelGGL(k_host_copy, dim3(stride_blocks(n16, 1024)), dim3(256), 0, st, static_cast<const uint4*>(src),
                       static_cast<uint4*>(dst), n16, tail);
    return hipGetLastError();
}

extern "C" int rt_scatter_rows_device(const double* src_dev, const int32_t* rows_dev, int n_rows, int W,
                                      double* fb_dev, void* hip_stream) {
    if (n_rows <= 0) return RT_OK;
    if (!src_dev || !rows_dev || !fb_dev || W <= 0) { rtamd::set_last_error("rt_scatter_rows_device: bad args"); return RT_ERR_INVALID_ARG; }
    const size_t total = (size_t)W * 3 * n_rows;
    hipLaunchKernelGGL(k_scatter_rows, dim3(stride_blocks(total, 8192)), dim3(256), 0, (hipStream_t)hip_stream, src_dev,
                       rows_dev, n_rows, W, fb_dev);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

extern "C" int rt_framebuffer_to_rgb8_device(const double* fb_dev, size_t n_pixels, uint8_t* rgb8_dev,
                                             void* hip_stream) {
    if (!n_pixels) return RT_OK;
    if (!fb_dev || !rgb8_dev) { rtamd::set_last_error("rt_framebuffer_to_rgb8_device: NULL"); return RT_ERR_INVALID_ARG; }
    const size_t n = n_pixels * 3;
    hipLaunchKernelGGL(k_to_rgb8, dim3(stride_blocks(n, 8192)), dim3(256), 0, (hipStream_t)hip_stream, fb_dev, n, rgb8_dev);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ------------------------------------------------------------------ C-ABI
extern "C" int rt_warmup(int what) {
    if (what & ~(RT_WARM_HOST | RT_WARM_DEVICE)) {
        rtamd::set_last_error("rt_warmup: unknown bits");
        return RT_ERR_INVALID_ARG;
    }
    if (what & RT_WARM_HOST) {
        try {
            rtamd::mt_prefetch_host_taps();
        } catch (const std::exception& e) {
            rtamd::set_last_error(std::string("rt_warmup: ") + e.what());
            return RT_ERR_PROCESSING;
        }
    }
    if (what & RT_WARM_DEVICE) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
            rtamd::set_last_error("rt_warmup: no HIP device available");
            return RT_ERR_NO_DEVICE;
        }
        // the FP64 render kernels' code object (one per fat binary and
        // device, loaded at its first use; hipFuncGetAttributes loads it)
        hipFuncAttributes a{};
        rtamd::KernelVariant lean;   // (k_std_lean<false, 1, false>)
        lean.wv = 1;
        HIP_TRY(hipFuncGetAttributes(&a, rtamd::trace_kernel(lean, false).fn));
    }
    return RT_OK;
}

extern "C" int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int rt_set_device(int device) {
    HIP_TRY(hipSetDevice(device));
    return RT_OK;
}

extern "C" int rt_device_alloc(size_t bytes, void** dev_out) {
    if (!dev_out) { rtamd::set_last_error("rt_device_alloc: NULL"); return RT_ERR_INVALID_ARG; }
    *dev_out = nullptr;
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes ? bytes : 1));
    const hipError_t e = hipMemset(p, 0, bytes ? bytes : 1);
    if (e != hipSuccess) {
        (void)hipFree(p);
        rtamd::set_last_error(std::string("rt_device_alloc: hipMemset failed: ") + hipGetErrorString(e));
        return RT_ERR_HIP;
    }
    *dev_out = p;
    return RT_OK;
}

extern "C" int rt_device_free(void* dev) {
    if (dev) HIP_TRY(hipFree(dev));
    return RT_OK;
}

extern "C" int rt_memcpy_h2d(void* dev, const void* host, size_t bytes) {
    if (!bytes) return RT_OK;
    if (!dev || !host) { rtamd::set_last_error("rt_memcpy_h2d: NULL"); return RT_ERR_INVALID_ARG; }
    HIP_TRY(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice));
    return RT_OK;
}

extern "C" int rt_memcpy_d2h(void* host, const void* dev, size_t bytes) {
    if (!bytes) return RT_OK;
    if (!dev || !host) { rtamd::set_last_error("rt_memcpy_d2h: NULL"); return RT_ERR_INVALID_ARG; }
    HIP_TRY(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_device_synchronize(void) {
    HIP_TRY(hipDeviceSynchronize());
    return RT_OK;
}

extern "C" int rt_stream_create(void** stream_out) {
    if (!stream_out) { rtamd::set_last_error("rt_stream_create: NULL"); return RT_ERR_INVALID_ARG; }
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *stream_out = st;
    return RT_OK;
}

extern "C" int rt_stream_destroy(void* stream) {
    if (stream) HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return RT_OK;
}

extern "C" int rt_host_register(void* host, size_t bytes) {
    if (!host || !bytes) { rtamd::set_last_error("rt_host_register: NULL or empty"); return RT_ERR_INVALID_ARG; }
    HIP_TRY(hipHostRegister(host, bytes, hipHostRegisterDefault));
    return RT_OK;
}

extern "C" int rt_host_unregister(void* host) {
    if (!host) { rtamd::set_last_error("rt_host_unregister: NULL"); return RT_ERR_INVALID_ARG; }
    HIP_TRY(hipHostUnregister(host));
    return RT_OK;
}
