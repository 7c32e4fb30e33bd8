// rt_kernels_f64.hip — the FP64 render kernels (namespace rtd): the parity
// path.  Device math follows the reference's double arithmetic step for step
// (DESIGN.md §Numerics).
#include "rt_device.hpp"
#include "rt_kernels.hpp"
#include "rt_test.h"

// ------------------------------------------------------------- test hook
// div3 (rt_device.hpp) against the compiler's own division on the device:
// out_div3[3i+k] = div3(a[3i..3i+2], b[i])[k], out_plain[3i+k] = a[3i+k] / b[i].
namespace {
__global__ void k_test_div3(const double* a, const double* b, int n, double* o3, double* op) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rtd::D3 q = rtd::div3(a[3 * i], a[3 * i + 1], a[3 * i + 2], b[i]);
    o3[3 * i] = q.x;
    o3[3 * i + 1] = q.y;
    o3[3 * i + 2] = q.z;
    op[3 * i] = a[3 * i] / b[i];
    op[3 * i + 1] = a[3 * i + 1] / b[i];
    op[3 * i + 2] = a[3 * i + 2] / b[i];
}
// pow_spec (rt_device.hpp), the specular term's power, on caller-given (x, y):
// integer and other exponents may share a wave, as materials do in shade().
__global__ void k_test_pow_spec(const double* x, const double* y, int n, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = rtd::pow_spec(x[i], y[i]);
}
// spec_skips (rt_device.hpp) on shade()'s own reflection vector, next to the
// power the lane computes where it does not skip.
__global__ void k_test_spec_skip(const double* nn, const double* wi, const double* wo, const double* shin, int n,
                                 int* skip, double* plain) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rtd::V3 N = rtd::v3(nn[3 * i], nn[3 * i + 1], nn[3 * i + 2]);
    const rtd::V3 I = rtd::v3(wi[3 * i], wi[3 * i + 1], wi[3 * i + 2]);
    const rtd::V3 O = rtd::v3(wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]);
    const rtd::V3 rv = rtd::v3(2.0 * rtd::dot3(N, I) * N.x - I.x, 2.0 * rtd::dot3(N, I) * N.y - I.y,
                               2.0 * rtd::dot3(N, I) * N.z - I.z);
    const double s = rtd::dot3(rv, rv);
    skip[i] = rtd::spec_skips(rv, s, O, shin[i]) ? 1 : 0;
    plain[i] = rtd::pow_spec(rtd::cmax(0.0, rtd::dot3(rtd::normalized(rv, s), O)), shin[i]);
}
// norm3 / normalized (rt_device.hpp) next to __builtin_sqrt and `/` on the
// same vectors; fast[i]: lane i's wave took the fused path.
__global__ void k_test_norm3(const double* v, int n, double* oL, double* oq, double* pL, double* pq, int* fast,
                             double* onrm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rtd::V3 a = rtd::v3(v[3 * i], v[3 * i + 1], v[3 * i + 2]);
    const rtd::N3 r = rtd::norm3(a);
    oL[i] = r.L;
    oq[3 * i] = r.q.x;
    oq[3 * i + 1] = r.q.y;
    oq[3 * i + 2] = r.q.z;
    fast[i] = r.fast ? 1 : 0;
    const double L = __builtin_sqrt(rtd::dot3(a, a));
    pL[i] = L;
    pq[3 * i] = a.x / L;
    pq[3 * i + 1] = a.y / L;
    pq[3 * i + 2] = a.z / L;
    if (onrm) {
        const rtd::V3 u = rtd::normalized(a);
        onrm[3 * i] = u.x;
        onrm[3 * i + 1] = u.y;
        onrm[3 * i + 2] = u.z;
    }
}
}  // namespace

static int test_norm3(const double* v_host, int n, double* L_host, double* q_host, double* plainL_host,
                      double* plainq_host, int* fast_host, double* nrm_host) {
    if (n <= 0 || !v_host || !L_host || !q_host || !plainL_host || !plainq_host || !fast_host) return RT_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RT_ERR_NO_DEVICE;
    const size_t n1 = (size_t)n * sizeof(double), n3 = 3 * n1, nf = (size_t)n * sizeof(int);
    double *v = nullptr, *oL = nullptr, *oq = nullptr, *pL = nullptr, *pq = nullptr, *on = nullptr;
    int* fast = nullptr;
    int rc = RT_OK;
    if (hipMalloc(&v, n3) != hipSuccess || hipMalloc(&oL, n1) != hipSuccess || hipMalloc(&oq, n3) != hipSuccess ||
        hipMalloc(&pL, n1) != hipSuccess || hipMalloc(&pq, n3) != hipSuccess || hipMalloc(&fast, nf) != hipSuccess ||
        (nrm_host && hipMalloc(&on, n3) != hipSuccess))
        rc = RT_ERR_HIP;
    if (rc == RT_OK && hipMemcpy(v, v_host, n3, hipMemcpyHostToDevice) != hipSuccess) rc = RT_ERR_HIP;
    if (rc == RT_OK) {
        hipLaunchKernelGGL(k_test_norm3, dim3((n + 255) / 256), dim3(256), 0, nullptr, v, n, oL, oq, pL, pq, fast, on);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(L_host, oL, n1, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(q_host, oq, n3, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(plainL_host, pL, n1, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(plainq_host, pq, n3, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(fast_host, fast, nf, hipMemcpyDeviceToHost) != hipSuccess ||
            (nrm_host && hipMemcpy(nrm_host, on, n3, hipMemcpyDeviceToHost) != hipSuccess))
            rc = RT_ERR_HIP;
    }
    if (v) (void)hipFree(v);
    if (oL) (void)hipFree(oL);
    if (oq) (void)hipFree(oq);
    if (pL) (void)hipFree(pL);
    if (pq) (void)hipFree(pq);
    if (fast) (void)hipFree(fast);
    if (on) (void)hipFree(on);
    return rc;
}

extern "C" int rt_test_norm3(const double* v_host, int n, double* L_host, double* q_host, double* plainL_host,
                             double* plainq_host, int* fast_host) {
    return test_norm3(v_host, n, L_host, q_host, plainL_host, plainq_host, fast_host, nullptr);
}

extern "C" int rt_test_normalized(const double* v_host, int n, double* out_host) {
    if (n <= 0 || !v_host || !out_host) return RT_ERR_INVALID_ARG;
    // (the other outputs of the kernel go to scratch arrays)
    double* tmp = new double[(size_t)n * 8];
    int* fast = new int[n];
    const int rc = test_norm3(v_host, n, tmp, tmp + n, tmp + 4 * (size_t)n, tmp + 5 * (size_t)n, fast, out_host);
    delete[] tmp;
    delete[] fast;
    return rc;
}

extern "C" int rt_test_pow_spec(const double* x_host, const double* y_host, int n, double* out_host) {
    if (n <= 0 || !x_host || !y_host || !out_host) return RT_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RT_ERR_NO_DEVICE;
    double *x = nullptr, *y = nullptr, *o = nullptr;
    const size_t nb = (size_t)n * sizeof(double);
    int rc = RT_OK;
    if (hipMalloc(&x, nb) != hipSuccess || hipMalloc(&y, nb) != hipSuccess || hipMalloc(&o, nb) != hipSuccess)
        rc = RT_ERR_HIP;
    if (rc == RT_OK && (hipMemcpy(x, x_host, nb, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(y, y_host, nb, hipMemcpyHostToDevice) != hipSuccess))
        rc = RT_ERR_HIP;
    if (rc == RT_OK) {
        hipLaunchKernelGGL(k_test_pow_spec, dim3((n + 255) / 256), dim3(256), 0, nullptr, x, y, n, o);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out_host, o, nb, hipMemcpyDeviceToHost) != hipSuccess)
            rc = RT_ERR_HIP;
    }
    if (x) (void)hipFree(x);
    if (y) (void)hipFree(y);
    if (o) (void)hipFree(o);
    return rc;
}

extern "C" int rt_test_spec_skip(const double* n_host, const double* wi_host, const double* wo_host,
                                 const double* shin_host, int n, int* skip_host, double* plain_host) {
    if (n <= 0 || !n_host || !wi_host || !wo_host || !shin_host || !skip_host || !plain_host) return RT_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RT_ERR_NO_DEVICE;
    const size_t n1 = (size_t)n * sizeof(double), n3 = 3 * n1, nf = (size_t)n * sizeof(int);
    double *nn = nullptr, *wi = nullptr, *wo = nullptr, *sh = nullptr, *pl = nullptr;
    int* sk = nullptr;
    int rc = RT_OK;
    if (hipMalloc(&nn, n3) != hipSuccess || hipMalloc(&wi, n3) != hipSuccess || hipMalloc(&wo, n3) != hipSuccess ||
        hipMalloc(&sh, n1) != hipSuccess || hipMalloc(&pl, n1) != hipSuccess || hipMalloc(&sk, nf) != hipSuccess)
        rc = RT_ERR_HIP;
    if (rc == RT_OK && (hipMemcpy(nn, n_host, n3, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(wi, wi_host, n3, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(wo, wo_host, n3, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(sh, shin_host, n1, hipMemcpyHostToDevice) != hipSuccess))
        rc = RT_ERR_HIP;
    if (rc == RT_OK) {
        hipLaunchKernelGGL(k_test_spec_skip, dim3((n + 255) / 256), dim3(256), 0, nullptr, nn, wi, wo, sh, n, sk, pl);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(skip_host, sk, nf, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(plain_host, pl, n1, hipMemcpyDeviceToHost) != hipSuccess)
            rc = RT_ERR_HIP;
    }
    if (nn) (void)hipFree(nn);
    if (wi) (void)hipFree(wi);
    if (wo) (void)hipFree(wo);
    if (sh) (void)hipFree(sh);
    if (pl) (void)hipFree(pl);
    if (sk) (void)hipFree(sk);
    return rc;
}

extern "C" int rt_test_div3(const double* a_host, const double* b_host, int n, double* div3_host, double* plain_host) {
    if (n <= 0 || !a_host || !b_host || !div3_host || !plain_host) return RT_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RT_ERR_NO_DEVICE;
    double *a = nullptr, *b = nullptr, *o3 = nullptr, *op = nullptr;
    const size_t n3 = (size_t)n * 3 * sizeof(double);
    int rc = RT_OK;
    if (hipMalloc(&a, n3) != hipSuccess || hipMalloc(&b, (size_t)n * sizeof(double)) != hipSuccess ||
        hipMalloc(&o3, n3) != hipSuccess || hipMalloc(&op, n3) != hipSuccess)
        rc = RT_ERR_HIP;
    if (rc == RT_OK && (hipMemcpy(a, a_host, n3, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(b, b_host, (size_t)n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess))
        rc = RT_ERR_HIP;
    if (rc == RT_OK) {
        hipLaunchKernelGGL(k_test_div3, dim3((n + 255) / 256), dim3(256), 0, nullptr, a, b, n, o3, op);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(div3_host, o3, n3, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(plain_host, op, n3, hipMemcpyDeviceToHost) != hipSuccess)
            rc = RT_ERR_HIP;
    }
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    if (o3) (void)hipFree(o3);
    if (op) (void)hipFree(op);
    return rc;
}
