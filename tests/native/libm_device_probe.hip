// libm_device_probe.hip -- the DEVICE-only instruction sequences of csrc/rls_libm.hpp, one call per lane, for
// tests/test_gpu_libm_primitives.py.  Compiled for the host those sequences are `1.0f / x`, `a / b`, sqrtf, so no host
// build of the header exercises them, and rls_libm_eval exposes none of them.  Test infrastructure: built with the
// product's own flags (rlshaders_amd/build.py, build_libm_probe) into tests/native/build/librls_libm_probe.so; the
// product libraries gain no entry point.  ratio_to_one_minus / slope_y_ratio come from csrc/rls_device.hpp at RLS_FAST=0,
// the way csrc/alternates.hip sees them.
#ifndef RLS_FAST
#define RLS_FAST 0
#endif
#if RLS_FAST
#error "the probe is for the EXACT forms"
#endif
#include "rls_device.hpp"

namespace {

// function ids: tests/libm_probe_util.py (PROBE_FN) names the same numbers
enum {
    P_RCP_W = 0, P_RCP = 1, P_RCP_HI = 2, P_DIV_M = 3,
    P_DIVC_3 = 4, P_DIVC_03333 = 5, P_DIVC_1M06666 = 6, P_DIVC_06666M03333 = 7,
    P_DIVCW_3 = 8, P_DIVCW_03333 = 9, P_DIVCW_1M06666 = 10, P_DIVCW_06666M03333 = 11,
    P_DIV_Y = 12, P_SQRT_1P = 13, P_SQRT_1M = 14, P_TWO_OVER = 15, P_EXP_IN_RANGE = 16, P_EXP_IN_RANGE_3 = 17,
    P_RATIO_TO_ONE_MINUS = 18, P_SLOPE_Y_RATIO = 19, P_COUNT = 20
};

__global__ __launch_bounds__(RLS_BLOCK) void probe_kernel(int fn, int64_t n, const float *a, const float *b, const float *c,
                                                          float *out)
{
    using namespace rlsd;
    stage_libm_tables();                                   // every lane of the workgroup: it ends in a barrier
    const int64_t i = (int64_t)blockIdx.x * RLS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float x = a[i];
    const float y = b ? b[i] : 0.0f;
    const float z = c ? c[i] : 0.0f;
    float r;
    switch (fn) {                                          // a kernel argument: uniform
    case P_RCP_W: r = rlm::rcp32_w(x); break;
    case P_RCP: r = rlm::rcp32(x); break;
    case P_RCP_HI: r = rlm::rcp32_hi(x); break;
    case P_DIV_M: r = rlm::div32_m(x, y); break;
    // the constants as the kernels spell them (rls_device.hpp: NDProfile's q / 3 and the three lobe ranges of rx)
    case P_DIVC_3: r = R_DIVC(x, 3.0f); break;
    case P_DIVC_03333: r = R_DIVC(x, 0.3333f - 0.0f); break;
    case P_DIVC_1M06666: r = R_DIVC(x, 1.0f - 0.6666f); break;
    case P_DIVC_06666M03333: r = R_DIVC(x, 0.6666f - 0.3333f); break;
    case P_DIVCW_3: r = R_DIVCW(x, 3.0f); break;
    case P_DIVCW_03333: r = R_DIVCW(x, 0.3333f - 0.0f); break;
    case P_DIVCW_1M06666: r = R_DIVCW(x, 1.0f - 0.6666f); break;
    case P_DIVCW_06666M03333: r = R_DIVCW(x, 0.6666f - 0.3333f); break;
    case P_DIV_Y: r = rlm::div32_y(x, y, rlm::rcp32_w(y)); break;
    case P_SQRT_1P: r = R_SQRT1P(x); break;
    case P_SQRT_1M: r = R_SQRT1M(x); break;
    case P_TWO_OVER: r = R_TWO_OVER(1.0f + R_SQRT1P(x)); break;
    case P_EXP_IN_RANGE: r = R_EXP_IN_RANGE(x); break;
    case P_EXP_IN_RANGE_3: r = rlm::exp32_in_range_3(x, y, z) ? 1.0f : 0.0f; break;
    case P_RATIO_TO_ONE_MINUS: r = ratio_to_one_minus(x); break;
    case P_SLOPE_Y_RATIO: r = slope_y_ratio(x); break;
    default: r = 0.0f; break;
    }
    out[i] = r;
}

} // namespace

// -> 0, or the hipError_t of the launch; -1 for arguments the kernel must not see
extern "C" int rls_libm_probe(int fn, int64_t n, const float *a, const float *b, const float *c, float *out, void *stream)
{
    if (fn < 0 || fn >= P_COUNT || n < 0 || n > ((int64_t)1 << 30) || (n > 0 && (!a || !out))) return -1;
    const bool binary = fn == P_DIV_M || fn == P_DIV_Y || fn == P_EXP_IN_RANGE_3;
    if (n > 0 && binary && !b) return -1;
    if (n > 0 && fn == P_EXP_IN_RANGE_3 && !c) return -1;
    if (n == 0) return 0;
    const unsigned blocks = (unsigned)((n + RLS_BLOCK - 1) / RLS_BLOCK);
    hipLaunchKernelGGL(probe_kernel, dim3(blocks), dim3(RLS_BLOCK), 0, (hipStream_t)stream, fn, n, a, binary ? b : nullptr,
                       fn == P_EXP_IN_RANGE_3 ? c : nullptr, out);
    return (int)hipGetLastError();
}
