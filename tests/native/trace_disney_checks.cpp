// trace_disney_checks.cpp -- the argument checks of rls_trace_disney_emit (librls_trace.so), driven with dummy planes and
// no GPU (tests/test_trace_abi.py builds and runs it), in the style of argument_checks.cpp.
//
// Every case starts from a set of arguments that passes every check, breaks one or two of them (or none) and records what
// the call returns.  A call whose arguments pass reaches the launch, and with no device there its hipSetDevice fails: status
// RLS_ERR_HIP.  That is only safe while no device is visible: on a GPU the dummy planes would reach a kernel.  The driver
// refuses to run if HIP reports a device.
//
// Output: one tab-separated line per case and math mode:
//   case  fast  status  expected-status  expected-text  message
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <functional>
#include <string>
#include <vector>

#include "../../rlshaders_amd/csrc/rls_internal.hpp"
#include "../../include/rlshaders_amd_trace.h"

namespace {

float g_plane[64];                      // the stand-in for every device plane: never dereferenced without a device
uint32_t g_ids[4];
int64_t g_offsets[4];
float *const D = g_plane;

struct World {
    rls_context context;
    rls_context *ctx;
    int64_t n;
    int lobe;
    int spp_n;
    rls_disney_closure dc;
    const rls_disney_closure *dp;
    rls_ray_queue q;
    const rls_ray_queue *qp;
    float *valid;

    explicit World(int fast)
    {
        context = {};
        context.device = 0;
        context.compute_units = 256;
        context.blocks_per_cu = 64;
        context.fast = fast;
        ctx = &context;
        n = 1000;
        lobe = RLS_RAY_DIFFUSE;
        spp_n = 4;
        dc = {};
        dc.wo = { D, D, D }; dc.N = { D, D, D }; dc.T = { D, D, D };
        dc.base_color = { D, D, D, 0.0f, 0.0f, 0.0f };
        dc.roughness = { D, 0.0f };
        dc.materials = { g_ids, 4 };
        dp = &dc;
        q = {};
        q.capacity = (int64_t)1 << 40;
        q.offsets = g_offsets;
        q.dir = { D, D, D };
        q.weight = { D, D, D };
        q.scratch = g_plane;
        q.scratch_bytes = SIZE_MAX;
        qp = &q;
        valid = D;
    }
};

struct Case {
    std::string what;
    std::function<void(World &)> brk;
    int status;
    std::string text;                   // for RLS_ERR_INVALID_ARGUMENT: "emit: <text>"
};

const int BAD = RLS_ERR_INVALID_ARGUMENT, HIP = RLS_ERR_HIP;
const char *const LOBE = "lobe must be RLS_RAY_DIFFUSE or RLS_RAY_GLOSSY", *const SPP = "spp_n must be in [1, 16]",
                  *const QUEUE = "queue or queue.offsets is NULL", *const FRAME = "wo/N/T plane is NULL",
                  *const WEIGHT = "queue.weight plane is NULL",
                  *const SCRATCH = "queue.scratch is NULL or smaller than rls_trace_scratch_bytes";

std::vector<Case> cases()
{
    return {
        { "valid, diffuse", [](World &) {}, HIP, "" },
        { "valid, glossy", [](World &w) { w.lobe = RLS_RAY_GLOSSY; }, HIP, "" },
        { "ctx NULL", [](World &w) { w.ctx = nullptr; }, BAD, "ctx is NULL" },
        { "n < 0", [](World &w) { w.n = -1; }, BAD, "n < 0" },
        { "n = 2^32", [](World &w) { w.n = (int64_t)1 << 32; }, BAD, "n > 2^32 - 1 (the queue's point index is 32-bit)" },
        { "spp_n 0", [](World &w) { w.spp_n = 0; }, BAD, SPP },
        { "spp_n 17", [](World &w) { w.spp_n = 17; }, BAD, SPP },
        { "spp_n 17, lobe 0", [](World &w) { w.spp_n = 17; w.lobe = 0; }, BAD, SPP },
        { "lobe 0", [](World &w) { w.lobe = 0; }, BAD, LOBE },
        { "lobe diffuse | glossy", [](World &w) { w.lobe = RLS_RAY_DIFFUSE | RLS_RAY_GLOSSY; }, BAD, LOBE },
        { "lobe 0, queue NULL", [](World &w) { w.lobe = 0; w.qp = nullptr; }, BAD, LOBE },
        { "queue NULL", [](World &w) { w.qp = nullptr; }, BAD, QUEUE },
        { "queue.offsets NULL", [](World &w) { w.q.offsets = nullptr; }, BAD, QUEUE },
        // an empty batch still writes offsets[0] = 0: a launch
        { "n == 0", [](World &w) { w.n = 0; }, HIP, "" },
        { "n == 0, spp_n 0", [](World &w) { w.n = 0; w.spp_n = 0; }, BAD, SPP },
        { "n == 0, lobe 0", [](World &w) { w.n = 0; w.lobe = 0; }, BAD, LOBE },
        { "n == 0, queue NULL", [](World &w) { w.n = 0; w.qp = nullptr; }, BAD, QUEUE },
        { "n == 0, closure NULL", [](World &w) { w.n = 0; w.dp = nullptr; }, HIP, "" },
        { "closure NULL", [](World &w) { w.dp = nullptr; }, BAD, "closure is NULL" },
        { "wo NULL", [](World &w) { w.dc.wo.y = nullptr; }, BAD, FRAME },
        { "N NULL", [](World &w) { w.dc.N.z = nullptr; }, BAD, FRAME },
        { "T NULL", [](World &w) { w.dc.T.x = nullptr; }, BAD, FRAME },
        { "base_color mixed NULL", [](World &w) { w.dc.base_color.b = nullptr; }, BAD,
          "base_color planes must be all set or all NULL" },
        { "materials.count 0", [](World &w) { w.dc.materials.count = 0; }, BAD, "materials.id is set but materials.count is 0" },
        { "closure NULL, queue.dir NULL", [](World &w) { w.dp = nullptr; w.q.dir.x = nullptr; }, BAD, "closure is NULL" },
        { "queue.dir NULL", [](World &w) { w.q.dir.y = nullptr; }, BAD, "queue.dir plane is NULL" },
        { "queue.weight.r NULL", [](World &w) { w.q.weight.r = nullptr; }, BAD, WEIGHT },
        { "queue.weight.g NULL", [](World &w) { w.q.weight.g = nullptr; }, BAD, WEIGHT },
        { "queue.weight.b NULL, glossy", [](World &w) { w.q.weight.b = nullptr; w.lobe = RLS_RAY_GLOSSY; }, BAD, WEIGHT },
        { "queue.capacity short", [](World &w) { w.q.capacity = w.n * w.spp_n * w.spp_n - 1; }, BAD,
          "queue.capacity < n * spp_n^2" },
        { "queue.scratch NULL", [](World &w) { w.q.scratch = nullptr; }, BAD, SCRATCH },
        { "queue.scratch short", [](World &w) { w.q.scratch_bytes = 4096; }, BAD, SCRATCH },
        { "valid_count NULL", [](World &w) { w.valid = nullptr; }, HIP, "" },
        { "point, sample NULL", [](World &w) { w.q.point = nullptr; w.q.sample = nullptr; }, HIP, "" },
        { "no materials", [](World &w) { w.dc.materials = {}; }, HIP, "" },
    };
}

} // namespace

int main()
{
    int devices = 0;
    if (hipGetDeviceCount(&devices) == hipSuccess && devices > 0) {
        fprintf(stderr, "trace_disney_checks: %d HIP device(s) visible; this driver hands dummy planes to the entry point "
                        "and runs only where no device is\n", devices);
        return 2;
    }
    (void)hipGetLastError();
    const std::vector<Case> all = cases();
    for (int fast = 0; fast < 2; fast++) {
        for (const Case &c : all) {
            World w(fast);
            c.brk(w);
            const rls_status st = rls_trace_disney_emit(w.ctx, w.n, w.dp, w.lobe, w.spp_n, 7u, 0u, w.qp, w.valid);
            const char *msg = st == RLS_OK ? "" : rls_last_error();
            printf("%s\t%d\t%d\t%d\t%s\t%s\n", c.what.c_str(), fast, st, c.status, c.text.c_str(), msg);
        }
    }
    return 0;
}
