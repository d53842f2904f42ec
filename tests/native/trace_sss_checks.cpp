// trace_sss_checks.cpp -- the argument checks of rls_trace_sss_probe_emit and rls_trace_sss_scatter_resolve
// (librls_trace.so), driven with dummy planes and no GPU (tests/test_trace_abi.py builds and runs it), in the style of
// trace_disney_checks.cpp.
//
// Every case starts from a set of arguments that passes every check, breaks one or two of them (or none) and records what
// the call returns.  A call whose arguments pass reaches the launch, and with no device there its hipSetDevice fails: status
// RLS_ERR_HIP.  That is only safe while no device is visible: on a GPU the dummy planes would reach a kernel.  The driver
// refuses to run if HIP reports a device.
//
// Output: one tab-separated line per case and math mode:
//   verb  case  fast  status  expected-status  expected-text  message
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
uint8_t g_bytes[64];
int64_t g_offsets[4];
float *const D = g_plane;

struct World {
    rls_context context;
    rls_context *ctx;
    int64_t n;
    int spp_n;
    rls_sss_closure sc;
    const rls_sss_closure *cp;
    rls_cvec3 P;
    rls_probe_queue q;
    const rls_probe_queue *qp;
    rls_probe_hits h;
    const rls_probe_hits *hp;
    int cavity, literal;
    rls_rgb result;
    float *depth;

    explicit World(int fast)
    {
        context = {};
        context.device = 0;
        context.compute_units = 256;
        context.blocks_per_cu = 64;
        context.fast = fast;
        ctx = &context;
        n = 1000;
        spp_n = 4;
        sc = {};
        sc.sss_color = { D, D, D, 0.0f, 0.0f, 0.0f };
        sc.sss_dist_multiplier = { nullptr, 1.0f };
        for (int k = 0; k < 3; k++) sc.sss_scatter_dist[k] = { D, 0.0f };
        sc.N = { D, D, D };
        sc.T = { D, D, D };
        sc.has_dPdu = 1;
        sc.materials = { g_ids, 4 };
        cp = &sc;
        P = { D, D, D };
        q = {};
        q.capacity = (int64_t)1 << 40;
        q.offsets = g_offsets;
        q.origin = { D, D, D };
        q.dir = { D, D, D };
        q.maxdist = D;
        q.point = g_ids;
        q.sample = g_bytes;
        qp = &q;
        h = {};
        h.max_hits = RLS_MAX_PROBE_HITS;
        h.stride = (int64_t)1 << 40;
        h.count = g_bytes;
        h.P = { D, D, D };
        h.N = { D, D, D };
        h.irradiance = { D, D, D };
        hp = &h;
        cavity = 1;
        literal = 0;
        result = { D, D, D };
        depth = D;
    }
};

struct Case {
    std::string what;
    std::function<void(World &)> brk;
    int status;
    std::string text;                   // for RLS_ERR_INVALID_ARGUMENT: "<entry point>: <text>"
};

const int BAD = RLS_ERR_INVALID_ARGUMENT, HIP = RLS_ERR_HIP, OK = RLS_OK;
const char *const SPP = "spp_n must be in [1, 16]", *const QUEUE = "queue or queue.offsets is NULL",
                  *const FRAME = "N/T plane is NULL", *const PLANES = "queue.origin, queue.dir or queue.maxdist plane is NULL",
                  *const HITS = "hits.count, hits.P, hits.N or hits.irradiance plane is NULL",
                  *const MAXH = "hits.max_hits must be in [1, 12]";

// the checks both entry points share
std::vector<Case> common()
{
    return {
        { "ctx NULL", [](World &w) { w.ctx = nullptr; }, BAD, "ctx is NULL" },
        { "n < 0", [](World &w) { w.n = -1; }, BAD, "n < 0" },
        { "n = 2^32", [](World &w) { w.n = (int64_t)1 << 32; }, BAD, "n > 2^32 - 1 (the queue's point index is 32-bit)" },
        { "spp_n 0", [](World &w) { w.spp_n = 0; }, BAD, SPP },
        { "spp_n 17", [](World &w) { w.spp_n = 17; }, BAD, SPP },
        { "spp_n -3", [](World &w) { w.spp_n = -3; }, BAD, SPP },
        { "closure NULL", [](World &w) { w.cp = nullptr; }, BAD, "closure is NULL" },
        { "N NULL", [](World &w) { w.sc.N.z = nullptr; }, BAD, FRAME },
        { "T NULL", [](World &w) { w.sc.T.x = nullptr; }, BAD, FRAME },
        { "sss_color mixed NULL", [](World &w) { w.sc.sss_color.g = nullptr; }, BAD,
          "sss_color planes must be all set or all NULL" },
        { "materials.count 0", [](World &w) { w.sc.materials.count = 0; }, BAD, "materials.id is set but materials.count is 0" },
        { "P NULL", [](World &w) { w.P.y = nullptr; }, BAD, "P plane is NULL" },
        { "queue.capacity short", [](World &w) { w.q.capacity = w.n * w.spp_n * w.spp_n - 1; }, BAD,
          "queue.capacity < n * spp_n^2" },
        { "no materials", [](World &w) { w.sc.materials = {}; }, HIP, "" },
        { "uniform colour", [](World &w) { w.sc.sss_color = { nullptr, nullptr, nullptr, 0.5f, 0.5f, 0.5f }; }, HIP, "" },
        { "valid", [](World &) {}, HIP, "" },
        { "spp_n 16", [](World &w) { w.spp_n = 16; }, HIP, "" },
        { "capacity exact", [](World &w) { w.q.capacity = w.n * w.spp_n * w.spp_n; }, HIP, "" },
    };
}

std::vector<Case> emit_cases()
{
    std::vector<Case> c = common();
    std::vector<Case> more = {
        { "queue NULL", [](World &w) { w.qp = nullptr; }, BAD, QUEUE },
        { "queue.offsets NULL", [](World &w) { w.q.offsets = nullptr; }, BAD, QUEUE },
        { "queue.origin NULL", [](World &w) { w.q.origin.x = nullptr; }, BAD, PLANES },
        { "queue.dir NULL", [](World &w) { w.q.dir.z = nullptr; }, BAD, PLANES },
        { "queue.maxdist NULL", [](World &w) { w.q.maxdist = nullptr; }, BAD, PLANES },
        { "point, sample NULL", [](World &w) { w.q.point = nullptr; w.q.sample = nullptr; }, HIP, "" },
        { "spp_n 17, queue NULL", [](World &w) { w.spp_n = 17; w.qp = nullptr; }, BAD, SPP },
        // an empty batch still writes offsets[0] = 0: a launch
        { "n == 0", [](World &w) { w.n = 0; }, HIP, "" },
        { "n == 0, closure NULL", [](World &w) { w.n = 0; w.cp = nullptr; }, HIP, "" },
        { "n == 0, spp_n 0", [](World &w) { w.n = 0; w.spp_n = 0; }, BAD, SPP },
        { "n == 0, queue NULL", [](World &w) { w.n = 0; w.qp = nullptr; }, BAD, QUEUE },
    };
    c.insert(c.end(), more.begin(), more.end());
    return c;
}

std::vector<Case> resolve_cases()
{
    std::vector<Case> c = common();
    std::vector<Case> more = {
        { "queue NULL", [](World &w) { w.qp = nullptr; }, BAD, "queue is NULL" },
        { "queue.offsets NULL", [](World &w) { w.q.offsets = nullptr; w.q.origin = {}; }, HIP, "" },
        { "hits NULL", [](World &w) { w.hp = nullptr; }, BAD, "hits is NULL" },
        { "max_hits 0", [](World &w) { w.h.max_hits = 0; }, BAD, MAXH },
        { "max_hits 13", [](World &w) { w.h.max_hits = 13; }, BAD, MAXH },
        { "max_hits -1", [](World &w) { w.h.max_hits = -1; }, BAD, MAXH },
        { "max_hits 1", [](World &w) { w.h.max_hits = 1; }, HIP, "" },
        { "hits.stride short", [](World &w) { w.h.stride = w.n * w.spp_n * w.spp_n - 1; }, BAD, "hits.stride < n * spp_n^2" },
        { "hits.stride exact", [](World &w) { w.h.stride = w.n * w.spp_n * w.spp_n; }, HIP, "" },
        { "hits.count NULL", [](World &w) { w.h.count = nullptr; }, BAD, HITS },
        { "hits.P NULL", [](World &w) { w.h.P.x = nullptr; }, BAD, HITS },
        { "hits.N NULL", [](World &w) { w.h.N.y = nullptr; }, BAD, HITS },
        { "hits.irradiance NULL", [](World &w) { w.h.irradiance.b = nullptr; }, BAD, HITS },
        { "result NULL", [](World &w) { w.result.g = nullptr; }, BAD, "NULL output plane" },
        { "mean_depth NULL", [](World &w) { w.depth = nullptr; }, HIP, "" },
        { "flags", [](World &w) { w.cavity = 0; w.literal = 7; }, HIP, "" },
        { "spp_n 17, max_hits 0", [](World &w) { w.spp_n = 17; w.h.max_hits = 0; }, BAD, SPP },
        { "max_hits 0, closure NULL", [](World &w) { w.h.max_hits = 0; w.cp = nullptr; }, BAD, MAXH },
        // nothing to resolve: no launch
        { "n == 0", [](World &w) { w.n = 0; }, OK, "" },
        { "n == 0, closure NULL", [](World &w) { w.n = 0; w.cp = nullptr; }, OK, "" },
        { "n == 0, max_hits 13", [](World &w) { w.n = 0; w.h.max_hits = 13; }, BAD, MAXH },
        { "n == 0, spp_n 0", [](World &w) { w.n = 0; w.spp_n = 0; }, BAD, SPP },
    };
    c.insert(c.end(), more.begin(), more.end());
    return c;
}

} // namespace

int main()
{
    int devices = 0;
    if (hipGetDeviceCount(&devices) == hipSuccess && devices > 0) {
        fprintf(stderr, "trace_sss_checks: %d HIP device(s) visible; this driver hands dummy planes to the entry points "
                        "and runs only where no device is\n", devices);
        return 2;
    }
    (void)hipGetLastError();
    const std::vector<Case> emits = emit_cases(), resolves = resolve_cases();
    for (int fast = 0; fast < 2; fast++) {
        for (const Case &c : emits) {
            World w(fast);
            c.brk(w);
            const rls_status st = rls_trace_sss_probe_emit(w.ctx, w.n, w.cp, w.P, w.spp_n, 7u, 0u, w.qp);
            const char *msg = st == RLS_OK ? "" : rls_last_error();
            printf("emit\t%s\t%d\t%d\t%d\t%s\t%s\n", c.what.c_str(), fast, st, c.status, c.text.c_str(), msg);
        }
        for (const Case &c : resolves) {
            World w(fast);
            c.brk(w);
            const rls_status st = rls_trace_sss_scatter_resolve(w.ctx, w.n, w.cp, w.P, w.spp_n, w.qp, w.hp, w.cavity,
                                                                w.literal, w.result, w.depth);
            const char *msg = st == RLS_OK ? "" : rls_last_error();
            printf("resolve\t%s\t%d\t%d\t%d\t%s\t%s\n", c.what.c_str(), fast, st, c.status, c.text.c_str(), msg);
        }
    }
    return 0;
}
