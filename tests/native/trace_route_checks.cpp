// trace_route_checks.cpp -- the argument checks of the five routing entry points (rls_trace_route_scratch_bytes, _hits, _gather,
// _scatter, _fill; librls_trace.so), driven with dummy planes and no GPU (tests/test_trace_route_checks.py builds and runs it),
// in the style of trace_sss_checks.cpp.
//
// Every case starts from a set of arguments that passes every check, breaks one or two of them (or none) and records what
// the call returns.  A call whose arguments pass reaches the launch, and with no device there its hipSetDevice fails: status
// RLS_ERR_HIP.  That is only safe while no device is visible: on a GPU the dummy planes would reach a kernel.  The driver
// refuses to run if HIP reports a device.
//
// Output: one tab-separated line per case:
//   verb  case  status  expected-status  expected-text  message
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <functional>
#include <string>
#include <vector>

#include "../../rlshaders_amd/csrc/rls_internal.hpp"
#include "../../include/rlshaders_amd_trace.h"

namespace {

float g_plane[64], g_other[64];         // the stand-ins for every device plane: never dereferenced without a device
uint8_t g_bytes[64], g_bytes2[64];
uint32_t g_index[64];
int64_t g_offsets[RLS_ROUTE_MAX_BINS + 2];

struct World {
    rls_context context;
    rls_context *ctx;
    int64_t rays, m;
    const uint8_t *bin;
    rls_hit_routes r;
    const rls_hit_routes *rp;
    const uint32_t *index;
    rls_route_planes p;
    const rls_route_planes *pp;
    int n_planes;
    float *dst[RLS_ROUTE_MAX_W32 + 1];
    float *const *dstp;
    float value[RLS_ROUTE_MAX_W32 + 1];
    const float *valuep;
    size_t bytes;
    size_t *bytesp;

    World()
    {
        context = {};
        context.device = 0;
        context.compute_units = 256;
        context.blocks_per_cu = 64;
        ctx = &context;
        rays = 100000;
        m = 1000;
        bin = g_bytes;
        r = {};
        r.bins = 3;
        r.offsets = g_offsets;
        r.order = g_index;
        r.slot = g_index;
        r.scratch = g_plane;
        rls_trace_route_scratch_bytes(rays, r.bins, &r.scratch_bytes);
        rp = &r;
        index = g_index;
        p = {};
        p.n_w32 = 12;
        p.n_u8 = 5;
        for (int k = 0; k < RLS_ROUTE_MAX_W32; k++) { p.src_w32[k] = g_plane; p.dst_w32[k] = g_other; }
        for (int k = 0; k < RLS_ROUTE_MAX_U8; k++) { p.src_u8[k] = g_bytes; p.dst_u8[k] = g_bytes2; }
        pp = &p;
        n_planes = 3;
        for (int k = 0; k <= RLS_ROUTE_MAX_W32; k++) { dst[k] = g_plane; value[k] = 0.5f; }
        dstp = dst;
        valuep = value;
        bytes = 0;
        bytesp = &bytes;
    }
};

struct Case {
    std::string what;
    std::function<void(World &)> brk;
    int status;
    std::string text;                   // for a refusal: "<entry point>: <text>"
};

const int BAD = RLS_ERR_INVALID_ARGUMENT, HIP = RLS_ERR_HIP, OK = RLS_OK, UNSUPPORTED = RLS_ERR_UNSUPPORTED;
const char *const BINS = "bins must be in [1, 16]", *const LARGE = "rays > 2^32 - 1 (order is 32-bit: route in chunks)",
                  *const SCRATCH = "routes.scratch is NULL or smaller than rls_trace_route_scratch_bytes",
                  *const ORDER = "bin or routes.order is NULL", *const W32 = "planes.n_w32 must be in [0, 24]",
                  *const U8 = "planes.n_u8 must be in [0, 8]", *const WPLANE = "planes.src_w32 or planes.dst_w32 plane is NULL",
                  *const BPLANE = "planes.src_u8 or planes.dst_u8 plane is NULL", *const ALIAS = "a plane's dst is its src",
                  *const NPLANES = "n_planes must be in [1, 24]";

std::vector<Case> size_cases()
{
    return {
        { "bytes NULL", [](World &w) { w.bytesp = nullptr; }, BAD, "bytes is NULL" },
        { "rays < 0", [](World &w) { w.rays = -1; }, BAD, "rays < 0" },
        { "rays = 2^32", [](World &w) { w.rays = (int64_t)1 << 32; }, UNSUPPORTED, LARGE },
        { "rays = 2^32 - 1", [](World &w) { w.rays = ((int64_t)1 << 32) - 1; }, OK, "" },
        { "bins 0", [](World &w) { w.r.bins = 0; }, BAD, BINS },
        { "bins 17", [](World &w) { w.r.bins = 17; }, BAD, BINS },
        { "bins -1", [](World &w) { w.r.bins = -1; }, BAD, BINS },
        { "bins 16", [](World &w) { w.r.bins = 16; }, OK, "" },
        { "rays == 0", [](World &w) { w.rays = 0; }, OK, "" },
        { "valid", [](World &) {}, OK, "" },
    };
}

std::vector<Case> hits_cases()
{
    return {
        { "ctx NULL", [](World &w) { w.ctx = nullptr; }, BAD, "ctx is NULL" },
        { "routes NULL", [](World &w) { w.rp = nullptr; }, BAD, "routes is NULL" },
        { "rays < 0", [](World &w) { w.rays = -1; }, BAD, "rays < 0" },
        { "rays = 2^32", [](World &w) { w.rays = (int64_t)1 << 32; w.r.scratch_bytes = (size_t)1 << 40; }, UNSUPPORTED, LARGE },
        { "bins 0", [](World &w) { w.r.bins = 0; }, BAD, BINS },
        { "bins 17", [](World &w) { w.r.bins = 17; w.r.scratch_bytes = (size_t)1 << 40; }, BAD, BINS },
        { "offsets NULL", [](World &w) { w.r.offsets = nullptr; }, BAD, "routes.offsets is NULL" },
        { "bin NULL", [](World &w) { w.bin = nullptr; }, BAD, ORDER },
        { "order NULL", [](World &w) { w.r.order = nullptr; }, BAD, ORDER },
        { "scratch NULL", [](World &w) { w.r.scratch = nullptr; }, BAD, SCRATCH },
        { "scratch short", [](World &w) { w.r.scratch_bytes -= 1; }, BAD, SCRATCH },
        { "scratch of fewer bins", [](World &w) { w.r.bins = 16; }, BAD, SCRATCH },
        { "slot NULL", [](World &w) { w.r.slot = nullptr; }, HIP, "" },
        { "scratch larger", [](World &w) { w.r.scratch_bytes += 4096; }, HIP, "" },
        { "bins 1", [](World &w) { w.r.bins = 1; }, HIP, "" },
        { "valid", [](World &) {}, HIP, "" },
        // no ray: offsets is still written, a launch; bin and order are not needed
        { "rays == 0", [](World &w) { w.rays = 0; w.bin = nullptr; w.r.order = nullptr; w.r.slot = nullptr; }, HIP, "" },
        { "rays == 0, offsets NULL", [](World &w) { w.rays = 0; w.r.offsets = nullptr; }, BAD, "routes.offsets is NULL" },
        { "rays == 0, bins 0", [](World &w) { w.rays = 0; w.r.bins = 0; }, BAD, BINS },
        { "rays == 0, scratch NULL", [](World &w) { w.rays = 0; w.r.scratch = nullptr; }, BAD, SCRATCH },
    };
}

std::vector<Case> move_cases()
{
    return {
        { "ctx NULL", [](World &w) { w.ctx = nullptr; }, BAD, "ctx is NULL" },
        { "m < 0", [](World &w) { w.m = -1; }, BAD, "m < 0" },
        { "planes NULL", [](World &w) { w.pp = nullptr; }, BAD, "planes is NULL" },
        { "n_w32 -1", [](World &w) { w.p.n_w32 = -1; }, BAD, W32 },
        { "n_w32 25", [](World &w) { w.p.n_w32 = 25; }, BAD, W32 },
        { "n_u8 -1", [](World &w) { w.p.n_u8 = -1; }, BAD, U8 },
        { "n_u8 9", [](World &w) { w.p.n_u8 = 9; }, BAD, U8 },
        { "no plane", [](World &w) { w.p.n_w32 = 0; w.p.n_u8 = 0; }, BAD, "planes holds no plane" },
        { "src_w32 NULL below the count", [](World &w) { w.p.src_w32[11] = nullptr; }, BAD, WPLANE },
        { "dst_w32 NULL below the count", [](World &w) { w.p.dst_w32[0] = nullptr; }, BAD, WPLANE },
        { "src_u8 NULL below the count", [](World &w) { w.p.src_u8[4] = nullptr; }, BAD, BPLANE },
        { "dst_u8 NULL below the count", [](World &w) { w.p.dst_u8[2] = nullptr; }, BAD, BPLANE },
        { "word dst == src", [](World &w) { w.p.dst_w32[5] = g_plane; }, BAD, ALIAS },
        { "byte dst == src", [](World &w) { w.p.dst_u8[1] = g_bytes; }, BAD, ALIAS },
        { "index NULL", [](World &w) { w.index = nullptr; }, BAD, "index is NULL" },
        { "planes NULL past the count", [](World &w) { w.p.src_w32[12] = nullptr; w.p.dst_u8[5] = nullptr; }, HIP, "" },
        { "dst == src past the count", [](World &w) { w.p.dst_w32[12] = g_plane; }, HIP, "" },
        { "24 and 8 planes", [](World &w) { w.p.n_w32 = 24; w.p.n_u8 = 8; }, HIP, "" },
        { "words only", [](World &w) { w.p.n_u8 = 0; }, HIP, "" },
        { "bytes only", [](World &w) { w.p.n_w32 = 0; }, HIP, "" },
        { "valid", [](World &) {}, HIP, "" },
        // nothing to move: no launch, the index is not needed; a bad argument is still refused
        { "m == 0", [](World &w) { w.m = 0; w.index = nullptr; }, OK, "" },
        { "m == 0, planes NULL", [](World &w) { w.m = 0; w.pp = nullptr; }, BAD, "planes is NULL" },
        { "m == 0, n_w32 25", [](World &w) { w.m = 0; w.p.n_w32 = 25; }, BAD, W32 },
        { "m == 0, dst == src", [](World &w) { w.m = 0; w.p.dst_w32[0] = g_plane; }, BAD, ALIAS },
        { "m == 0, ctx NULL", [](World &w) { w.m = 0; w.ctx = nullptr; }, BAD, "ctx is NULL" },
    };
}

std::vector<Case> fill_cases()
{
    return {
        { "ctx NULL", [](World &w) { w.ctx = nullptr; }, BAD, "ctx is NULL" },
        { "m < 0", [](World &w) { w.m = -1; }, BAD, "m < 0" },
        { "n_planes 0", [](World &w) { w.n_planes = 0; }, BAD, NPLANES },
        { "n_planes 25", [](World &w) { w.n_planes = 25; }, BAD, NPLANES },
        { "dst NULL", [](World &w) { w.dstp = nullptr; }, BAD, "dst or value is NULL" },
        { "value NULL", [](World &w) { w.valuep = nullptr; }, BAD, "dst or value is NULL" },
        { "dst plane NULL below the count", [](World &w) { w.dst[2] = nullptr; }, BAD, "dst plane is NULL" },
        { "index NULL", [](World &w) { w.index = nullptr; }, BAD, "index is NULL" },
        { "dst plane NULL past the count", [](World &w) { w.dst[3] = nullptr; }, HIP, "" },
        { "n_planes 24", [](World &w) { w.n_planes = 24; }, HIP, "" },
        { "n_planes 1", [](World &w) { w.n_planes = 1; }, HIP, "" },
        { "valid", [](World &) {}, HIP, "" },
        { "m == 0", [](World &w) { w.m = 0; w.index = nullptr; }, OK, "" },
        { "m == 0, n_planes 25", [](World &w) { w.m = 0; w.n_planes = 25; }, BAD, NPLANES },
        { "m == 0, dst plane NULL", [](World &w) { w.m = 0; w.dst[0] = nullptr; }, BAD, "dst plane is NULL" },
    };
}

void report(const char *verb, const Case &c, rls_status st)
{
    const char *msg = st == RLS_OK ? "" : rls_last_error();
    printf("%s\t%s\t%d\t%d\t%s\t%s\n", verb, c.what.c_str(), st, c.status, c.text.c_str(), msg);
}

} // namespace

int main()
{
    int devices = 0;
    if (hipGetDeviceCount(&devices) == hipSuccess && devices > 0) {
        fprintf(stderr, "trace_route_checks: %d HIP device(s) visible; this driver hands dummy planes to the entry points "
                        "and runs only where no device is\n", devices);
        return 2;
    }
    (void)hipGetLastError();
    for (const Case &c : size_cases()) {
        World w;
        c.brk(w);
        report("scratch_bytes", c, rls_trace_route_scratch_bytes(w.rays, w.r.bins, w.bytesp));
    }
    for (const Case &c : hits_cases()) {
        World w;
        c.brk(w);
        report("hits", c, rls_trace_route_hits(w.ctx, w.rays, w.bin, w.rp));
    }
    for (const Case &c : move_cases()) {
        for (int gather = 0; gather < 2; gather++) {
            World w;
            c.brk(w);
            report(gather ? "gather" : "scatter", c, gather ? rls_trace_route_gather(w.ctx, w.m, w.index, w.pp)
                                                            : rls_trace_route_scatter(w.ctx, w.m, w.index, w.pp));
        }
    }
    for (const Case &c : fill_cases()) {
        World w;
        c.brk(w);
        report("fill", c, rls_trace_route_fill(w.ctx, w.m, w.index, w.n_planes, w.dstp, w.valuep));
    }
    return 0;
}
