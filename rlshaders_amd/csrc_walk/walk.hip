// walk.hip -- rlSss's probe walk on the device (include/rlshaders_amd_walk.h): the host side of librls_walk.so -- the scratch's
// layout, the checks of its own structs, the launches of a begin and of a step, the C ABI.  The kernels are in
// rls_walk_device.hpp; what a walk over an active list needs whichever rays it walks -- the tile arithmetic, the carve, the
// checks of a ray count, a context and a list, the scan and placement launches, the read of a count -- is in rls_walk_list.hpp,
// which the shadow rays' walk includes too.  The scan of the tile counts is the trace library's, included from its source
// (csrc_trace/rls_trace_queue.hpp over csrc_trace/rls_trace_device.hpp), not copied.  That header's other kernels are
// templates nothing here instantiates, but for hits_compact_kernel, which this code object carries unused.
//
// A third companion beside librls_ggx_rr.so and librls_trace.so, for the same reason: the product's device code and the trace
// library's surface stay what they are.  Built once (rlshaders_amd/build.py, build_walk_library): the walk is mode-free, so
// there is one code object, compiled with RLS_FAST=0 -- IEEE arithmetic, the correctly rounded square root.
#include <string.h>

#include <algorithm>

#include "../csrc_trace/rls_trace_device.hpp"
#include "../../include/rlshaders_amd_walk.h"

#if RLS_FAST
#error "walk.hip has no FAST flavour"
#endif

namespace {

#include "../csrc_trace/rls_trace_queue.hpp"
#include "rls_walk_list.hpp"
#include "rls_walk_device.hpp"

// The scratch of a walk over `rays` probe rays, each part 256-byte aligned: an entry's flag byte and new maxdist, the tiles'
// survivor counts, the scan's tile sums.  One step's working set: nothing in it outlives the step.
struct WalkScratch {
    uint8_t *flag;
    float *left;
    int64_t *counts, *totals;
    size_t bytes;
};
inline WalkScratch walk_scratch(void *base, int64_t rays)
{
    WalkScratch s = {};
    Carve c = { (char *)base, 0 };
    const int64_t tiles = walk_tiles(rays);
    s.flag = c.take<uint8_t>(rays);
    s.left = c.take<float>(rays);
    s.counts = c.take<int64_t>(tiles + 1);
    s.totals = c.take<int64_t>(scan_tiles(tiles));
    s.bytes = c.off;
    return s;
}

// the walk: its size, its points, its hits, its scratch; fn: the entry point the message names
rls_status check_walk(const char *fn, const rls_context *ctx, const rls_walk *w)
{
    if (rls_status s = check_ctx(fn, ctx)) return s;
    RLS_REQUIRE_IN(fn, w != nullptr, "walk is NULL");
    if (rls_status s = check_rays(fn, w->rays)) return s;
    RLS_REQUIRE_IN(fn, w->point != nullptr || w->spp >= 1, "walk.spp < 1 and walk.point is NULL");
    RLS_REQUIRE_IN(fn, w->foreign == RLS_WALK_FOREIGN_STOPS || w->foreign == RLS_WALK_FOREIGN_SKIPS,
                   "walk.foreign is neither RLS_WALK_FOREIGN_STOPS nor RLS_WALK_FOREIGN_SKIPS");
    RLS_REQUIRE_IN(fn, w->hits.max_hits >= 1 && w->hits.max_hits <= RLS_MAX_PROBE_HITS, "walk.hits.max_hits must be in [1, 12]");
    RLS_REQUIRE_IN(fn, w->hits.stride >= w->rays, "walk.hits.stride < walk.rays");
    RLS_REQUIRE_IN(fn, w->rays == 0 || rlsh::has3(w->P), "walk.P plane is NULL");
    RLS_REQUIRE_IN(fn, w->rays == 0 || (w->hits.count != nullptr && rlsh::has3(w->hits.P) && rlsh::has3(w->hits.N)),
                   "walk.hits.count, walk.hits.P or walk.hits.N plane is NULL");
    RLS_REQUIRE_IN(fn, w->scratch != nullptr && w->scratch_bytes >= walk_scratch(nullptr, w->rays).bytes,
                   "walk.scratch is NULL or smaller than rls_walk_scratch_bytes");
    return RLS_OK;
}

WalkIO walk_io(const rls_walk *w, const rls_walk_rays *out, int64_t bound)
{
    const WalkScratch sc = walk_scratch(w->scratch, w->rays);
    WalkIO io = {};
    io.w = *w; io.out = *out;
    io.bound = bound; io.tiles = walk_tiles(bound);
    io.flag = sc.flag; io.left = sc.left; io.counts = sc.counts;
    return io;
}

} // namespace

extern "C" {

rls_status rls_walk_scratch_bytes(int64_t rays, size_t *bytes)
{
    RLS_REQUIRE(bytes != nullptr, "bytes is NULL");
    if (rls_status s = check_rays(__func__, rays)) return s;
    *bytes = walk_scratch(nullptr, rays).bytes;
    return RLS_OK;
}

rls_status rls_walk_begin(rls_context *ctx, const rls_walk *w, const rls_probe_queue *q, const rls_walk_rays *out)
{
    if (rls_status s = check_walk(__func__, ctx, w)) return s;
    RLS_REQUIRE(q != nullptr, "queue is NULL");
    RLS_REQUIRE(q->capacity >= w->rays, "queue.capacity < walk.rays");
    RLS_REQUIRE(w->rays == 0 || (rlsh::has3(q->origin) && rlsh::has3(q->dir) && q->maxdist != nullptr),
                "queue.origin, queue.dir or queue.maxdist plane is NULL");
    if (rls_status s = check_list(__func__, out, w->rays, false)) return s;
    WalkIO io = walk_io(w, out, w->rays);
    io.q = *q;
    hipLaunchKernelGGL(walk_begin_kernel, rlsh::grid_for(ctx, io.bound, kWalkTile), dim3(rlsh::kBlock), 0, ctx->stream, io);
    if (rls_status s = rlsh::check_launch("walk_begin_kernel")) return s;
    return scan_and_place(ctx, io, walk_scratch(w->scratch, w->rays).totals, walk_place_kernel<true>, __func__);
}

rls_status rls_walk_step(rls_context *ctx, const rls_walk *w, const rls_walk_rays *in, const rls_walk_found *found, int64_t bound,
                         const rls_walk_rays *out)
{
    if (rls_status s = check_walk(__func__, ctx, w)) return s;
    if (rls_status s = check_list(__func__, in, w->rays, true)) return s;
    if (rls_status s = check_list(__func__, out, w->rays, false)) return s;
    if (rls_status s = check_in_is_not_out(__func__, in, out, w->rays)) return s;
    RLS_REQUIRE(found != nullptr, "found is NULL");
    RLS_REQUIRE(w->rays == 0 || (found->hit != nullptr && found->t != nullptr && rlsh::has3(found->P) && rlsh::has3(found->N) &&
                                 rlsh::has3(found->Ns)),
                "found.hit, found.t, found.P, found.N or found.Ns plane is NULL");
    RLS_REQUIRE((w->own == nullptr) == (found->object == nullptr), "walk.own and found.object must be both set or both NULL");
    WalkIO io = walk_io(w, out, step_bound(bound, w->rays));
    io.in = *in; io.f = *found;
    hipLaunchKernelGGL(walk_step_kernel, rlsh::grid_for(ctx, io.bound, kWalkTile), dim3(rlsh::kBlock), 0, ctx->stream, io);
    if (rls_status s = rlsh::check_launch("walk_step_kernel")) return s;
    return scan_and_place(ctx, io, walk_scratch(w->scratch, w->rays).totals, walk_place_kernel<false>, __func__);
}

rls_status rls_walk_active(rls_context *ctx, const rls_walk_rays *rays, int64_t *host_count)
{
    return list_active(__func__, ctx, rays, host_count);
}

} // extern "C"
