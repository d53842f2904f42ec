// shadow_walk.hip -- shadow rays walked on the device (include/rlshaders_amd_shadow_walk.h): the host side of
// librls_shadow_walk.so -- the scratch's layout, the checks of its own structs, the launches of a begin and of a step, the
// C ABI.  The kernels are in rls_shadow_walk_device.hpp; what a walk over an active list needs whichever rays it walks is the
// probe walk's, included from its source (csrc_walk/rls_walk_list.hpp) and compiled into this code object, not copied; so is
// the trace library's scan of the tile counts (csrc_trace/rls_trace_queue.hpp over csrc_trace/rls_trace_device.hpp).  That
// header's other kernels are templates nothing here instantiates, but for hits_compact_kernel, which this code object carries
// unused.
//
// A fourth companion beside librls_ggx_rr.so, librls_trace.so and librls_walk.so, for the same reason: the product's device code
// and the other libraries' surfaces stay what they are.  Built once (rlshaders_amd/build.py, build_shadow_walk_library): the
// walk is mode-free, so there is one code object, compiled with RLS_FAST=0 -- IEEE arithmetic.
#include <string.h>

#include <algorithm>

#include "../csrc_trace/rls_trace_device.hpp"
#include "../../include/rlshaders_amd_shadow_walk.h"

#if RLS_FAST
#error "shadow_walk.hip has no FAST flavour"
#endif

namespace {

#include "../csrc_trace/rls_trace_queue.hpp"
#include "../csrc_walk/rls_walk_list.hpp"
#include "rls_shadow_walk_device.hpp"

inline bool has3(rls_crgb v) { return v.r && v.g && v.b; }
inline bool none3(rls_crgb v) { return !v.r && !v.g && !v.b; }

// The scratch of a walk over `rays` shadow rays, each part 256-byte aligned (the header's table): an entry's state and new
// maxdist, the tiles' survivor counts, the scan's tile sums.  One step's working set: nothing in it outlives the step.
struct ShadowScratch {
    uint16_t *state;
    float *left;
    int64_t *counts, *totals;
    size_t bytes;
};
inline ShadowScratch shadow_scratch(void *base, int64_t rays)
{
    ShadowScratch s = {};
    Carve c = { (char *)base, 0 };
    const int64_t tiles = walk_tiles(rays);
    s.state = c.take<uint16_t>(rays);
    s.left = c.take<float>(rays);
    s.counts = c.take<int64_t>(tiles + 1);
    s.totals = c.take<int64_t>(scan_tiles(tiles));
    s.bytes = c.off;
    return s;
}

// the walk: its size, its budget, its planes, its scratch; fn: the entry point the message names
rls_status check_walk(const char *fn, const rls_context *ctx, const rls_shadow_walk *w)
{
    if (rls_status s = check_ctx(fn, ctx)) return s;
    RLS_REQUIRE_IN(fn, w != nullptr, "walk is NULL");
    if (rls_status s = check_rays(fn, w->rays)) return s;
    RLS_REQUIRE_IN(fn, w->max_steps >= 1 && w->max_steps <= RLS_SHADOW_WALK_MAX_STEPS, "walk.max_steps must be in [1, 255]");
    RLS_REQUIRE_IN(fn, has3(w->base) || none3(w->base), "walk.base is partly NULL: all three planes or none");
    RLS_REQUIRE_IN(fn, w->rays == 0 || rlsh::has3(w->visibility), "walk.visibility plane is NULL");
    RLS_REQUIRE_IN(fn, w->scratch != nullptr && w->scratch_bytes >= shadow_scratch(nullptr, w->rays).bytes,
                   "walk.scratch is NULL or smaller than rls_shadow_walk_scratch_bytes");
    return RLS_OK;
}

ShadowWalkIO walk_io(const rls_shadow_walk *w, const rls_walk_rays *out, int64_t bound)
{
    const ShadowScratch sc = shadow_scratch(w->scratch, w->rays);
    ShadowWalkIO io = {};
    io.w = *w; io.out = *out;
    io.bound = bound; io.tiles = walk_tiles(bound);
    io.state = sc.state; io.left = sc.left; io.counts = sc.counts;
    return io;
}

} // namespace

extern "C" {

rls_status rls_shadow_walk_scratch_bytes(int64_t rays, size_t *bytes)
{
    RLS_REQUIRE(bytes != nullptr, "bytes is NULL");
    if (rls_status s = check_rays(__func__, rays)) return s;
    *bytes = shadow_scratch(nullptr, rays).bytes;
    return RLS_OK;
}

rls_status rls_shadow_walk_begin(rls_context *ctx, const rls_shadow_walk *w, const rls_shadow_queue *q, const rls_walk_rays *out)
{
    if (rls_status s = check_walk(__func__, ctx, w)) return s;
    RLS_REQUIRE(w->rays == 0 || rlsh::has3(w->O), "walk.O plane is NULL");
    RLS_REQUIRE(q != nullptr, "queue is NULL");
    RLS_REQUIRE(q->capacity >= w->rays, "queue.capacity < walk.rays");
    RLS_REQUIRE(w->rays == 0 || (rlsh::has3(q->dir) && q->maxdist != nullptr), "queue.dir or queue.maxdist plane is NULL");
    RLS_REQUIRE(w->rays == 0 || q->point != nullptr, "queue.point is NULL: the walk reads every ray's origin through it");
    if (rls_status s = check_list(__func__, out, w->rays, false)) return s;
    ShadowWalkIO io = walk_io(w, out, w->rays);
    io.q = *q;
    hipLaunchKernelGGL(shadow_begin_kernel, rlsh::grid_for(ctx, io.bound, kWalkTile), dim3(rlsh::kBlock), 0, ctx->stream, io);
    if (rls_status s = rlsh::check_launch("shadow_begin_kernel")) return s;
    return scan_and_place(ctx, io, shadow_scratch(w->scratch, w->rays).totals, shadow_place_kernel<true>, __func__);
}

rls_status rls_shadow_walk_step(rls_context *ctx, const rls_shadow_walk *w, const rls_walk_rays *in,
                                const rls_shadow_walk_found *found, int64_t bound, const rls_walk_rays *out)
{
    if (rls_status s = check_walk(__func__, ctx, w)) return s;
    if (rls_status s = check_list(__func__, in, w->rays, true)) return s;
    if (rls_status s = check_list(__func__, out, w->rays, false)) return s;
    if (rls_status s = check_in_is_not_out(__func__, in, out, w->rays)) return s;
    RLS_REQUIRE(found != nullptr, "found is NULL");
    RLS_REQUIRE(w->rays == 0 || (found->hit != nullptr && found->t != nullptr && rlsh::has3(found->P) && has3(found->opacity)),
                "found.hit, found.t, found.P or found.opacity plane is NULL");
    RLS_REQUIRE(found->index == nullptr || found->table_count >= 1, "found.index is set with found.table_count == 0");
    ShadowWalkIO io = walk_io(w, out, step_bound(bound, w->rays));
    io.in = *in; io.f = *found;
    hipLaunchKernelGGL(shadow_step_kernel, rlsh::grid_for(ctx, io.bound, kWalkTile), dim3(rlsh::kBlock), 0, ctx->stream, io);
    if (rls_status s = rlsh::check_launch("shadow_step_kernel")) return s;
    return scan_and_place(ctx, io, shadow_scratch(w->scratch, w->rays).totals, shadow_place_kernel<false>, __func__);
}

rls_status rls_shadow_walk_active(rls_context *ctx, const rls_walk_rays *rays, int64_t *host_count)
{
    return list_active(__func__, ctx, rays, host_count);
}

} // extern "C"
