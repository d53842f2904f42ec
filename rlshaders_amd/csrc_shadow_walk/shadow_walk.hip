// shadow_walk.hip -- shadow rays walked on the device (include/rlshaders_amd_shadow_walk.h): the host side of
// librls_shadow_walk.so -- the scratch's carve, the argument checks (each written once), the launches of a begin and of a step,
// the C ABI.  The kernels are in rls_shadow_walk_device.hpp; the scan of the tile counts is the trace library's, included from
// its source (csrc_trace/rls_trace_queue.hpp over csrc_trace/rls_trace_device.hpp) as csrc_walk/walk.hip includes it, not
// copied.  That header's other kernels are templates nothing here instantiates, but for hits_compact_kernel, which this code
// object carries unused.
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
#include "rls_shadow_walk_device.hpp"

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int64_t walk_tiles(int64_t entries) { return std::max<int64_t>((entries + kShadowWalkTile - 1) / kShadowWalkTile, 1); }
inline int64_t scan_tiles(int64_t n) { return (n + kScanTile - 1) / kScanTile; }
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
    char *p = (char *)base;
    size_t off = 0;
    auto carve = [&](size_t bytes) { char *at = p + off; off += align256(bytes); return (void *)at; };
    const int64_t tiles = walk_tiles(rays);
    s.state = (uint16_t *)carve((size_t)rays * sizeof(uint16_t));
    s.left = (float *)carve((size_t)rays * sizeof(float));
    s.counts = (int64_t *)carve((size_t)(tiles + 1) * sizeof(int64_t));
    s.totals = (int64_t *)carve((size_t)scan_tiles(tiles) * sizeof(int64_t));
    s.bytes = off;
    return s;
}

// ---- the argument checks, each written once; fn: the entry point its message names ---------------------------------------------
rls_status check_rays(const char *fn, int64_t rays)
{
    RLS_REQUIRE_IN(fn, rays >= 0, "rays < 0");
    RLS_REQUIRE_IN(fn, rays <= (int64_t)UINT32_MAX, "rays > 2^32 - 1 (the list's ray index is 32-bit)");
    return RLS_OK;
}
rls_status check_ctx(const char *fn, const rls_context *ctx)
{
    RLS_REQUIRE_IN(fn, ctx != nullptr, "ctx is NULL");
    return RLS_OK;
}
// the walk: its size, its budget, its planes, its scratch
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
// a list: its count always, its planes where it can hold an entry of the walk (in: the list a step reads, else the one written)
rls_status check_list(const char *fn, const rls_walk_rays *l, int64_t rays, bool in)
{
    RLS_REQUIRE_IN(fn, l != nullptr, in ? "in is NULL" : "out is NULL");
    RLS_REQUIRE_IN(fn, l->count != nullptr, in ? "in.count is NULL" : "out.count is NULL");
    RLS_REQUIRE_IN(fn, l->capacity >= rays, in ? "in.capacity < walk.rays" : "out.capacity < walk.rays");
    RLS_REQUIRE_IN(fn, rays == 0 || (l->ray != nullptr && rlsh::has3(l->origin) && rlsh::has3(l->dir) && l->maxdist != nullptr &&
                                     l->trials != nullptr),
                   in ? "in.ray, in.origin, in.dir, in.maxdist or in.trials plane is NULL"
                      : "out.ray, out.origin, out.dir, out.maxdist or out.trials plane is NULL");
    return RLS_OK;
}

// steps 2 and 3 of a begin or a step: the tile counts scanned (the grand total to the output list's count), the survivors placed
template <bool BEGIN>
rls_status scan_and_place(rls_context *ctx, const ShadowWalkIO &io, int64_t *totals, const char *fn)
{
    rls_status s;
    const int64_t st = scan_tiles(io.tiles);
    hipLaunchKernelGGL(trace_scan_block_kernel, dim3((unsigned)st), dim3(rlsh::kBlock), 0, ctx->stream, io.counts, io.tiles, totals);
    if ((s = rlsh::check_launch("trace_scan_block_kernel")) != RLS_OK) return s;
    hipLaunchKernelGGL(trace_scan_totals_kernel, dim3(1), dim3(rlsh::kBlock), 0, ctx->stream, totals, st, io.out.count);
    if ((s = rlsh::check_launch("trace_scan_totals_kernel")) != RLS_OK) return s;
    hipLaunchKernelGGL(trace_scan_add_kernel, rlsh::grid_for(ctx, io.tiles), dim3(rlsh::kBlock), 0, ctx->stream, io.counts, io.tiles,
                       (const int64_t *)totals);
    if ((s = rlsh::check_launch("trace_scan_add_kernel")) != RLS_OK) return s;
    hipLaunchKernelGGL(shadow_place_kernel<BEGIN>, rlsh::grid_for(ctx, io.bound, kShadowWalkTile), dim3(rlsh::kBlock), 0, ctx->stream,
                       io);
    return rlsh::check_launch(fn);
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
    hipLaunchKernelGGL(shadow_begin_kernel, rlsh::grid_for(ctx, io.bound, kShadowWalkTile), dim3(rlsh::kBlock), 0, ctx->stream, io);
    if (rls_status s = rlsh::check_launch("shadow_begin_kernel")) return s;
    return scan_and_place<true>(ctx, io, shadow_scratch(w->scratch, w->rays).totals, __func__);
}

rls_status rls_shadow_walk_step(rls_context *ctx, const rls_shadow_walk *w, const rls_walk_rays *in,
                                const rls_shadow_walk_found *found, int64_t bound, const rls_walk_rays *out)
{
    if (rls_status s = check_walk(__func__, ctx, w)) return s;
    if (rls_status s = check_list(__func__, in, w->rays, true)) return s;
    if (rls_status s = check_list(__func__, out, w->rays, false)) return s;
    RLS_REQUIRE(in->count != out->count && (w->rays == 0 || (in->ray != out->ray && in->maxdist != out->maxdist)),
                "out is in: a step reads one list and writes the other");
    RLS_REQUIRE(found != nullptr, "found is NULL");
    RLS_REQUIRE(w->rays == 0 || (found->hit != nullptr && found->t != nullptr && rlsh::has3(found->P) && has3(found->opacity)),
                "found.hit, found.t, found.P or found.opacity plane is NULL");
    RLS_REQUIRE(found->index == nullptr || found->table_count >= 1, "found.index is set with found.table_count == 0");
    // no more entries than rays: the scratch is sized by the walk's rays
    ShadowWalkIO io = walk_io(w, out, bound < 0 || bound > w->rays ? w->rays : bound);
    io.in = *in; io.f = *found;
    hipLaunchKernelGGL(shadow_step_kernel, rlsh::grid_for(ctx, io.bound, kShadowWalkTile), dim3(rlsh::kBlock), 0, ctx->stream, io);
    if (rls_status s = rlsh::check_launch("shadow_step_kernel")) return s;
    return scan_and_place<false>(ctx, io, shadow_scratch(w->scratch, w->rays).totals, __func__);
}

rls_status rls_shadow_walk_active(rls_context *ctx, const rls_walk_rays *rays, int64_t *host_count)
{
    if (rls_status s = check_ctx(__func__, ctx)) return s;
    RLS_REQUIRE(rays != nullptr && rays->count != nullptr, "rays or rays.count is NULL");
    RLS_REQUIRE(host_count != nullptr, "host_count is NULL");
    RLS_HIP_TRY(hipSetDevice(ctx->device));
    RLS_HIP_TRY(hipMemcpyAsync(host_count, rays->count, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    RLS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RLS_OK;
}

} // extern "C"
