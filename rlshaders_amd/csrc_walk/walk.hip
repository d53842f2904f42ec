// walk.hip -- rlSss's probe walk on the device (include/rlshaders_amd_walk.h): the host side of librls_walk.so -- the scratch's
// carve, the argument checks (each written once), the launches of a begin and of a step, the C ABI.  The kernels are in
// rls_walk_device.hpp; the scan of the tile counts is the trace library's, included from its source
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
#include "rls_walk_device.hpp"

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int64_t walk_tiles(int64_t entries) { return std::max<int64_t>((entries + kWalkTile - 1) / kWalkTile, 1); }
inline int64_t scan_tiles(int64_t n) { return (n + kScanTile - 1) / kScanTile; }

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
    char *p = (char *)base;
    size_t off = 0;
    auto carve = [&](size_t bytes) { char *at = p + off; off += align256(bytes); return (void *)at; };
    const int64_t tiles = walk_tiles(rays);
    s.flag = (uint8_t *)carve((size_t)rays);
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
// the walk: its size, its points, its hits, its scratch
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
rls_status scan_and_place(rls_context *ctx, const WalkIO &io, int64_t *totals, const char *fn)
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
    hipLaunchKernelGGL(walk_place_kernel<BEGIN>, rlsh::grid_for(ctx, io.bound, kWalkTile), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(fn);
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
    return scan_and_place<true>(ctx, io, walk_scratch(w->scratch, w->rays).totals, __func__);
}

rls_status rls_walk_step(rls_context *ctx, const rls_walk *w, const rls_walk_rays *in, const rls_walk_found *found, int64_t bound,
                         const rls_walk_rays *out)
{
    if (rls_status s = check_walk(__func__, ctx, w)) return s;
    if (rls_status s = check_list(__func__, in, w->rays, true)) return s;
    if (rls_status s = check_list(__func__, out, w->rays, false)) return s;
    RLS_REQUIRE(in->count != out->count && (w->rays == 0 || (in->ray != out->ray && in->maxdist != out->maxdist)),
                "out is in: a step reads one list and writes the other");
    RLS_REQUIRE(found != nullptr, "found is NULL");
    RLS_REQUIRE(w->rays == 0 || (found->hit != nullptr && found->t != nullptr && rlsh::has3(found->P) && rlsh::has3(found->N) &&
                                 rlsh::has3(found->Ns)),
                "found.hit, found.t, found.P, found.N or found.Ns plane is NULL");
    RLS_REQUIRE((w->own == nullptr) == (found->object == nullptr), "walk.own and found.object must be both set or both NULL");
    // no more entries than rays: the scratch is sized by the walk's rays
    WalkIO io = walk_io(w, out, bound < 0 || bound > w->rays ? w->rays : bound);
    io.in = *in; io.f = *found;
    hipLaunchKernelGGL(walk_step_kernel, rlsh::grid_for(ctx, io.bound, kWalkTile), dim3(rlsh::kBlock), 0, ctx->stream, io);
    if (rls_status s = rlsh::check_launch("walk_step_kernel")) return s;
    return scan_and_place<false>(ctx, io, walk_scratch(w->scratch, w->rays).totals, __func__);
}

rls_status rls_walk_active(rls_context *ctx, const rls_walk_rays *rays, int64_t *host_count)
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
