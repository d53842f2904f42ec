// any.hip -- any-hit shadow queries (include/rlshaders_amd_nearest_any.h): the host side of librls_nearest_any.so -- the argument
// checks (each written once), the one launch path of both queries, the flag table's launch, the C ABI.  A triangle's class, the
// candidate predicate, the traversal and the kernels are in rls_nearest_any.hpp.
//
// A ninth companion beside librls_ggx_rr.so, librls_trace.so, librls_walk.so, librls_shadow_walk.so, librls_nearest.so,
// librls_nearest_refit.so, librls_nearest_rebuild.so and librls_nearest_group.so, for the same reason: the other libraries'
// device code and surfaces stay what they are.  It reads a scene through rls_nearest_scene.hpp alone and calls nothing of
// librls_nearest.so.  Built once (rlshaders_amd/build.py, build_nearest_any_library): mode-free, one code object, compiled with
// RLS_FAST=0.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../csrc/rls_internal.hpp"
#include "../../include/rlshaders_amd_nearest_any.h"

#if RLS_FAST
#error "any.hip has no FAST flavour"
#endif

#include "rls_nearest_scene.hpp"
#include "rls_nearest_any.hpp"

static_assert(kNearestStack == RLS_NEAREST_STACK, "the header's stack size is the kernel's");
static_assert(kAnyClear == RLS_NEAREST_ANY_CLEAR && kAnyBlocked == RLS_NEAREST_ANY_BLOCKED && kAnyVeiled == RLS_NEAREST_ANY_VEILED,
              "the header's states are the kernel's");

namespace {

inline bool all3(rls_rgb v) { return v.r && v.g && v.b; }
inline bool none3(rls_rgb v) { return !v.r && !v.g && !v.b; }
inline bool all3(rls_crgb v) { return v.r && v.g && v.b; }
inline bool none3(rls_crgb v) { return !v.r && !v.g && !v.b; }
inline int64_t tiles_of(int64_t count) { return (count + rlsh::kBlock - 1) / rlsh::kBlock; }

const char *const kLayoutText =
    "scene is not a scene of this build's layout (librls_nearest.so and librls_nearest_any.so must be of one build)";

// ---- the argument checks, each written once; fn: the entry point its message names ---------------------------------------------
rls_status check_found(const char *fn, const rls_nearest_any_found *f, int64_t rays)
{
    RLS_REQUIRE_IN(fn, f != nullptr, "found is NULL");
    RLS_REQUIRE_IN(fn, rays == 0 || f->state != nullptr, "found.state plane is NULL");
    RLS_REQUIRE_IN(fn, f->opaque == nullptr || f->opaque_count >= 1, "found.opaque is set with found.opaque_count == 0");
    RLS_REQUIRE_IN(fn, (all3(f->base) || none3(f->base)) && (all3(f->visibility) || none3(f->visibility)),
                   "found.base or found.visibility is partly NULL: all three planes or none");
    return RLS_OK;
}

// the one launch path: both queries arrive here with their rays in one struct
rls_status launch(const char *fn, rls_context *ctx, const rls_nearest_scene *scene, const rls_nearest_rays &r,
                  const rls_nearest_any_found *f)
{
    RLS_REQUIRE_IN(fn, r.rays >= 0, "rays < 0");
    RLS_REQUIRE_IN(fn, r.rays <= (int64_t)UINT32_MAX, "rays > 2^32 - 1 (a ray id is 32-bit)");
    RLS_REQUIRE_IN(fn, r.rays == 0 || (rlsh::has3(r.origin) && rlsh::has3(r.dir)), "rays.origin or rays.dir plane is NULL");
    if (rls_status s = check_found(fn, f, r.rays)) return s;
    RLS_REQUIRE_IN(fn, scene->layout == kNearestSceneLayout, kLayoutText);
    if (r.rays == 0) return RLS_OK;
    RLS_REQUIRE_IN(fn, scene->device == ctx->device, "the scene lives on another device than ctx");
    AnyIO io = {};
    io.nodes = scene->nodes; io.tris = scene->tris; io.node_count = scene->info.nodes;
    io.cls.surface = scene->surface; io.cls.flags = f->opaque; io.cls.count = f->opaque_count;
    io.r = r; io.f = *f;
    io.tiles = tiles_of(r.rays);
    hipLaunchKernelGGL(any_kernel, rlsh::grid_for(ctx, r.rays), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(fn);
}

} // namespace

extern "C" {

rls_status rls_nearest_any_hits(rls_context *ctx, const rls_nearest_scene *scene, const rls_nearest_rays *rays,
                                const rls_nearest_any_found *found)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(scene != nullptr, "scene is NULL");
    RLS_REQUIRE(rays != nullptr, "rays is NULL");
    return launch(__func__, ctx, scene, *rays, found);
}

rls_status rls_nearest_any_walk_hits(rls_context *ctx, const rls_nearest_scene *scene, const rls_walk_rays *list, int64_t bound,
                                     const rls_nearest_any_found *found)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(scene != nullptr, "scene is NULL");
    RLS_REQUIRE(list != nullptr, "list is NULL");
    RLS_REQUIRE(list->count != nullptr, "list.count is NULL");
    RLS_REQUIRE(list->capacity >= 0, "list.capacity < 0");
    const int64_t rays = bound < 0 || bound > list->capacity ? list->capacity : bound;
    RLS_REQUIRE(rays == 0 || (list->ray != nullptr && list->maxdist != nullptr), "list.ray or list.maxdist plane is NULL");
    rls_nearest_rays r = {};
    r.rays = rays; r.count = list->count;
    r.origin.x = list->origin.x; r.origin.y = list->origin.y; r.origin.z = list->origin.z;
    r.dir.x = list->dir.x; r.dir.y = list->dir.y; r.dir.z = list->dir.z;
    r.maxdist = list->maxdist; r.ray = list->ray;
    return launch(__func__, ctx, scene, r, found);
}

rls_status rls_nearest_any_opaque(rls_context *ctx, const rls_crgb *opacity, uint32_t count, uint8_t *flags)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(count == 0 || (opacity != nullptr && all3(*opacity)), "opacity or one of its planes is NULL");
    RLS_REQUIRE(count == 0 || flags != nullptr, "flags is NULL");
    if (count == 0) return RLS_OK;
    AnyFlagsIO io = {};
    io.opacity = *opacity; io.flags = flags; io.count = count; io.tiles = tiles_of(count);
    hipLaunchKernelGGL(any_flags_kernel, rlsh::grid_for(ctx, count), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(__func__);
}

} // extern "C"
