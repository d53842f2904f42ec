// trace.hip -- caller-traced rlGgx, rlDisney, rlSss and rlSkin integrators, light loops and whole nodes
// (include/rlshaders_amd_trace.h): the reference's loops cut where it traces, into an emit of every ray and a resolve of what the
// caller traced for them.  The kernels are in the headers included below, by theme and in this order (one anonymous namespace:
// they are parts of this unit, not interfaces); this file holds each verb's kernel selection and, in the EXACT unit, the host
// side: the staging's carve, the argument checks, the emit and resolve steps, the C ABI.
//
// Emit, three steps on the context's stream: the closure's emit kernel (every sample staged, the per-point counts to
// offsets), the scan of the counts, the compaction into the queue.  The sample-ray emits (run_ray_emit) and the light loops'
// (run_shadow_emit) share the staging's carve (staging) and the scan (scan_counts); the probe emits write a dense queue.
// compact_rays is the sample-ray compaction, also of the hit list's diffuse queue.
// Resolve: one launch per verb; a whole node's walks every queue of the node and composes the AOVs in registers.
//
// The whole nodes have a second pair of verbs for the hits of secondary rays (rls_trace_*_bounce_*): the same checks and steps
// (ggx_node_emit, ggx_node_resolve, disney_node_emit, disney_node_resolve, skin_node_emit, skin_node_resolve) with the
// per-point ray state and the kernels that read it -- an emit names each queue once, node_ray_emit / node_shadow_emit picking
// the kernel; rlSkin's has a sixth queue, integrateScatter's light loop at diffuse rays.  That queue and the one of rlSss's
// probe-hit shading are one shape, written once: check_hit_list_queue, set_hit_list_staging, compact_hit_list,
// hit_list_resolve_io.
// The visibility the light loops' resolves read has four verbs of its own at the end of this file (rls_trace_opacity.hpp): the
// opacity each node returns at a shadow ray's hit, and the fold of a ray's hits into its visibility.  After them the five verbs
// that route a traced queue's hits to the nodes (rls_trace_route.hpp): the stable partition by node bin, gather, scatter, fill.
//
// Built twice like the closure units of librlshaders_amd.so (rlshaders_amd/build.py, build_trace_library): RLS_FAST=0
// carries the C ABI, the EXACT emit kernels and the mode-free scan / compact / resolve kernels; RLS_FAST=1 the FAST emit
// kernels behind hidden symbols.
#include <string.h>

#include <initializer_list>

#include "rls_trace_device.hpp"

namespace {

#include "rls_trace_emit.hpp"
#include "rls_trace_shadow_emit.hpp"
#include "rls_trace_probe.hpp"
#include "rls_trace_queue.hpp"
#include "rls_trace_node_resolve.hpp"
#include "rls_trace_hits.hpp"
#include "rls_trace_opacity.hpp"
#include "rls_trace_route.hpp"

// one launch of the rlSss emit or resolve: a workgroup per tile of io.tile_points points, grid-striding past the cap
template <class IO>
rls_status launch_tiles(rls_context *ctx, void (*kernel)(IO), const IO &io, const char *name)
{
    const dim3 grid = rlsh::grid_for(ctx, io.n, io.tile_points);
    hipLaunchKernelGGL(kernel, grid, dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(name, RLS_FAST);
}
// one launch of a kernel that takes a lane per point of io.n
template <class IO>
rls_status launch_points(rls_context *ctx, void (*kernel)(IO), const IO &io, const char *name)
{
    hipLaunchKernelGGL(kernel, rlsh::grid_for(ctx, io.n), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(name, RLS_FAST);
}

} // namespace

// The kernel selection of each verb (rls_internal.hpp, RLS_FLAVOURS), the verbs in the order of their first use: a code object
// holds its kernels in that order (csrc/sss.hip).  RLS_TRACE_G_VERB: a verb whose kernels are <verb>_kernel<G>, chosen by the
// lane group g; RLS_TRACE_TILE_VERB, RLS_TRACE_POINT_VERB: the probe verbs and rlSkin's resolve, one kernel chosen by nothing,
// launched by launch_tiles and launch_points.
#define RLS_TRACE_G_VERB(verb, IO)                                                                            \
    static rls_status launch_##verb(rls_context *ctx, int g, const IO &io, const char *name)                  \
    {                                                                                                         \
        return launch_g(ctx, RLS_G_FAMILY(verb##_kernel), g, io, name);                                       \
    }                                                                                                         \
    RLS_FLAVOURS(verb, IO)
#define RLS_TRACE_TILE_VERB(verb, IO)                                                                         \
    static rls_status launch_##verb(rls_context *ctx, int, const IO &io, const char *name) { return launch_tiles(ctx, verb##_kernel<>, io, name); } \
    RLS_FLAVOURS(verb, IO)
#define RLS_TRACE_POINT_VERB(verb, IO)                                                                        \
    static rls_status launch_##verb(rls_context *ctx, int, const IO &io, const char *name) { return launch_points(ctx, verb##_kernel<>, io, name); } \
    RLS_FLAVOURS(verb, IO)
using GgxShadowEmitIO = ShadowEmitIO<rls_ggx_closure, rls_ggx_shader>;
using DisneyShadowEmitIO = ShadowEmitIO<rls_disney_closure, NoShader>;
RLS_TRACE_G_VERB(ggx_glossy_emit, EmitIO<rls_ggx_closure>)
RLS_TRACE_G_VERB(ggx_refract_emit, EmitIO<rls_ggx_closure>)
RLS_TRACE_G_VERB(disney_diffuse_emit, EmitIO<rls_disney_closure>)
RLS_TRACE_G_VERB(disney_specular_emit, EmitIO<rls_disney_closure>)
RLS_TRACE_G_VERB(ggx_node_glossy_emit, GgxNodeEmitIO)
RLS_TRACE_G_VERB(ggx_node_refract_emit, GgxNodeEmitIO)
RLS_TRACE_G_VERB(ggx_node_diffuse_emit, GgxNodeEmitIO)
RLS_TRACE_G_VERB(disney_node_diffuse_emit, EmitIO<rls_disney_closure>)
RLS_TRACE_G_VERB(disney_node_specular_emit, EmitIO<rls_disney_closure>)
RLS_TRACE_G_VERB(ggx_direct_emit, GgxShadowEmitIO)
RLS_TRACE_G_VERB(disney_direct_emit, DisneyShadowEmitIO)
RLS_TRACE_TILE_VERB(sss_probe_emit, SssEmitIO)
RLS_TRACE_TILE_VERB(sss_scatter_resolve, SssResolveIO)
RLS_TRACE_G_VERB(skin_shadow_emit, SkinShadowEmitIO)
RLS_TRACE_G_VERB(skin_sheen_glossy_emit, SkinGlossyEmitIO)
RLS_TRACE_G_VERB(skin_specular_glossy_emit, SkinGlossyEmitIO)
RLS_TRACE_TILE_VERB(skin_probe_emit, SkinProbeEmitIO)
RLS_TRACE_POINT_VERB(skin_node_resolve, SkinNodeResolveIO)
RLS_TRACE_TILE_VERB(sss_hits_gate, HitGateIO)
RLS_TRACE_G_VERB(sss_hits_emit, HitEmitIO)
RLS_TRACE_G_VERB(ggx_bounce_direct_emit, GgxShadowEmitIO)
RLS_TRACE_G_VERB(ggx_bounce_glossy_emit, GgxBounceEmitIO)
RLS_TRACE_G_VERB(ggx_bounce_refract_emit, GgxBounceEmitIO)
RLS_TRACE_G_VERB(ggx_bounce_diffuse_emit, GgxBounceEmitIO)
RLS_TRACE_G_VERB(disney_bounce_direct_emit, DisneyShadowEmitIO)
RLS_TRACE_G_VERB(disney_bounce_diffuse_emit, DisneyBounceEmitIO)
RLS_TRACE_G_VERB(disney_bounce_specular_emit, DisneyBounceEmitIO)
RLS_TRACE_G_VERB(skin_bounce_shadow_emit, SkinBounceShadowEmitIO)
RLS_TRACE_G_VERB(skin_bounce_sheen_glossy_emit, SkinBounceGlossyEmitIO)
RLS_TRACE_G_VERB(skin_bounce_specular_glossy_emit, SkinBounceGlossyEmitIO)
RLS_TRACE_TILE_VERB(skin_bounce_probe_emit, SkinBounceProbeEmitIO)
RLS_TRACE_G_VERB(skin_diffuse_emit, SkinDiffuseEmitIO)
RLS_TRACE_POINT_VERB(skin_bounce_resolve, SkinBounceResolveIO)

#if !RLS_FAST

namespace {

// The staging of an emit carved out of the caller's scratch, each part 256-byte aligned: `planes` float planes and the tags
// (tag_bytes each) of n * slots_per_point slots, then the scan's tile sums.  The sample-ray emits: dir[3], w[3], 16-bit tags,
// spp slots a point; the light loops: ShadowCompactIO's planes, 32-bit tags, n_lights * 3 * spp slots a point.
constexpr int kRayPlanes = 6;
struct Staging {
    float *f[kShadowPlanes];
    void *tag;
    int64_t *totals;
    int64_t tiles;
    size_t bytes;
};
static_assert(kRayPlanes <= kShadowPlanes, "Staging::f holds the planes of either emit");
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline Staging staging(void *base, int64_t n, int slots_per_point, int planes, size_t tag_bytes)
{
    Staging s = {};
    const size_t slots = (size_t)n * (size_t)slots_per_point;
    char *p = (char *)base;
    size_t off = 0;
    for (int k = 0; k < planes; k++) { s.f[k] = (float *)(p + off); off += align256(slots * sizeof(float)); }
    s.tag = p + off; off += align256(slots * tag_bytes);
    s.tiles = (n + kScanTile - 1) / kScanTile;
    s.totals = (int64_t *)(p + off); off += align256((size_t)(s.tiles > 0 ? s.tiles : 1) * sizeof(int64_t));
    s.bytes = off;
    return s;
}
// the staging of a sample-ray emit at spp samples a point, and of a light-loop emit (nwd: the planes of weight_diffuse, rlDisney
// 3; rlGgx 1, its .r; a lobe of rlSkin 0: none, and two segments a light instead of three): a point's slots, the staged planes
inline Staging ray_staging(void *base, int64_t n, int spp) { return staging(base, n, spp, kRayPlanes, sizeof(uint16_t)); }
inline int shadow_slots(int nwd, int nl, int spp) { return nl * (nwd == 0 ? kSkinShadowSegments : kShadowSegments) * spp; }
inline int shadow_planes(int nwd) { return nwd == 0 ? kSkinShadowPlanes : kShadowPlanes; }
inline Staging shadow_staging(void *base, int64_t n, int nwd, int nl, int spp)
{
    return staging(base, n, shadow_slots(nwd, nl, spp), shadow_planes(nwd), sizeof(uint32_t));
}

// The scratch of the hit verbs (rls_hit_queues.scratch), each part 256-byte aligned: the gate's per-ray masks and counts, the
// tile sums of the three scans (one after another on the stream: one block, sized to the longest), the light loop's staging
// over the list (kHitStagePlanes float planes and 32-bit tags of hit_capacity * n_lights * 2 * hit_spp_n^2 slots) and the
// diffuse ray's (dir[3], weight, 16-bit tags of hit_capacity slots).
struct HitScratch {
    uint16_t *mask;
    int64_t *ray_count, *totals;
    float *f[kHitStagePlanes], *df[4];
    uint32_t *tag;
    uint16_t *dtag;
    size_t bytes;
};
inline int64_t scan_tiles(int64_t n) { return (n + kScanTile - 1) / kScanTile; }
inline HitScratch hit_scratch(void *base, int64_t rays, int64_t capacity, int nl, int hit_spp)
{
    HitScratch s = {};
    char *p = (char *)base;
    size_t off = 0;
    auto carve = [&](size_t bytes) { char *at = p + off; off += align256(bytes); return (void *)at; };
    s.mask = (uint16_t *)carve((size_t)rays * sizeof(uint16_t));
    s.ray_count = (int64_t *)carve((size_t)(rays + 1) * sizeof(int64_t));
    s.totals = (int64_t *)carve((size_t)std::max<int64_t>(std::max(scan_tiles(rays), scan_tiles(capacity)), 1) * sizeof(int64_t));
    const size_t slots = (size_t)capacity * (size_t)(nl * kSkinShadowSegments * hit_spp);
    for (int k = 0; k < kHitStagePlanes; k++) s.f[k] = (float *)carve(slots * sizeof(float));
    s.tag = (uint32_t *)carve(slots * sizeof(uint32_t));
    for (int k = 0; k < 4; k++) s.df[k] = (float *)carve((size_t)capacity * sizeof(float));
    s.dtag = (uint16_t *)carve((size_t)capacity * sizeof(uint16_t));
    s.bytes = off;
    return s;
}

// ---- the argument checks, each written once; fn: the name its messages carry --------------------------------------------------
// the ranges of n and spp_n (the scratch-size verbs check no more); what every queue verb opens with, in this order
rls_status check_n(const char *fn, int64_t n) { RLS_REQUIRE_IN(fn, n >= 0, "n < 0"); return RLS_OK; }
rls_status check_spp_n(const char *fn, int spp_n)
{
    RLS_REQUIRE_IN(fn, spp_n >= 1 && spp_n * spp_n <= kMaxSpp, "spp_n must be in [1, 16]");
    return RLS_OK;
}
rls_status check_batch(const char *fn, const rls_context *ctx, int64_t n, int spp_n)
{
    RLS_REQUIRE_IN(fn, ctx != nullptr, "ctx is NULL");
    if (rls_status s = check_n(fn, n)) return s;
    RLS_REQUIRE_IN(fn, n <= (int64_t)UINT32_MAX, "n > 2^32 - 1 (the queue's point index is 32-bit)");
    return check_spp_n(fn, spp_n);
}

// the planes a ray emit needs of its queue (nw: the weight's planes), for n points at spp_n^2 samples
rls_status check_ray_queue(const char *fn, const rls_ray_queue *q, int nw, int64_t n, int spp_n)
{
    RLS_REQUIRE_IN(fn, rlsh::has3(q->dir), "queue.dir plane is NULL");
    RLS_REQUIRE_IN(fn, nw == 1 ? q->weight.r != nullptr : rlsh::has3(q->weight), "queue.weight plane is NULL");
    RLS_REQUIRE_IN(fn, q->capacity >= n * spp_n * spp_n, "queue.capacity < n * spp_n^2");
    RLS_REQUIRE_IN(fn, q->scratch != nullptr && q->scratch_bytes >= ray_staging(nullptr, n, spp_n * spp_n).bytes,
                   "queue.scratch is NULL or smaller than rls_trace_scratch_bytes");
    return RLS_OK;
}

// The resolve side of a ray queue, checked and written into io: its offsets and weight planes (nw), the radiance traced for
// it, the planes it sums into (checked by the caller), the factor on a one-plane queue's sum (read by trace_resolve_kernel
// alone: the node kernels scale by themselves).  missing: the message for a NULL queue or offsets; need: the capacity a node
// resolve requires (0: the queue verbs, which do not check it).
rls_status ray_resolve_io(const char *fn, TraceResolveIO &io, const rls_ray_queue *q, int nw, int64_t n, int64_t need,
                          rls_crgb radiance, rls_rgb out, float scale, const char *missing)
{
    RLS_REQUIRE_IN(fn, q != nullptr && q->offsets != nullptr, missing);
    RLS_REQUIRE_IN(fn, nw == 1 ? q->weight.r != nullptr : rlsh::has3(q->weight), "queue.weight plane is NULL");
    RLS_REQUIRE_IN(fn, need == 0 || q->capacity >= need, "queue.capacity < n * spp_n^2");
    RLS_REQUIRE_IN(fn, radiance.r && radiance.g && radiance.b, "radiance plane is NULL");
    io.offsets = q->offsets;
    io.w[0] = q->weight.r; io.w[1] = q->weight.g; io.w[2] = q->weight.b;
    io.L = radiance; io.out = out; io.scale = scale; io.n = n;
    return RLS_OK;
}
// one ray queue of a node resolve and the AOV it feeds
rls_status node_ray_io(const char *fn, TraceResolveIO &io, const rls_ray_queue *q, int nw, int64_t n, int spp_n, rls_crgb radiance,
                       rls_rgb aov, float scale = 1.0f)
{
    return ray_resolve_io(fn, io, q, nw, n, n * spp_n * spp_n, radiance, aov, scale, "queue.offsets is NULL");
}

// the planes both sides of a light loop need of its queue, and the scratch its emit needs
rls_status check_shadow_queue(const char *fn, const rls_shadow_queue *q, int nwd, int64_t n, int nl, int spp)
{
    RLS_REQUIRE_IN(fn, rlsh::has3(q->dir) && q->maxdist != nullptr, "queue.dir or queue.maxdist plane is NULL");
    if (nwd == 0) RLS_REQUIRE_IN(fn, rlsh::has3(q->weight_specular), "queue.weight_specular plane is NULL");
    else RLS_REQUIRE_IN(fn, rlsh::has3(q->weight_specular) && (nwd == 1 ? q->weight_diffuse.r != nullptr : rlsh::has3(q->weight_diffuse)),
                        "queue.weight_specular or queue.weight_diffuse plane is NULL");
    RLS_REQUIRE_IN(fn, q->kind != nullptr, "queue.kind is NULL");
    if (nwd == 0) RLS_REQUIRE_IN(fn, q->capacity >= n * nl * kSkinShadowSegments * spp, "queue.capacity < n * n_lights * 2 * spp_n^2");
    else RLS_REQUIRE_IN(fn, q->capacity >= n * nl * kShadowSegments * spp, "queue.capacity < n * n_lights * 3 * spp_n^2");
    return RLS_OK;
}
rls_status check_shadow_scratch(const char *fn, const rls_shadow_queue *q, int nwd, int64_t n, int nl, int spp)
{
    RLS_REQUIRE_IN(fn, q->scratch != nullptr && q->scratch_bytes >= shadow_staging(nullptr, n, nwd, nl, spp).bytes,
                   "queue.scratch is NULL or smaller than rls_trace_shadow_scratch_bytes");
    return RLS_OK;
}
// What a light-loop emit of n > 0 points checks after its closure: the lights, copied into its argument struct, then the queue
template <class IO>
rls_status check_shadow_emit(const char *fn, IO &io, const rls_sphere_light *lights, int n_lights, const rls_shadow_queue *q,
                             int nwd, int64_t n, int spp)
{
    if (rls_status s = copy_lights(lights, n_lights, 1, io.lights, &io.nl)) return s;
    if (rls_status s = check_shadow_queue(fn, q, nwd, n, io.nl, spp)) return s;
    return check_shadow_scratch(fn, q, nwd, n, io.nl, spp);
}

// the planes and capacity a probe emit needs of its queue; what a scatter resolve needs of the queue and of the caller's hits,
// ahead of the n == 0 return (check_max_hits) and after it
rls_status check_probe_queue(const char *fn, const rls_probe_queue *q, int64_t rays)
{
    RLS_REQUIRE_IN(fn, rlsh::has3(q->origin) && rlsh::has3(q->dir) && q->maxdist != nullptr,
                   "queue.origin, queue.dir or queue.maxdist plane is NULL");
    RLS_REQUIRE_IN(fn, q->capacity >= rays, "queue.capacity < n * spp_n^2");
    return RLS_OK;
}
rls_status check_max_hits(const char *fn, const rls_probe_hits *h)
{
    RLS_REQUIRE_IN(fn, h->max_hits >= 1 && h->max_hits <= RLS_MAX_PROBE_HITS, "hits.max_hits must be in [1, 12]");
    return RLS_OK;
}
rls_status check_probe_hits(const char *fn, const rls_probe_queue *q, const rls_probe_hits *h, int64_t rays)
{
    RLS_REQUIRE_IN(fn, q->capacity >= rays, "queue.capacity < n * spp_n^2");
    RLS_REQUIRE_IN(fn, h->stride >= rays, "hits.stride < n * spp_n^2");
    RLS_REQUIRE_IN(fn, h->count != nullptr && rlsh::has3(h->P) && rlsh::has3(h->N) && h->irradiance.r && h->irradiance.g &&
                   h->irradiance.b, "hits.count, hits.P, hits.N or hits.irradiance plane is NULL");
    return RLS_OK;
}

// The hit-list-shaped light-loop queue (weight_diffuse.r its only weight plane, two segments a light: rlSss's probe-hit shading
// over the hit list, the rlSkin bounce's diffuse_shadow over the points): the planes both sides need of it for n entries;
// planes false: a list of no entries has no rays
rls_status check_hit_list_queue(const char *fn, const rls_shadow_queue *q, bool planes, int64_t n, int nl, int spp)
{
    RLS_REQUIRE_IN(fn, !planes || (rlsh::has3(q->dir) && q->maxdist != nullptr), "queue.dir or queue.maxdist plane is NULL");
    RLS_REQUIRE_IN(fn, !planes || q->weight_diffuse.r != nullptr, "queue.weight_specular or queue.weight_diffuse plane is NULL");
    RLS_REQUIRE_IN(fn, !planes || q->kind != nullptr, "queue.kind is NULL");
    RLS_REQUIRE_IN(fn, q->capacity >= n * nl * kSkinShadowSegments * spp, "queue.capacity < n * n_lights * 2 * spp_n^2");
    return RLS_OK;
}

// What both hit verbs check of their list, loop and queues (emit: the scratch and the staging's limits too)
rls_status check_hit_queues(const char *fn, const rls_hit_queues *hq, int n_lights, int hit_spp_n, int trace_diffuse)
{
    RLS_REQUIRE_IN(fn, hq != nullptr, "queues is NULL");
    RLS_REQUIRE_IN(fn, n_lights >= 0 && n_lights <= RLS_MAX_LIGHTS, "n_lights out of range (RLS_MAX_LIGHTS)");
    RLS_REQUIRE_IN(fn, hit_spp_n >= 1 && hit_spp_n * hit_spp_n <= kMaxSpp, "hit_spp_n must be in [1, 16]");
    RLS_REQUIRE_IN(fn, hq->hit_capacity >= 0, "queues.hit_capacity < 0");
    RLS_REQUIRE_IN(fn, hq->hit_capacity <= (int64_t)UINT32_MAX, "queues.hit_capacity > 2^32 - 1 (the queue's point index is 32-bit)");
    RLS_REQUIRE_IN(fn, hq->hit_count != nullptr && (hq->hit_capacity == 0 || hq->hit_element != nullptr),
                   "queues.hit_count or queues.hit_element is NULL");
    const bool planes = hq->hit_capacity > 0;                    // (a list of no entries has no rays: offsets[0] alone)
    if (n_lights > 0) {
        RLS_REQUIRE_IN(fn, hq->shadow.offsets != nullptr, "queue or queue.offsets is NULL");
        if (rls_status s = check_hit_list_queue(fn, &hq->shadow, planes, hq->hit_capacity, n_lights, hit_spp_n * hit_spp_n)) return s;
    }
    if (trace_diffuse) {
        const rls_ray_queue &q = hq->diffuse;
        RLS_REQUIRE_IN(fn, q.offsets != nullptr, "queue or queue.offsets is NULL");
        RLS_REQUIRE_IN(fn, !planes || rlsh::has3(q.dir), "queue.dir plane is NULL");
        RLS_REQUIRE_IN(fn, !planes || q.weight.r != nullptr, "queue.weight plane is NULL");
        RLS_REQUIRE_IN(fn, q.capacity >= hq->hit_capacity, "queue.capacity < n * spp_n^2");
    }
    return RLS_OK;
}

// What the node verbs check first: the batch, the queue struct, the light count (check_node_batch); then their shadow queues
// present exactly where there are lights, each node in its own words
rls_status check_node_batch(const char *fn, const rls_context *ctx, int64_t n, int spp_n, int n_lights, bool have_queues)
{
    if (rls_status s = check_batch(fn, ctx, n, spp_n)) return s;
    RLS_REQUIRE_IN(fn, have_queues, "queues is NULL");
    RLS_REQUIRE_IN(fn, n_lights >= 0 && n_lights <= RLS_MAX_LIGHTS, "n_lights out of range (RLS_MAX_LIGHTS)");
    return RLS_OK;
}
rls_status check_node(const char *fn, const rls_context *ctx, int64_t n, int spp_n, int n_lights, bool have_queues,
                      const rls_shadow_queue *const *shadow)
{
    if (rls_status s = check_node_batch(fn, ctx, n, spp_n, n_lights, have_queues)) return s;
    RLS_REQUIRE_IN(fn, n_lights > 0 || *shadow == nullptr, "queues.shadow is set but n_lights is 0");
    RLS_REQUIRE_IN(fn, n_lights == 0 || *shadow != nullptr, "queues.shadow is NULL but n_lights > 0");
    return RLS_OK;
}
// (rlSkin: the lights and the queue struct's members too)
rls_status check_skin_node(const char *fn, const rls_context *ctx, int64_t n, int spp_n, const rls_sphere_light *lights,
                           int n_lights, const rls_skin_node_queues *q)
{
    if (rls_status s = check_node_batch(fn, ctx, n, spp_n, n_lights, q != nullptr)) return s;
    RLS_REQUIRE_IN(fn, n_lights == 0 || lights != nullptr, "lights is NULL");
    RLS_REQUIRE_IN(fn, n_lights > 0 || (q->sheen_shadow == nullptr && q->specular_shadow == nullptr),
                   "queues.sheen_shadow or queues.specular_shadow is set but n_lights is 0");
    RLS_REQUIRE_IN(fn, n_lights == 0 || (q->sheen_shadow != nullptr && q->specular_shadow != nullptr),
                   "queues.sheen_shadow or queues.specular_shadow is NULL but n_lights > 0");
    RLS_REQUIRE_IN(fn, q->sheen_glossy != nullptr && q->specular_glossy != nullptr && q->probes != nullptr,
                   "queues.sheen_glossy, queues.specular_glossy or queues.probes is NULL");
    RLS_REQUIRE_IN(fn, q->sheenFresnel != nullptr && q->specularFresnel != nullptr && q->sssWeight != nullptr,
                   "queues.sheenFresnel, queues.specularFresnel or queues.sssWeight is NULL");
    RLS_REQUIRE_IN(fn, q->sheen_glossy->offsets != nullptr && q->specular_glossy->offsets != nullptr && q->probes->offsets != nullptr &&
                   (n_lights == 0 || (q->sheen_shadow->offsets != nullptr && q->specular_shadow->offsets != nullptr)),
                   "queue.offsets is NULL");
    return RLS_OK;
}

// a node resolve's AOVs: every plane of `aovs` set, sg->out.RGB all set or all NULL
rls_status check_aov_planes(const char *fn, std::initializer_list<rls_rgb> aovs, rls_rgb out)
{
    for (const rls_rgb &aov : aovs) RLS_REQUIRE_IN(fn, rlsh::has3(aov), "NULL AOV plane");
    RLS_REQUIRE_IN(fn, rlsh::has3(out) || (!out.r && !out.g && !out.b), "out planes must be all set or all NULL");
    return RLS_OK;
}

// ---- the steps: unchecked, on the context's stream ------------------------------------------------------------------------------
// the queue of an empty batch: offsets[0] = 0
rls_status empty_queue(rls_context *ctx, int64_t *offsets, const char *name)
{
    hipLaunchKernelGGL(trace_scan_totals_kernel, dim3(1), dim3(rlsh::kBlock), 0, ctx->stream, offsets, (int64_t)0, offsets);
    return rlsh::check_launch(name);
}

// offsets: the per-point counts of an emit scanned in place (exclusive), offsets[n] = the ray count
rls_status scan_counts(rls_context *ctx, int64_t *offsets, int64_t n, int64_t *totals, int64_t tiles)
{
    rls_status s;
    hipLaunchKernelGGL(trace_scan_block_kernel, dim3((unsigned)tiles), dim3(rlsh::kBlock), 0, ctx->stream, offsets, n, totals);
    if ((s = rlsh::check_launch("trace_scan_block_kernel")) != RLS_OK) return s;
    hipLaunchKernelGGL(trace_scan_totals_kernel, dim3(1), dim3(rlsh::kBlock), 0, ctx->stream, totals, tiles, offsets + n);
    if ((s = rlsh::check_launch("trace_scan_totals_kernel")) != RLS_OK) return s;
    hipLaunchKernelGGL(trace_scan_add_kernel, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, offsets, n,
                       (const int64_t *)totals);
    return rlsh::check_launch("trace_scan_add_kernel");
}
// points per compaction tile: as many as tile_slots slots hold, a point's index in its tile being 8 bits
inline int compact_tile_points(int tile_slots, int per_point) { return std::min(tile_slots / per_point, kCompactMaxPoints); }

// the compaction of a ray emit's kept records into its queue, the counts scanned: the staged planes f (dir[3], then nw weight
// planes) and 16-bit tags of n points at spp slots a point
rls_status compact_rays(rls_context *ctx, float *const *f, const uint16_t *tag, const rls_ray_queue *q, int64_t n, int spp, int nw)
{
    TraceCompactIO cio = {};
    for (int k = 0; k < 3; k++) cio.sdir[k] = f[k];
    for (int k = 0; k < nw; k++) cio.sw[k] = f[3 + k];
    cio.tag = tag; cio.offsets = q->offsets; cio.q = *q; cio.n = n; cio.spp = spp;
    cio.tile_points = compact_tile_points(kCompactSlots, spp);
    const dim3 cgrid = rlsh::grid_for(ctx, n, cio.tile_points);
    if (nw == 1) hipLaunchKernelGGL(trace_compact_kernel<1>, cgrid, dim3(rlsh::kBlock), 0, ctx->stream, cio);
    else hipLaunchKernelGGL(trace_compact_kernel<3>, cgrid, dim3(rlsh::kBlock), 0, ctx->stream, cio);
    return rlsh::check_launch("trace_compact_kernel");
}

// A ray emit of n > 0 points at `spp` samples a point (a node's untraced refraction: 1) into a checked queue: the staging in
// the queue's scratch, the closure's emit kernel (io: its closure part filled; dispatch, with G for the batch), the scan of the
// per-point counts in place into offsets, the compaction of the kept records into the queue (nw weight planes).  side: the
// per-point side output; name: the entry point.
template <class IO>
rls_status run_ray_emit(rls_context *ctx, int64_t n, IO &io, int spp, uint32_t seed, uint64_t first_index, const rls_ray_queue *q,
                        float *side, int nw, const char *name, rls_status (*dispatch)(rls_context *, int, const IO &, const char *))
{
    const Staging st = ray_staging(q->scratch, n, spp);
    for (int k = 0; k < 3; k++) { io.dir[k] = st.f[k]; io.w[k] = st.f[3 + k]; }
    io.tag = (uint16_t *)st.tag; io.side = side;
    io.count = q->offsets;
    io.n = n; io.spp = spp; io.seed = seed; io.first = first_index;
    if (rls_status s = dispatch(ctx, pick_group(ctx, n, spp), io, name)) return s;
    if (rls_status s = scan_counts(ctx, q->offsets, n, st.totals, st.tiles)) return s;
    return compact_rays(ctx, st.f, io.tag, q, n, spp, nw);
}

// One ray queue of a node emit, named once for the node call and the bounce call.  io: the bounce kernels' argument struct, whose
// base Node is the node kernels'; st: the bounce call's state, copied in ahead of the bounce kernel, or NULL: the node kernel
// on the base.  The rest: run_ray_emit's.
template <class Node, class Bounce>
rls_status node_ray_emit(rls_context *ctx, int64_t n, Bounce &io, const BounceState *st, int spp, uint32_t seed, uint64_t first_index,
                         const rls_ray_queue *q, float *side, int nw, const char *name,
                         rls_status (*node)(rls_context *, int, const Node &, const char *),
                         rls_status (*bounce)(rls_context *, int, const Bounce &, const char *))
{
    if (st) {
        io.st = *st;
        return run_ray_emit(ctx, n, io, spp, seed, first_index, q, side, nw, name, bounce);
    }
    Node &base = io;
    return run_ray_emit(ctx, n, base, spp, seed, first_index, q, side, nw, name, node);
}

// one ray resolve: the sum of io's queue (nw weight planes; one plane: x io.scale) into io.out
rls_status launch_ray_resolve(rls_context *ctx, const TraceResolveIO &io, int nw, const char *name)
{
    const dim3 grid = rlsh::grid_for(ctx, io.n);
    if (nw == 1) hipLaunchKernelGGL(trace_resolve_kernel<1>, grid, dim3(rlsh::kBlock), 0, ctx->stream, io);
    else hipLaunchKernelGGL(trace_resolve_kernel<3>, grid, dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(name);
}

// the staged diffuse planes of a light-loop emit (rlSkin's has none)
template <class C, class S>
void set_diffuse_staging(ShadowEmitIO<C, S> &io, const Staging &st) { for (int k = 0; k < 3; k++) io.wd[k] = st.f[7 + k]; }
void set_diffuse_staging(SkinShadowEmitIO &, const Staging &) {}

// A light-loop emit of n > 0 points into a checked queue, run_ray_emit's steps: io has its closure part filled and the lights
// copied in (check_shadow_emit).
template <class IO>
rls_status run_shadow_emit(rls_context *ctx, int64_t n, IO &io, int spp_n, uint32_t seed, uint64_t first_index,
                           const rls_shadow_queue *q, int nwd, const char *name,
                           rls_status (*dispatch)(rls_context *, int, const IO &, const char *))
{
    const int spp = spp_n * spp_n, slots = shadow_slots(nwd, io.nl, spp);
    const Staging st = shadow_staging(q->scratch, n, nwd, io.nl, spp);
    for (int k = 0; k < 3; k++) { io.dir[k] = st.f[k]; io.ws[k] = st.f[4 + k]; }
    set_diffuse_staging(io, st);
    io.maxdist = st.f[3]; io.tag = (uint32_t *)st.tag;
    io.count = q->offsets;
    set_loop(io, n, spp_n, seed, first_index);
    if (rls_status s = dispatch(ctx, pick_group(ctx, n, spp), io, name)) return s;
    if (rls_status s = scan_counts(ctx, q->offsets, n, st.totals, st.tiles)) return s;

    ShadowCompactIO cio = {};
    for (int k = 0; k < shadow_planes(nwd); k++) cio.src[k] = st.f[k];
    cio.tag = io.tag; cio.offsets = q->offsets; cio.q = *q; cio.n = n; cio.spp = spp; cio.slots = slots;
    cio.tile_points = compact_tile_points(kShadowMaxSlots, slots);
    const dim3 cgrid = rlsh::grid_for(ctx, n, cio.tile_points);
    if (nwd == 0) hipLaunchKernelGGL(shadow_compact_kernel<0>, cgrid, dim3(rlsh::kBlock), 0, ctx->stream, cio);
    else if (nwd == 1) hipLaunchKernelGGL(shadow_compact_kernel<1>, cgrid, dim3(rlsh::kBlock), 0, ctx->stream, cio);
    else hipLaunchKernelGGL(shadow_compact_kernel<3>, cgrid, dim3(rlsh::kBlock), 0, ctx->stream, cio);
    return rlsh::check_launch("shadow_compact_kernel");
}
// a node emit's light-loop queue, as node_ray_emit (rlGgx, rlDisney: one struct serves both kernels)
template <class Node, class Bounce>
rls_status node_shadow_emit(rls_context *ctx, int64_t n, Bounce &io, const BounceState *st, int spp_n, uint32_t seed,
                            uint64_t first_index, const rls_shadow_queue *q, int nwd, const char *name,
                            rls_status (*node)(rls_context *, int, const Node &, const char *),
                            rls_status (*bounce)(rls_context *, int, const Bounce &, const char *))
{
    if (st) {
        io.st = *st;
        return run_shadow_emit(ctx, n, io, spp_n, seed, first_index, q, nwd, name, bounce);
    }
    Node &base = io;
    return run_shadow_emit(ctx, n, base, spp_n, seed, first_index, q, nwd, name, node);
}

// The hit-list-shaped queue's emit and compaction.  f: its kHitStagePlanes staged planes -- dir[3], maxdist, weight_diffuse.r --
// of n entries at nl * 2 * spp slots an entry; tag: their 32-bit tags; count: the queue's offsets (NULL: no light loop)
template <class IO>
void set_hit_list_staging(IO &io, float *const *f, uint32_t *tag, int64_t *count)
{
    for (int k = 0; k < 3; k++) io.dir[k] = f[k];
    io.maxdist = f[3]; io.wd[0] = f[4]; io.tag = tag; io.count = count;
}
// totals: scan_tiles(n) tile sums
rls_status compact_hit_list(rls_context *ctx, float *const *f, const uint32_t *tag, const rls_shadow_queue *q, int64_t n, int nl,
                            int spp, int64_t *totals)
{
    if (rls_status s = scan_counts(ctx, q->offsets, n, totals, scan_tiles(n))) return s;
    ShadowCompactIO cio = {};
    for (int k = 0; k < 4; k++) cio.src[k] = f[k];
    cio.src[7] = f[4];
    cio.tag = tag; cio.offsets = q->offsets; cio.q = *q; cio.n = n; cio.spp = spp;
    cio.slots = nl * kSkinShadowSegments * spp;
    cio.tile_points = compact_tile_points(kShadowMaxSlots, cio.slots);
    hipLaunchKernelGGL(hits_compact_kernel, rlsh::grid_for(ctx, n, cio.tile_points), dim3(rlsh::kBlock), 0, ctx->stream, cio);
    return rlsh::check_launch("hits_compact_kernel");
}
// its part of a resolve's argument struct: no weight_specular, one plane of weight_diffuse (the lights' radiance, their count,
// 1 / spp and n: the caller's)
void hit_list_resolve_io(ShadowResolveIO &io, const rls_shadow_queue *q, rls_crgb visibility)
{
    io.offsets = q->offsets; io.kind = q->kind; io.vis = visibility;
    for (int k = 0; k < 3; k++) { io.ws[k] = nullptr; io.wd[k] = nullptr; }
    io.wd[0] = q->weight_diffuse.r;
}

// one light-loop resolve: io's queue (nwd planes of weight_diffuse: rlGgx 1, rlDisney 3) into io.dd and io.ds
rls_status launch_shadow_resolve(rls_context *ctx, const ShadowResolveIO &io, int nwd, const char *name)
{
    const dim3 grid = rlsh::grid_for(ctx, io.n);
    if (nwd == 1) hipLaunchKernelGGL(shadow_resolve_kernel<1>, grid, dim3(rlsh::kBlock), 0, ctx->stream, io);
    else hipLaunchKernelGGL(shadow_resolve_kernel<3>, grid, dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(name);
}

// ---- the queue verbs: checks, then steps -------------------------------------------------------------------------------------
// Every sample-ray emit: the argument checks (lobe_ok: the rlDisney lobe, checked after spp_n), the empty queue of n == 0, then
// run_ray_emit.
template <class Closure>
rls_status emit(rls_context *ctx, int64_t n, const Closure *c, int spp_n, uint32_t seed, uint64_t first_index, bool lobe_ok,
                const rls_ray_queue *q, float *side, int nw, const char *name,
                rls_status (*dispatch)(rls_context *, int, const EmitIO<Closure> &, const char *))
{
    if (rls_status s = check_batch(__func__, ctx, n, spp_n)) return s;
    RLS_REQUIRE(lobe_ok, "lobe must be RLS_RAY_DIFFUSE or RLS_RAY_GLOSSY");
    RLS_REQUIRE(q != nullptr && q->offsets != nullptr, "queue or queue.offsets is NULL");
    if (n == 0) return empty_queue(ctx, q->offsets, name);
    if (rls_status s = rlsh::check_closure(__func__, c)) return s;
    if (rls_status s = check_ray_queue(__func__, q, nw, n, spp_n)) return s;
    EmitIO<Closure> io = {};
    io.c = *c;
    return run_ray_emit(ctx, n, io, spp_n * spp_n, seed, first_index, q, side, nw, name, dispatch);
}

rls_status resolve(rls_context *ctx, int64_t n, const rls_ray_queue *q, int spp_n, rls_crgb radiance, rls_rgb out, bool refract)
{
    RLS_LOOP_PROLOGUE(spp_n);                            // (the glossy resolve passes spp_n = 1)
    TraceResolveIO io = {};
    const float scale = refract ? 1.0f / (float)(spp_n * spp_n) : 1.0f;     // AiSamplerGetSampleInvCount, src/rlGgx.h:244
    if (rls_status s = ray_resolve_io(__func__, io, q, refract ? 1 : 3, n, 0, radiance, out, scale,
                                      "queue or queue.offsets is NULL")) return s;
    RLS_REQUIRE(rlsh::has3(out), "NULL output plane");
    return launch_ray_resolve(ctx, io, refract ? 1 : 3, refract ? "rls_trace_ggx_refract_resolve" : "rls_trace_ggx_glossy_resolve");
}

// The light loop's part of a resolve's argument struct (the light-loop resolves and the node resolves): the lights, the queue's
// planes, the visibility, 1 / spp.  n_lights >= 1.
rls_status shadow_resolve_io(const char *name, ShadowResolveIO &io, int64_t n, int nwd, const rls_sphere_light *lights,
                             int n_lights, int spp_n, const rls_shadow_queue *q, rls_crgb visibility)
{
    rls_sphere_light lt[RLS_MAX_LIGHTS];
    if (rls_status s = copy_lights(lights, n_lights, 1, lt, &io.nl)) return s;
    if (rls_status s = check_shadow_queue(name, q, nwd, n, io.nl, spp_n * spp_n)) return s;
    RLS_REQUIRE_IN(name, visibility.r && visibility.g && visibility.b, "visibility plane is NULL");
    for (int l = 0; l < io.nl; l++)
        for (int k = 0; k < 3; k++) io.rad[l][k] = lt[l].radiance[k];
    io.offsets = q->offsets; io.kind = q->kind; io.vis = visibility;
    io.ws[0] = q->weight_specular.r; io.ws[1] = q->weight_specular.g; io.ws[2] = q->weight_specular.b;
    io.wd[0] = q->weight_diffuse.r; io.wd[1] = q->weight_diffuse.g; io.wd[2] = q->weight_diffuse.b;
    io.inv = 1.0f / (float)(spp_n * spp_n);                      // as the loop kernels: 1 / spp
    io.n = n;
    return RLS_OK;
}

// Both light-loop resolves; c, sh: rlGgx's tail (NULL for rlDisney)
rls_status shadow_resolve(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh, bool ggx,
                          const rls_sphere_light *lights, int n_lights, int spp_n, const rls_shadow_queue *q, rls_crgb visibility,
                          rls_rgb direct_diffuse, rls_rgb direct_specular, const char *name)
{
    if (rls_status s = check_batch(name, ctx, n, spp_n)) return s;
    if (n == 0) return RLS_OK;
    RLS_REQUIRE_IN(name, q != nullptr && q->offsets != nullptr, "queue or queue.offsets is NULL");
    ShadowResolveIO io = {};
    if (ggx) {
        RLS_REQUIRE_IN(name, c != nullptr && sh != nullptr, "closure or shader is NULL");
        RLS_REQUIRE_IN(name, rlsh::ok_rgb(sh->KdColor), "colour planes must be all set or all NULL");
        RLS_REQUIRE_IN(name, rlsh::ok_materials(c->materials), "materials.id is set but materials.count is 0");
        io.materials = c->materials; io.sh = *sh;
    }
    if (rls_status s = shadow_resolve_io(name, io, n, ggx ? 1 : 3, lights, n_lights, spp_n, q, visibility)) return s;
    RLS_REQUIRE_IN(name, rlsh::has3(direct_diffuse) && rlsh::has3(direct_specular), "NULL output plane");
    io.dd = direct_diffuse; io.ds = direct_specular;
    return launch_shadow_resolve(ctx, io, ggx ? 1 : 3, name);
}

// RLS_NODE_RESOLVE=separate: the node resolves through the queue verbs' resolve kernels (launch_shadow_resolve; launch_ray_resolve
// per ray queue: its plain sum, x its scale for a one-plane queue, into its AOV plane) and a compose pass (see
// ggx_node_compose_kernel)
bool separate_node_resolve()
{
    const char *e = getenv("RLS_NODE_RESOLVE");
    return e != nullptr && strcmp(e, "separate") == 0;
}

} // namespace

extern "C" {

rls_status rls_trace_scratch_bytes(int64_t n, int spp_n, size_t *bytes)
{
    RLS_REQUIRE(bytes != nullptr, "bytes is NULL");
    if (rls_status s = check_n(__func__, n)) return s;
    if (rls_status s = check_spp_n(__func__, spp_n)) return s;
    *bytes = ray_staging(nullptr, n, spp_n * spp_n).bytes;
    return RLS_OK;
}

rls_status rls_trace_ggx_glossy_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, int spp_n, uint32_t seed,
                                     uint64_t first_index, const rls_ray_queue *q, float *avg_reflect_weight)
{
    return emit(ctx, n, c, spp_n, seed, first_index, true, q, avg_reflect_weight, 3, __func__, dispatch_ggx_glossy_emit);
}

rls_status rls_trace_ggx_refract_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, int spp_n, uint32_t seed,
                                      uint64_t first_index, const rls_ray_queue *q, float *tir_fraction)
{
    return emit(ctx, n, c, spp_n, seed, first_index, true, q, tir_fraction, 1, __func__, dispatch_ggx_refract_emit);
}

rls_status rls_trace_disney_emit(rls_context *ctx, int64_t n, const rls_disney_closure *c, int lobe, int spp_n, uint32_t seed,
                                 uint64_t first_index, const rls_ray_queue *q, float *valid_count)
{
    const bool lobe_ok = lobe == RLS_RAY_DIFFUSE || lobe == RLS_RAY_GLOSSY;
    return emit(ctx, n, c, spp_n, seed, first_index, lobe_ok, q, valid_count, 3, __func__,
                lobe == RLS_RAY_DIFFUSE ? dispatch_disney_diffuse_emit : dispatch_disney_specular_emit);
}

rls_status rls_trace_ggx_glossy_resolve(rls_context *ctx, int64_t n, const rls_ray_queue *q, rls_crgb radiance, rls_rgb sum)
{
    return resolve(ctx, n, q, 1, radiance, sum, false);
}

rls_status rls_trace_ggx_refract_resolve(rls_context *ctx, int64_t n, const rls_ray_queue *q, int spp_n, rls_crgb radiance,
                                         rls_rgb result)
{
    return resolve(ctx, n, q, spp_n, radiance, result, true);
}

rls_status rls_trace_sss_probe_emit(rls_context *ctx, int64_t n, const rls_sss_closure *c, rls_cvec3 P, int spp_n,
                                    uint32_t seed, uint64_t first_index, const rls_probe_queue *q)
{
    if (rls_status s = check_batch(__func__, ctx, n, spp_n)) return s;
    RLS_REQUIRE(q != nullptr && q->offsets != nullptr, "queue or queue.offsets is NULL");
    const int spp = spp_n * spp_n;
    if (n == 0) return empty_queue(ctx, q->offsets, __func__);
    if (rls_status s = rlsh::check_closure(__func__, c, true)) return s;
    RLS_REQUIRE(rlsh::has3(P), "P plane is NULL");
    if (rls_status s = check_probe_queue(__func__, q, n * spp)) return s;
    SssEmitIO io = {};
    io.c = *c; io.P = P; io.q = *q;
    set_loop(io, n, spp_n, seed, first_index);
    io.tile_points = sss_emit_tile_points(spp);
    return dispatch_sss_probe_emit(ctx, 0, io, __func__);
}

rls_status rls_trace_sss_scatter_resolve(rls_context *ctx, int64_t n, const rls_sss_closure *c, rls_cvec3 P, int spp_n,
                                         const rls_probe_queue *q, const rls_probe_hits *h, int use_cavity_fade,
                                         int literal_matrix, rls_rgb result, float *mean_depth)
{
    if (rls_status s = check_batch(__func__, ctx, n, spp_n)) return s;
    RLS_REQUIRE(q != nullptr, "queue is NULL");
    RLS_REQUIRE(h != nullptr, "hits is NULL");
    if (rls_status s = check_max_hits(__func__, h)) return s;
    if (n == 0) return RLS_OK;
    const int spp = spp_n * spp_n;
    if (rls_status s = rlsh::check_closure(__func__, c, true)) return s;
    RLS_REQUIRE(rlsh::has3(P), "P plane is NULL");
    if (rls_status s = check_probe_hits(__func__, q, h, n * spp)) return s;
    RLS_REQUIRE(rlsh::has3(result), "NULL output plane");
    SssResolveIO io = {};
    io.c = *c; io.P = P; io.h = *h; io.result = result; io.depth = mean_depth;
    io.n = n; io.spp = spp; io.tile_points = sss_resolve_tile_points(spp);
    io.cavity = use_cavity_fade != 0; io.literal = literal_matrix != 0;
    return dispatch_sss_scatter_resolve(ctx, 0, io, __func__);
}

rls_status rls_trace_shadow_scratch_bytes(int64_t n, int n_lights, int spp_n, size_t *bytes)
{
    RLS_REQUIRE(bytes != nullptr, "bytes is NULL");
    if (rls_status s = check_n(__func__, n)) return s;
    RLS_REQUIRE(n_lights >= 1 && n_lights <= RLS_MAX_LIGHTS, "n_lights out of range (RLS_MAX_LIGHTS)");
    if (rls_status s = check_spp_n(__func__, spp_n)) return s;
    *bytes = shadow_staging(nullptr, n, 3, n_lights, spp_n * spp_n).bytes;
    return RLS_OK;
}

rls_status rls_trace_ggx_direct_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                     rls_cvec3 P, const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                     uint64_t first_index, const rls_shadow_queue *q)
{
    const char *fn = __func__;
    if (rls_status s = check_batch(fn, ctx, n, spp_n)) return s;
    RLS_REQUIRE(q != nullptr && q->offsets != nullptr, "queue or queue.offsets is NULL");
    if (n == 0) return empty_queue(ctx, q->offsets, fn);
    RLS_REQUIRE(c != nullptr && sh != nullptr, "closure or shader is NULL");
    if (rls_status s = rlsh::check_closure(fn, c, &P, sh)) return s;
    GgxShadowEmitIO io = {};
    io.c = *c; io.sh = *sh; io.P = P;
    if (rls_status s = check_shadow_emit(fn, io, lights, n_lights, q, 1, n, spp_n * spp_n)) return s;
    return run_shadow_emit(ctx, n, io, spp_n, seed, first_index, q, 1, fn, dispatch_ggx_direct_emit);
}

rls_status rls_trace_disney_direct_emit(rls_context *ctx, int64_t n, const rls_disney_closure *c, rls_cvec3 P,
                                        const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                        uint64_t first_index, const rls_shadow_queue *q)
{
    const char *fn = __func__;
    if (rls_status s = check_batch(fn, ctx, n, spp_n)) return s;
    RLS_REQUIRE(q != nullptr && q->offsets != nullptr, "queue or queue.offsets is NULL");
    if (n == 0) return empty_queue(ctx, q->offsets, fn);
    if (rls_status s = rlsh::check_closure(fn, c, &P)) return s;
    DisneyShadowEmitIO io = {};
    io.c = *c; io.P = P;
    if (rls_status s = check_shadow_emit(fn, io, lights, n_lights, q, 3, n, spp_n * spp_n)) return s;
    return run_shadow_emit(ctx, n, io, spp_n, seed, first_index, q, 3, fn, dispatch_disney_direct_emit);
}

rls_status rls_trace_ggx_direct_resolve(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                        const rls_sphere_light *lights, int n_lights, int spp_n, const rls_shadow_queue *q,
                                        rls_crgb visibility, rls_rgb direct_diffuse, rls_rgb direct_specular)
{
    return shadow_resolve(ctx, n, c, sh, true, lights, n_lights, spp_n, q, visibility, direct_diffuse, direct_specular, __func__);
}

rls_status rls_trace_disney_direct_resolve(rls_context *ctx, int64_t n, const rls_sphere_light *lights, int n_lights,
                                           int spp_n, const rls_shadow_queue *q, rls_crgb visibility,
                                           rls_rgb direct_diffuse, rls_rgb direct_specular)
{
    return shadow_resolve(ctx, n, nullptr, nullptr, false, lights, n_lights, spp_n, q, visibility, direct_diffuse,
                          direct_specular, __func__);
}

} // extern "C"

namespace {

// ---- the whole nodes of rlGgx and rlDisney: the node calls (st == NULL: a camera ray at depth 0 at every point) and the bounce
// calls (st: the per-point ray state) are one set of checks and steps each; only the kernels differ ----------------------------
// a bounce call's state, checked and copied into st; planes: n > 0
rls_status check_state(const char *fn, const rls_ray_state *state, const rls_gi_depths *depths, bool planes, BounceState &st)
{
    RLS_REQUIRE_IN(fn, state != nullptr, "state is NULL");
    RLS_REQUIRE_IN(fn, depths != nullptr, "depths is NULL");
    RLS_REQUIRE_IN(fn, !planes || (state->ray_type && state->Rr && state->Rr_diff && state->Rr_gloss && state->Rr_refr),
                   "state.ray_type, state.Rr, state.Rr_diff, state.Rr_gloss or state.Rr_refr plane is NULL");
    st.s = *state; st.d = *depths;
    return RLS_OK;
}

rls_status ggx_node_emit(const char *fn, rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                         rls_cvec3 P, const rls_sphere_light *lights, int n_lights, int traced, int spp_n, uint32_t seed,
                         uint64_t first_index, const BounceState *st, const rls_ggx_node_queues *q)
{
    RLS_REQUIRE_IN(fn, q->glossy != nullptr && q->refract != nullptr && q->diffuse != nullptr,
                   "queues.glossy, queues.refract or queues.diffuse is NULL");
    const rls_ray_queue *const rq[3] = { q->glossy, q->refract, q->diffuse };
    const int nw[3] = { 3, 1, 1 }, spp = spp_n * spp_n;
    for (int k = 0; k < 3; k++) RLS_REQUIRE_IN(fn, rq[k]->offsets != nullptr, "queue.offsets is NULL");
    GgxShadowEmitIO sio = {};                              // the light loop: rls_trace_ggx_direct_emit's queue
    if (n > 0) {
        RLS_REQUIRE_IN(fn, c != nullptr && sh != nullptr, "closure or shader is NULL");
        if (rls_status s = rlsh::check_closure(fn, c, &P, sh, true)) return s;
        for (int k = 0; k < 3; k++)
            if (rls_status s = check_ray_queue(fn, rq[k], nw[k], n, spp_n)) return s;
        sio.c = *c; sio.sh = *sh; sio.P = P;
    }
    if (n_lights > 0) {                                          // (with this every check has passed: what follows launches)
        RLS_REQUIRE_IN(fn, q->shadow->offsets != nullptr, "queue or queue.offsets is NULL");
        if (n > 0)
            if (rls_status s = check_shadow_emit(fn, sio, lights, n_lights, q->shadow, 1, n, spp)) return s;
    }
    if (n == 0) {
        if (n_lights > 0)
            if (rls_status s = empty_queue(ctx, q->shadow->offsets, fn)) return s;
        for (int k = 0; k < 3; k++)
            if (rls_status s = empty_queue(ctx, rq[k]->offsets, fn)) return s;
        return RLS_OK;
    }
    GgxBounceEmitIO io = {};
    io.c = *c; io.sh = *sh; io.traced = traced ? 1 : 0;
    if (n_lights > 0)
        if (rls_status s = node_shadow_emit(ctx, n, sio, st, spp_n, seed, first_index, q->shadow, 1, fn, dispatch_ggx_direct_emit,
                                            dispatch_ggx_bounce_direct_emit)) return s;
    if (rls_status s = node_ray_emit(ctx, n, io, st, spp, seed, first_index, q->glossy, nullptr, 3, fn, dispatch_ggx_node_glossy_emit,
                                     dispatch_ggx_bounce_glossy_emit)) return s;
    // the node call's untraced branch is one ray a point: one sample (GgxNodeRefract).  The bounce call (traced = 1) has both
    // branches of integrateRefract in one launch at the call's spp: an untraced point's one ray is its sample 0
    if (rls_status s = node_ray_emit(ctx, n, io, st, traced ? spp : 1, seed, first_index, q->refract, nullptr, 1, fn,
                                     dispatch_ggx_node_refract_emit, dispatch_ggx_bounce_refract_emit)) return s;
    return node_ray_emit(ctx, n, io, st, spp, seed, first_index, q->diffuse, nullptr, 1, fn, dispatch_ggx_node_diffuse_emit,
                         dispatch_ggx_bounce_diffuse_emit);
}

rls_status ggx_node_resolve(const char *fn, rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                            const rls_sphere_light *lights, int n_lights, int traced, int spp_n, const BounceState *st,
                            const rls_ggx_node_queues *q, const rls_ggx_node_traced *t, const rls_ggx_shade_out *out)
{
    RLS_REQUIRE_IN(fn, q->glossy != nullptr && q->refract != nullptr && q->diffuse != nullptr,
                   "queues.glossy, queues.refract or queues.diffuse is NULL");
    RLS_REQUIRE_IN(fn, t != nullptr && out != nullptr, "traced or out is NULL");
    if (n == 0) return RLS_OK;
    RLS_REQUIRE_IN(fn, c != nullptr && sh != nullptr, "closure or shader is NULL");
    RLS_REQUIRE_IN(fn, rlsh::ok_rgb(c->KsColor) && rlsh::ok_rgb(sh->KdColor) && rlsh::ok_rgb(sh->KtColor),
                   "colour planes must be all set or all NULL");
    RLS_REQUIRE_IN(fn, rlsh::ok_materials(c->materials), "materials.id is set but materials.count is 0");
    if (rls_status s = check_aov_planes(fn, { out->direct_diffuse, out->direct_specular, out->refraction, out->indirect_diffuse,
                                              out->indirect_specular }, out->out)) return s;
    GgxNodeResolveIO io = {};
    if (n_lights > 0)
        if (rls_status s = shadow_resolve_io(fn, io.s, n, 1, lights, n_lights, spp_n, q->shadow, t->visibility)) return s;
    io.s.materials = c->materials; io.s.sh = *sh; io.s.n = n;
    io.s.dd = out->direct_diffuse; io.s.ds = out->direct_specular;
    io.inv = 1.0f / (float)(spp_n * spp_n);                      // as the loop kernels: 1 / spp
    if (rls_status s = node_ray_io(fn, io.glossy, q->glossy, 3, n, spp_n, t->glossy, out->indirect_specular)) return s;
    if (rls_status s = node_ray_io(fn, io.refract, q->refract, 1, n, spp_n, t->refract, out->refraction, traced ? io.inv : 1.0f))
        return s;
    if (rls_status s = node_ray_io(fn, io.diffuse, q->diffuse, 1, n, spp_n, t->diffuse, out->indirect_diffuse, io.inv)) return s;
    io.KsColor = c->KsColor; io.out = out->out; io.traced = traced ? 1 : 0; io.n = n;
    if (st) {
        io.st = *st;
        hipLaunchKernelGGL(ggx_bounce_resolve_kernel, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, io);
        return rlsh::check_launch(fn);
    }
    if (separate_node_resolve()) {
        if (io.s.nl > 0)
            if (rls_status s = launch_shadow_resolve(ctx, io.s, 1, fn)) return s;
        if (rls_status s = launch_ray_resolve(ctx, io.glossy, 3, fn)) return s;
        if (rls_status s = launch_ray_resolve(ctx, io.refract, 1, fn)) return s;
        if (rls_status s = launch_ray_resolve(ctx, io.diffuse, 1, fn)) return s;
        hipLaunchKernelGGL(ggx_node_compose_kernel, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, io);
        return rlsh::check_launch(fn);
    }
    hipLaunchKernelGGL(ggx_node_resolve_kernel, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(fn);
}

rls_status disney_node_emit(const char *fn, rls_context *ctx, int64_t n, const rls_disney_closure *c, rls_cvec3 P,
                            const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed, uint64_t first_index,
                            const BounceState *st, const rls_disney_node_queues *q)
{
    RLS_REQUIRE_IN(fn, q->diffuse != nullptr && q->specular != nullptr, "queues.diffuse or queues.specular is NULL");
    RLS_REQUIRE_IN(fn, q->diffuse->offsets != nullptr && q->specular->offsets != nullptr, "queue.offsets is NULL");
    const int spp = spp_n * spp_n;
    DisneyShadowEmitIO sio = {};                           // the light loop: rls_trace_disney_direct_emit's queue
    if (n > 0) {
        if (rls_status s = rlsh::check_closure(fn, c, &P)) return s;
        if (rls_status s = check_ray_queue(fn, q->diffuse, 3, n, spp_n)) return s;
        if (rls_status s = check_ray_queue(fn, q->specular, 3, n, spp_n)) return s;
        sio.c = *c; sio.P = P;
    }
    if (n_lights > 0) {                                          // (with this every check has passed: what follows launches)
        RLS_REQUIRE_IN(fn, q->shadow->offsets != nullptr, "queue or queue.offsets is NULL");
        if (n > 0)
            if (rls_status s = check_shadow_emit(fn, sio, lights, n_lights, q->shadow, 3, n, spp)) return s;
    }
    if (n == 0) {
        if (n_lights > 0)
            if (rls_status s = empty_queue(ctx, q->shadow->offsets, fn)) return s;
        if (rls_status s = empty_queue(ctx, q->diffuse->offsets, fn)) return s;
        return empty_queue(ctx, q->specular->offsets, fn);
    }
    DisneyBounceEmitIO io = {};
    io.c = *c;
    if (n_lights > 0)
        if (rls_status s = node_shadow_emit(ctx, n, sio, st, spp_n, seed, first_index, q->shadow, 3, fn, dispatch_disney_direct_emit,
                                            dispatch_disney_bounce_direct_emit)) return s;
    if (rls_status s = node_ray_emit(ctx, n, io, st, spp, seed, first_index, q->diffuse, nullptr, 3, fn,
                                     dispatch_disney_node_diffuse_emit, dispatch_disney_bounce_diffuse_emit)) return s;
    return node_ray_emit(ctx, n, io, st, spp, seed, first_index, q->specular, nullptr, 3, fn, dispatch_disney_node_specular_emit,
                         dispatch_disney_bounce_specular_emit);
}

// sc: the bounce call's closure and scales (its materials index alone is read), checked by the caller
rls_status disney_node_resolve(const char *fn, rls_context *ctx, int64_t n, const rls_sphere_light *lights, int n_lights,
                               int spp_n, const BounceState *st, const rls_disney_closure *c, rls_param diffuse_scale,
                               rls_param specular_scale, const rls_disney_node_queues *q, const rls_disney_node_traced *t,
                               const rls_disney_shade_out *out)
{
    RLS_REQUIRE_IN(fn, q->diffuse != nullptr && q->specular != nullptr, "queues.diffuse or queues.specular is NULL");
    RLS_REQUIRE_IN(fn, t != nullptr && out != nullptr, "traced or out is NULL");
    if (n == 0) return RLS_OK;
    if (st) {
        RLS_REQUIRE_IN(fn, c != nullptr, "closure is NULL");
        RLS_REQUIRE_IN(fn, rlsh::ok_materials(c->materials), "materials.id is set but materials.count is 0");
    }
    if (rls_status s = check_aov_planes(fn, { out->direct_diffuse, out->direct_specular, out->indirect_diffuse,
                                              out->indirect_specular }, out->out)) return s;
    DisneyNodeResolveIO io = {};
    if (n_lights > 0)
        if (rls_status s = shadow_resolve_io(fn, io.s, n, 3, lights, n_lights, spp_n, q->shadow, t->visibility)) return s;
    io.s.n = n; io.s.dd = out->direct_diffuse; io.s.ds = out->direct_specular;
    if (rls_status s = node_ray_io(fn, io.diffuse, q->diffuse, 3, n, spp_n, t->diffuse, out->indirect_diffuse)) return s;
    if (rls_status s = node_ray_io(fn, io.specular, q->specular, 3, n, spp_n, t->specular, out->indirect_specular)) return s;
    io.out = out->out; io.n = n;
    io.inv = 1.0f / (float)(spp_n * spp_n);
    if (st) {
        io.st = *st; io.materials = c->materials; io.diffuse_scale = diffuse_scale; io.specular_scale = specular_scale;
        hipLaunchKernelGGL(disney_bounce_resolve_kernel, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, io);
        return rlsh::check_launch(fn);
    }
    if (separate_node_resolve()) {
        if (io.s.nl > 0)
            if (rls_status s = launch_shadow_resolve(ctx, io.s, 3, fn)) return s;
        if (rls_status s = launch_ray_resolve(ctx, io.diffuse, 3, fn)) return s;
        if (rls_status s = launch_ray_resolve(ctx, io.specular, 3, fn)) return s;
        hipLaunchKernelGGL(disney_node_compose_kernel, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, io);
        return rlsh::check_launch(fn);
    }
    hipLaunchKernelGGL(disney_node_resolve_kernel, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(fn);
}

// ---- rlSkin's whole node: the node calls (st == NULL) and the bounce calls (st: the per-point ray state; dq: the queue of
// integrateScatter's light loop at diffuse rays' points, NULL without lights) ------------------------------------------------
// the bounce calls' queue struct: the node's, and the sixth queue present exactly where there are lights
rls_status check_skin_bounce(const char *fn, const rls_context *ctx, int64_t n, int spp_n, const rls_sphere_light *lights,
                             int n_lights, const rls_skin_bounce_queues *q)
{
    if (rls_status s = check_skin_node(fn, ctx, n, spp_n, lights, n_lights, q ? &q->node : nullptr)) return s;
    RLS_REQUIRE_IN(fn, n_lights > 0 || q->diffuse_shadow == nullptr, "queues.diffuse_shadow is set but n_lights is 0");
    RLS_REQUIRE_IN(fn, n_lights == 0 || q->diffuse_shadow != nullptr, "queues.diffuse_shadow is NULL but n_lights > 0");
    RLS_REQUIRE_IN(fn, n_lights == 0 || q->diffuse_shadow->offsets != nullptr, "queue.offsets is NULL");
    return RLS_OK;
}
// that queue's staging (its planes: check_hit_list_queue): the hit list's planes (dir[3], maxdist, weight_diffuse.r) and 32-bit
// tags of n * n_lights * 2 * spp slots
inline Staging diffuse_shadow_staging(void *base, int64_t n, int nl, int spp)
{
    return staging(base, n, nl * kSkinShadowSegments * spp, kHitStagePlanes, sizeof(uint32_t));
}

rls_status skin_node_emit(const char *fn, rls_context *ctx, int64_t n, const rls_skin_closure *c, rls_cvec3 P,
                          const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed, uint64_t first_index,
                          const BounceState *st, const rls_skin_node_queues *q, const rls_shadow_queue *dq)
{
    const rls_shadow_queue *const sq[2] = { q->sheen_shadow, q->specular_shadow };
    const rls_ray_queue *const gq[2] = { q->sheen_glossy, q->specular_glossy };
    float *const fresnel[2] = { q->sheenFresnel, q->specularFresnel };
    const int spp = spp_n * spp_n;
    if (n == 0) {
        for (int k = 0; k < 2; k++) {
            if (n_lights > 0)
                if (rls_status s = empty_queue(ctx, sq[k]->offsets, fn)) return s;
            if (rls_status s = empty_queue(ctx, gq[k]->offsets, fn)) return s;
        }
        if (rls_status s = empty_queue(ctx, q->probes->offsets, fn)) return s;
        return dq ? empty_queue(ctx, dq->offsets, fn) : RLS_OK;
    }
    if (rls_status s = rlsh::check_closure(fn, c, &P)) return s;
    for (int k = 0; k < 2; k++)
        if (rls_status s = check_ray_queue(fn, gq[k], 3, n, spp_n)) return s;
    if (rls_status s = check_probe_queue(fn, q->probes, n * spp)) return s;
    SkinBounceShadowEmitIO sio = {};
    if (n_lights > 0) {
        for (int k = 0; k < 2; k++) {
            if (rls_status s = check_shadow_queue(fn, sq[k], 0, n, n_lights, spp)) return s;
            if (rls_status s = check_shadow_scratch(fn, sq[k], 0, n, n_lights, spp)) return s;
        }
        if (dq) {
            if (rls_status s = check_hit_list_queue(fn, dq, true, n, n_lights, spp)) return s;
            RLS_REQUIRE_IN(fn, dq->scratch != nullptr && dq->scratch_bytes >= diffuse_shadow_staging(nullptr, n, n_lights, spp).bytes,
                           "queue.scratch is NULL or smaller than rls_trace_shadow_scratch_bytes");
        }
        if (rls_status s = copy_lights(lights, n_lights, 1, sio.lights, &sio.nl)) return s;
        sio.c = *c; sio.P = P; sio.fcnt = q->sssWeight;
    }
    // per lobe: the light loop, which leaves its Fresnel (sum, count) in (the lobe's Fresnel plane, sssWeight); integrateGlossy,
    // which folds on from there and writes the lobe's hand-down into its Fresnel plane
    for (int k = 0; k < 2; k++) {
        if (n_lights > 0) {
            sio.lobe = k; sio.fsum = fresnel[k];
            if (rls_status s = node_shadow_emit(ctx, n, sio, st, spp_n, seed, first_index, sq[k], 0, fn, dispatch_skin_shadow_emit,
                                                dispatch_skin_bounce_shadow_emit)) return s;
        }
        SkinBounceGlossyEmitIO io = {};
        io.c = *c;
        if (n_lights > 0) { io.fsum = fresnel[k]; io.fcnt = q->sssWeight; }
        if (rls_status s = node_ray_emit(ctx, n, io, st, spp, seed, first_index, gq[k], fresnel[k], 3, fn,
                                         k == 0 ? dispatch_skin_sheen_glossy_emit : dispatch_skin_specular_glossy_emit,
                                         k == 0 ? dispatch_skin_bounce_sheen_glossy_emit : dispatch_skin_bounce_specular_glossy_emit))
            return s;
    }
    // integrateScatter's probe rays; sssWeight from the two hand-downs
    SkinBounceProbeEmitIO io = {};
    io.c = *c; io.P = P; io.q = *q->probes;
    io.sheenFresnel = q->sheenFresnel; io.specularFresnel = q->specularFresnel; io.sssWeight = q->sssWeight;
    set_loop(io, n, spp_n, seed, first_index);
    io.tile_points = sss_emit_tile_points(spp);
    if (!st) return dispatch_skin_probe_emit(ctx, 0, io, fn);
    io.st = *st;
    if (rls_status s = dispatch_skin_bounce_probe_emit(ctx, 0, io, fn)) return s;
    if (!dq) return RLS_OK;
    // integrateScatter's light loop at the diffuse rays' points, last: it reads the sssWeight the probe emit has just written.
    // Its streams are the lobes' light loops' at another seed.
    SkinDiffuseEmitIO dio = {};
    dio.wo = c->wo; dio.N = c->N; dio.T = c->T; dio.P = P; dio.sssWeight = q->sssWeight;
    for (int l = 0; l < sio.nl; l++) dio.lights[l] = sio.lights[l];
    dio.nl = sio.nl; dio.st = *st;
    const Staging sg = diffuse_shadow_staging(dq->scratch, n, dio.nl, spp);
    set_hit_list_staging(dio, sg.f, (uint32_t *)sg.tag, dq->offsets);
    set_loop(dio, n, spp_n, seed ^ RLS_SKIN_DIFFUSE_SEED, first_index);
    if (rls_status s = dispatch_skin_diffuse_emit(ctx, pick_group(ctx, n, spp), dio, fn)) return s;
    return compact_hit_list(ctx, sg.f, dio.tag, dq, n, dio.nl, spp, sg.totals);
}

// t, out: not NULL (the callers' check); dvis: the visibility traced for dq's rays
rls_status skin_node_resolve(const char *fn, rls_context *ctx, int64_t n, const rls_skin_closure *c, rls_cvec3 P,
                             const rls_sphere_light *lights, int n_lights, int use_cavity_fade, int literal_matrix, int spp_n,
                             const BounceState *st, const rls_skin_node_queues *q, const rls_shadow_queue *dq,
                             const rls_skin_node_traced *t, rls_crgb dvis, const rls_skin_integrate_out *out)
{
    RLS_REQUIRE_IN(fn, t->hits != nullptr, "traced.hits is NULL");
    if (rls_status s = check_max_hits(fn, t->hits)) return s;
    if (n == 0) return RLS_OK;
    const int spp = spp_n * spp_n;
    if (rls_status s = rlsh::check_closure(fn, c, &P)) return s;
    if (rls_status s = check_aov_planes(fn, { out->sheen, out->specular, out->sss }, out->out)) return s;
    SkinBounceResolveIO io = {};
    if (n_lights > 0) {
        if (rls_status s = shadow_resolve_io(fn, io.sheen_s, n, 0, lights, n_lights, spp_n, q->sheen_shadow, t->sheen_visibility))
            return s;
        if (rls_status s = shadow_resolve_io(fn, io.spec_s, n, 0, lights, n_lights, spp_n, q->specular_shadow, t->specular_visibility))
            return s;
        if (dq) {
            if (rls_status s = check_hit_list_queue(fn, dq, true, n, n_lights, spp)) return s;
            RLS_REQUIRE_IN(fn, dvis.r && dvis.g && dvis.b, "visibility plane is NULL");
            io.dif_s = io.sheen_s;                               // the lights' radiance, their count, 1 / spp
            hit_list_resolve_io(io.dif_s, dq, dvis);
        }
    }
    io.sheen_s.n = n; io.spec_s.n = n; io.dif_s.n = n;
    if (rls_status s = node_ray_io(fn, io.sheen_g, q->sheen_glossy, 3, n, spp_n, t->sheen_glossy, out->sheen)) return s;
    if (rls_status s = node_ray_io(fn, io.spec_g, q->specular_glossy, 3, n, spp_n, t->specular_glossy, out->specular)) return s;
    if (rls_status s = check_probe_hits(fn, q->probes, t->hits, n * spp)) return s;
    io.c = *c; io.P = P; io.h = *t->hits; io.o = *out;
    io.sheenFresnel = q->sheenFresnel; io.specularFresnel = q->specularFresnel; io.sssWeight = q->sssWeight;
    io.inv = 1.0f / (float)spp;                                  // as the loop kernels: 1 / spp
    io.spp = spp; io.tile_points = sss_resolve_tile_points(spp);
    io.cavity = use_cavity_fade != 0; io.literal = literal_matrix != 0; io.n = n;
    if (!st) return dispatch_skin_node_resolve(ctx, 0, io, fn);
    io.st = *st;
    return dispatch_skin_bounce_resolve(ctx, 0, io, fn);
}

} // namespace

extern "C" {

rls_status rls_trace_ggx_shade_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                    rls_cvec3 P, const rls_sphere_light *lights, int n_lights, int traced, int spp_n,
                                    uint32_t seed, uint64_t first_index, const rls_ggx_node_queues *q)
{
    if (rls_status s = check_node(__func__, ctx, n, spp_n, n_lights, q != nullptr, q ? &q->shadow : nullptr)) return s;
    return ggx_node_emit(__func__, ctx, n, c, sh, P, lights, n_lights, traced, spp_n, seed, first_index, nullptr, q);
}

rls_status rls_trace_ggx_shade_resolve(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                       const rls_sphere_light *lights, int n_lights, int traced, int spp_n,
                                       const rls_ggx_node_queues *q, const rls_ggx_node_traced *t,
                                       const rls_ggx_shade_out *out)
{
    if (rls_status s = check_node(__func__, ctx, n, spp_n, n_lights, q != nullptr, q ? &q->shadow : nullptr)) return s;
    return ggx_node_resolve(__func__, ctx, n, c, sh, lights, n_lights, traced, spp_n, nullptr, q, t, out);
}

rls_status rls_trace_disney_shade_emit(rls_context *ctx, int64_t n, const rls_disney_closure *c, rls_cvec3 P,
                                       const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                       uint64_t first_index, const rls_disney_node_queues *q)
{
    if (rls_status s = check_node(__func__, ctx, n, spp_n, n_lights, q != nullptr, q ? &q->shadow : nullptr)) return s;
    return disney_node_emit(__func__, ctx, n, c, P, lights, n_lights, spp_n, seed, first_index, nullptr, q);
}

rls_status rls_trace_disney_shade_resolve(rls_context *ctx, int64_t n, const rls_sphere_light *lights, int n_lights,
                                          int spp_n, const rls_disney_node_queues *q, const rls_disney_node_traced *t,
                                          const rls_disney_shade_out *out)
{
    if (rls_status s = check_node(__func__, ctx, n, spp_n, n_lights, q != nullptr, q ? &q->shadow : nullptr)) return s;
    return disney_node_resolve(__func__, ctx, n, lights, n_lights, spp_n, nullptr, nullptr, rls_param{}, rls_param{}, q, t, out);
}

rls_status rls_trace_ggx_bounce_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                     rls_cvec3 P, const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                     uint64_t first_index, const rls_ray_state *state, const rls_gi_depths *depths,
                                     const rls_ggx_node_queues *q)
{
    BounceState st = {};
    if (rls_status s = check_node(__func__, ctx, n, spp_n, n_lights, q != nullptr, q ? &q->shadow : nullptr)) return s;
    if (rls_status s = check_state(__func__, state, depths, n > 0, st)) return s;
    return ggx_node_emit(__func__, ctx, n, c, sh, P, lights, n_lights, 1, spp_n, seed, first_index, &st, q);
}

rls_status rls_trace_ggx_bounce_resolve(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                        const rls_sphere_light *lights, int n_lights, int spp_n, const rls_ray_state *state,
                                        const rls_gi_depths *depths, const rls_ggx_node_queues *q,
                                        const rls_ggx_node_traced *t, const rls_ggx_shade_out *out)
{
    BounceState st = {};
    if (rls_status s = check_node(__func__, ctx, n, spp_n, n_lights, q != nullptr, q ? &q->shadow : nullptr)) return s;
    if (rls_status s = check_state(__func__, state, depths, n > 0, st)) return s;
    return ggx_node_resolve(__func__, ctx, n, c, sh, lights, n_lights, 1, spp_n, &st, q, t, out);
}

rls_status rls_trace_disney_bounce_emit(rls_context *ctx, int64_t n, const rls_disney_closure *c, rls_cvec3 P,
                                        const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                        uint64_t first_index, const rls_ray_state *state, const rls_gi_depths *depths,
                                        const rls_disney_node_queues *q)
{
    BounceState st = {};
    if (rls_status s = check_node(__func__, ctx, n, spp_n, n_lights, q != nullptr, q ? &q->shadow : nullptr)) return s;
    if (rls_status s = check_state(__func__, state, depths, n > 0, st)) return s;
    return disney_node_emit(__func__, ctx, n, c, P, lights, n_lights, spp_n, seed, first_index, &st, q);
}

rls_status rls_trace_disney_bounce_resolve(rls_context *ctx, int64_t n, const rls_disney_closure *c,
                                           rls_param indirectDiffuseScale, rls_param indirectSpecularScale,
                                           const rls_sphere_light *lights, int n_lights, int spp_n,
                                           const rls_ray_state *state, const rls_gi_depths *depths,
                                           const rls_disney_node_queues *q, const rls_disney_node_traced *t,
                                           const rls_disney_shade_out *out)
{
    BounceState st = {};
    if (rls_status s = check_node(__func__, ctx, n, spp_n, n_lights, q != nullptr, q ? &q->shadow : nullptr)) return s;
    if (rls_status s = check_state(__func__, state, depths, n > 0, st)) return s;
    return disney_node_resolve(__func__, ctx, n, lights, n_lights, spp_n, &st, c, indirectDiffuseScale, indirectSpecularScale, q, t,
                               out);
}

rls_status rls_trace_ray_state_advance(rls_context *ctx, int64_t rays, const uint32_t *point, const rls_ray_state *parent,
                                       int ray_type, const rls_ray_state *child)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(rays >= 0, "rays < 0");
    RLS_REQUIRE(parent != nullptr && child != nullptr, "parent or child is NULL");
    RLS_REQUIRE(ray_type >= 0 && ray_type <= 0xFF, "ray_type is not a byte of RLS_RT_* bits");
    if (rays == 0) return RLS_OK;
    RLS_REQUIRE(point != nullptr, "point is NULL");
    for (const rls_ray_state *s : { parent, child })
        RLS_REQUIRE(s->ray_type && s->Rr && s->Rr_diff && s->Rr_gloss && s->Rr_refr,
                    "state.ray_type, state.Rr, state.Rr_diff, state.Rr_gloss or state.Rr_refr plane is NULL");
    StateAdvanceIO io = {};
    io.point = point; io.parent = *parent; io.ray_type = ray_type; io.rays = rays;
    const uint8_t *const planes[5] = { child->ray_type, child->Rr, child->Rr_diff, child->Rr_gloss, child->Rr_refr };
    for (int k = 0; k < 5; k++) io.child[k] = const_cast<uint8_t *>(planes[k]);
    hipLaunchKernelGGL(state_advance_kernel, rlsh::grid_for(ctx, rays), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(__func__);
}

rls_status rls_trace_skin_emit(rls_context *ctx, int64_t n, const rls_skin_closure *c, rls_cvec3 P,
                               const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                               uint64_t first_index, const rls_skin_node_queues *q)
{
    if (rls_status s = check_skin_node(__func__, ctx, n, spp_n, lights, n_lights, q)) return s;
    return skin_node_emit(__func__, ctx, n, c, P, lights, n_lights, spp_n, seed, first_index, nullptr, q, nullptr);
}

rls_status rls_trace_skin_resolve(rls_context *ctx, int64_t n, const rls_skin_closure *c, rls_cvec3 P,
                                  const rls_sphere_light *lights, int n_lights, int use_cavity_fade, int literal_matrix,
                                  int spp_n, const rls_skin_node_queues *q, const rls_skin_node_traced *t,
                                  const rls_skin_integrate_out *out)
{
    if (rls_status s = check_skin_node(__func__, ctx, n, spp_n, lights, n_lights, q)) return s;
    RLS_REQUIRE(t != nullptr && out != nullptr, "traced or out is NULL");
    return skin_node_resolve(__func__, ctx, n, c, P, lights, n_lights, use_cavity_fade, literal_matrix, spp_n, nullptr, q, nullptr,
                             t, rls_crgb{}, out);
}

rls_status rls_trace_skin_bounce_emit(rls_context *ctx, int64_t n, const rls_skin_closure *c, rls_cvec3 P,
                                      const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                      uint64_t first_index, const rls_ray_state *state, const rls_gi_depths *depths,
                                      const rls_skin_bounce_queues *q)
{
    BounceState st = {};
    if (rls_status s = check_skin_bounce(__func__, ctx, n, spp_n, lights, n_lights, q)) return s;
    if (rls_status s = check_state(__func__, state, depths, n > 0, st)) return s;
    return skin_node_emit(__func__, ctx, n, c, P, lights, n_lights, spp_n, seed, first_index, &st, &q->node, q->diffuse_shadow);
}

rls_status rls_trace_skin_bounce_resolve(rls_context *ctx, int64_t n, const rls_skin_closure *c, rls_cvec3 P,
                                         const rls_sphere_light *lights, int n_lights, int use_cavity_fade,
                                         int literal_matrix, int spp_n, const rls_ray_state *state,
                                         const rls_gi_depths *depths, const rls_skin_bounce_queues *q,
                                         const rls_skin_bounce_traced *t, const rls_skin_integrate_out *out)
{
    BounceState st = {};
    if (rls_status s = check_skin_bounce(__func__, ctx, n, spp_n, lights, n_lights, q)) return s;
    if (rls_status s = check_state(__func__, state, depths, n > 0, st)) return s;
    RLS_REQUIRE(t != nullptr && out != nullptr, "traced or out is NULL");
    return skin_node_resolve(__func__, ctx, n, c, P, lights, n_lights, use_cavity_fade, literal_matrix, spp_n, &st, &q->node,
                             q->diffuse_shadow, &t->node, t->diffuse_visibility, out);
}

rls_status rls_trace_sss_hits_scratch_bytes(int64_t n, int spp_n, int max_hits, int64_t hit_capacity, int n_lights,
                                            int hit_spp_n, size_t *bytes)
{
    RLS_REQUIRE(bytes != nullptr, "bytes is NULL");
    if (rls_status s = check_n(__func__, n)) return s;
    if (rls_status s = check_spp_n(__func__, spp_n)) return s;
    RLS_REQUIRE(max_hits >= 1 && max_hits <= RLS_MAX_PROBE_HITS, "hits.max_hits must be in [1, 12]");
    RLS_REQUIRE(hit_capacity >= 0, "queues.hit_capacity < 0");
    RLS_REQUIRE(n_lights >= 0 && n_lights <= RLS_MAX_LIGHTS, "n_lights out of range (RLS_MAX_LIGHTS)");
    RLS_REQUIRE(hit_spp_n >= 1 && hit_spp_n * hit_spp_n <= kMaxSpp, "hit_spp_n must be in [1, 16]");
    *bytes = hit_scratch(nullptr, n * spp_n * spp_n, hit_capacity, n_lights, hit_spp_n * hit_spp_n).bytes;
    return RLS_OK;
}

rls_status rls_trace_sss_hits_emit(rls_context *ctx, int64_t n, const rls_sss_closure *c, rls_cvec3 P, int spp_n,
                                   const rls_probe_queue *q, const rls_probe_hits *h, rls_cvec3 hitT, int use_cavity_fade,
                                   const rls_sphere_light *lights, int n_lights, int hit_spp_n, int trace_diffuse,
                                   uint32_t seed, uint64_t hit_first_index, const rls_hit_queues *hq)
{
    const char *fn = __func__;
    if (rls_status s = check_batch(fn, ctx, n, spp_n)) return s;
    RLS_REQUIRE(q != nullptr, "queue is NULL");
    RLS_REQUIRE(h != nullptr, "hits is NULL");
    if (rls_status s = check_max_hits(fn, h)) return s;
    if (rls_status s = check_hit_queues(fn, hq, n_lights, hit_spp_n, trace_diffuse)) return s;
    const int spp = spp_n * spp_n, hit_spp = hit_spp_n * hit_spp_n;
    const int64_t rays = n * spp, cap = hq->hit_capacity;
    HitEmitIO io = {};
    if (rls_status s = copy_lights(lights, n_lights, 0, io.lights, &io.nl)) return s;
    const HitScratch sc = hit_scratch(hq->scratch, rays, cap, io.nl, hit_spp);
    RLS_REQUIRE(hq->scratch != nullptr && hq->scratch_bytes >= sc.bytes,
                "queues.scratch is NULL or smaller than rls_trace_sss_hits_scratch_bytes");
    RLS_REQUIRE(rlsh::has3(hitT) || rlsh::none3(hitT), "hitT planes must be all set or all NULL");
    if (n > 0) {
        if (rls_status s = rlsh::check_closure(fn, c, true)) return s;
        RLS_REQUIRE(rlsh::has3(P), "P plane is NULL");
        RLS_REQUIRE(q->capacity >= rays, "queue.capacity < n * spp_n^2");
        RLS_REQUIRE(h->stride >= rays, "hits.stride < n * spp_n^2");
        RLS_REQUIRE(h->count != nullptr && rlsh::has3(h->P) && rlsh::has3(h->N), "hits.count, hits.P or hits.N plane is NULL");
        // the list: the gate, the scan of the rays' shaded counts, hit_element and hit_count
        HitGateIO gio = {};
        gio.c = *c; gio.P = P; gio.h = *h; gio.mask = sc.mask; gio.count = sc.ray_count;
        gio.n = n; gio.spp = spp; gio.tile_points = sss_emit_tile_points(spp); gio.cavity = use_cavity_fade != 0;
        if (rls_status s = dispatch_sss_hits_gate(ctx, 0, gio, fn)) return s;
        if (rls_status s = scan_counts(ctx, sc.ray_count, rays, sc.totals, scan_tiles(rays))) return s;
        HitListIO lio = { sc.mask, sc.ray_count, rays, h->stride, cap, hq->hit_element, hq->hit_count };
        hipLaunchKernelGGL(sss_hits_list_kernel, rlsh::grid_for(ctx, rays), dim3(rlsh::kBlock), 0, ctx->stream, lio);
        if (rls_status s = rlsh::check_launch("sss_hits_list_kernel")) return s;
    } else if (rls_status s = empty_queue(ctx, hq->hit_count, fn)) return s;
    const bool shadow = io.nl > 0, diffuse = trace_diffuse != 0;
    if (cap == 0) {
        if (shadow)
            if (rls_status s = empty_queue(ctx, hq->shadow.offsets, fn)) return s;
        return diffuse ? empty_queue(ctx, hq->diffuse.offsets, fn) : RLS_OK;
    }
    if (!shadow && !diffuse) return RLS_OK;
    // the two emits over the list in one kernel, then each queue's scan and compaction
    io.h = *h; io.T = hitT; io.hit_count = hq->hit_count; io.hit_element = hq->hit_element;
    set_hit_list_staging(io, sc.f, sc.tag, shadow ? hq->shadow.offsets : nullptr);
    if (diffuse) {
        for (int k = 0; k < 3; k++) io.ddir[k] = sc.df[k];
        io.dw = sc.df[3]; io.dtag = sc.dtag; io.dcount = hq->diffuse.offsets;
    }
    set_loop(io, cap, hit_spp_n, seed, hit_first_index);
    if (rls_status s = dispatch_sss_hits_emit(ctx, pick_group(ctx, cap, hit_spp), io, fn)) return s;
    if (shadow)
        if (rls_status s = compact_hit_list(ctx, sc.f, sc.tag, &hq->shadow, cap, io.nl, hit_spp, sc.totals)) return s;
    if (diffuse) {
        if (rls_status s = scan_counts(ctx, hq->diffuse.offsets, cap, sc.totals, scan_tiles(cap))) return s;
        return compact_rays(ctx, sc.df, sc.dtag, &hq->diffuse, cap, 1, 1);
    }
    return RLS_OK;
}

rls_status rls_trace_sss_hits_resolve(rls_context *ctx, const rls_probe_hits *h, const rls_sphere_light *lights, int n_lights,
                                      int hit_spp_n, int trace_diffuse, const rls_hit_queues *hq, rls_crgb visibility,
                                      rls_crgb radiance, rls_rgb E)
{
    const char *fn = __func__;
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(h != nullptr, "hits is NULL");
    if (rls_status s = check_max_hits(fn, h)) return s;
    RLS_REQUIRE(h->stride >= 0, "hits.stride < 0");
    if (rls_status s = check_hit_queues(fn, hq, n_lights, hit_spp_n, trace_diffuse)) return s;
    HitResolveIO io = {};
    rls_sphere_light lt[RLS_MAX_LIGHTS];
    if (rls_status s = copy_lights(lights, n_lights, 0, lt, &io.s.nl)) return s;
    RLS_REQUIRE(io.s.nl == 0 || (visibility.r && visibility.g && visibility.b), "visibility plane is NULL");
    RLS_REQUIRE(!trace_diffuse || (radiance.r && radiance.g && radiance.b), "radiance plane is NULL");
    const int64_t elements = (int64_t)h->max_hits * h->stride;
    if (elements == 0) return RLS_OK;
    RLS_REQUIRE(rlsh::has3(E), "NULL output plane");
    hipLaunchKernelGGL(sss_hits_fill_kernel, rlsh::grid_for(ctx, elements), dim3(rlsh::kBlock), 0, ctx->stream, E, elements);
    if (rls_status s = rlsh::check_launch("sss_hits_fill_kernel")) return s;
    if (hq->hit_capacity == 0) return RLS_OK;
    for (int l = 0; l < io.s.nl; l++)
        for (int k = 0; k < 3; k++) io.s.rad[l][k] = lt[l].radiance[k];
    if (io.s.nl > 0) hit_list_resolve_io(io.s, &hq->shadow, visibility);
    io.s.inv = 1.0f / (float)(hit_spp_n * hit_spp_n);                // as the loop kernels: 1 / spp
    io.s.n = hq->hit_capacity;
    io.hit_count = hq->hit_count; io.hit_element = hq->hit_element;
    if (trace_diffuse) { io.doffsets = hq->diffuse.offsets; io.dw = hq->diffuse.weight.r; io.L = radiance; }
    io.E = E; io.n = hq->hit_capacity;
    hipLaunchKernelGGL(sss_hits_resolve_kernel, rlsh::grid_for(ctx, io.n), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(fn);
}

} // extern "C"

// ---- shadow rays' hits: the nodes' opacity and the fold into a visibility (rls_trace_opacity.hpp) ---------------------------
namespace {

// what the three opacity verbs check of their arguments ahead of the n == 0 return (the struct's own members: the caller), and
// after it
rls_status check_opacity(const char *fn, const rls_context *ctx, int64_t n, bool have_params)
{
    RLS_REQUIRE_IN(fn, ctx != nullptr, "ctx is NULL");
    if (rls_status s = check_n(fn, n)) return s;
    RLS_REQUIRE_IN(fn, have_params, "params is NULL");
    return RLS_OK;
}
rls_status check_opacity_params(const char *fn, std::initializer_list<const rls_param_rgb *> colours, const rls_material_index &m)
{
    for (const rls_param_rgb *c : colours) RLS_REQUIRE_IN(fn, rlsh::ok_rgb(*c), "colour planes must be all set or all NULL");
    RLS_REQUIRE_IN(fn, rlsh::ok_materials(m), "materials.id is set but materials.count is 0");
    return RLS_OK;
}
inline bool all_or_none(rls_crgb v) { return (v.r && v.g && v.b) || (!v.r && !v.g && !v.b); }

} // namespace

extern "C" {

rls_status rls_trace_ggx_opacity(rls_context *ctx, int64_t n, const rls_ggx_opacity *p, const uint8_t *ray_type,
                                 rls_rgb out_opacity)
{
    if (rls_status s = check_opacity(__func__, ctx, n, p != nullptr)) return s;
    if (rls_status s = check_opacity_params(__func__, { &p->opacity_color, &p->KtColor }, p->materials)) return s;
    if (n == 0) return RLS_OK;
    RLS_REQUIRE(rlsh::has3(out_opacity), "NULL output plane");
    const GgxOpacityIO io = { *p, ray_type, out_opacity, n };
    return launch_points(ctx, ggx_opacity_kernel, io, __func__);
}

rls_status rls_trace_disney_opacity(rls_context *ctx, int64_t n, const rls_disney_opacity *p, const uint8_t *ray_type,
                                    rls_rgb out_opacity)
{
    if (rls_status s = check_opacity(__func__, ctx, n, p != nullptr)) return s;
    if (rls_status s = check_opacity_params(__func__, { &p->opacity }, p->materials)) return s;
    if (n == 0) return RLS_OK;
    RLS_REQUIRE(rlsh::has3(out_opacity), "NULL output plane");
    const DisneyOpacityIO io = { *p, ray_type, out_opacity, n };
    return launch_points(ctx, disney_opacity_kernel, io, __func__);
}

rls_status rls_trace_skin_opacity(rls_context *ctx, int64_t n, const rls_skin_opacity *p, const uint8_t *ray_type,
                                  rls_crgb incoming, rls_rgb out_opacity)
{
    if (rls_status s = check_opacity(__func__, ctx, n, p != nullptr)) return s;
    if (rls_status s = check_opacity_params(__func__, { &p->opacity_color }, p->materials)) return s;
    RLS_REQUIRE(all_or_none(incoming), "incoming planes must be all set or all NULL");
    if (n == 0) return RLS_OK;
    RLS_REQUIRE(rlsh::has3(out_opacity), "NULL output plane");
    const SkinOpacityIO io = { *p, ray_type, incoming, out_opacity, n };
    return launch_points(ctx, skin_opacity_kernel, io, __func__);
}

rls_status rls_trace_shadow_visibility(rls_context *ctx, int64_t rays, const rls_shadow_hits *h, rls_crgb base,
                                       rls_rgb visibility)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(rays >= 0, "rays < 0");
    RLS_REQUIRE(h != nullptr, "hits is NULL");
    RLS_REQUIRE(h->max_hits >= 1 && h->max_hits <= 255, "hits.max_hits must be in [1, 255]");
    RLS_REQUIRE(h->stride >= rays, "hits.stride < rays");
    RLS_REQUIRE(h->index == nullptr || h->table_count > 0, "hits.index is set but hits.table_count is 0");
    RLS_REQUIRE(all_or_none(base), "base planes must be all set or all NULL");
    if (rays == 0) return RLS_OK;
    RLS_REQUIRE(h->count != nullptr && h->opacity.r && h->opacity.g && h->opacity.b, "hits.count or hits.opacity plane is NULL");
    RLS_REQUIRE(rlsh::has3(visibility), "NULL output plane");
    const ShadowFoldIO io = { *h, base, visibility, rays };
    hipLaunchKernelGGL(shadow_visibility_kernel, rlsh::grid_for(ctx, rays), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(__func__);
}

} // extern "C"

// ---- routing a queue's hits to the nodes (rls_trace_route.hpp) ----------------------------------------------------------------
namespace {

// The scratch of rls_trace_route_hits, each part 256-byte aligned: the bin-major counts of (bins + 1) keys x tiles, scanned in
// place, with the grand total behind them, then the scan's tile sums.
struct RouteScratch {
    int64_t *counts, *totals;
    int64_t tiles, cells;
    size_t bytes;
};
inline RouteScratch route_scratch(void *base, int64_t rays, int bins)
{
    RouteScratch s = {};
    s.tiles = (rays + kRouteTile - 1) / kRouteTile;
    s.cells = (int64_t)(bins + 1) * s.tiles;
    char *p = (char *)base;
    s.counts = (int64_t *)p;
    size_t off = align256((size_t)(s.cells + 1) * sizeof(int64_t));
    s.totals = (int64_t *)(p + off);
    off += align256((size_t)std::max<int64_t>(scan_tiles(s.cells), 1) * sizeof(int64_t));
    s.bytes = off;
    return s;
}
rls_status check_route_size(const char *fn, int64_t rays, int bins)
{
    RLS_REQUIRE_IN(fn, rays >= 0, "rays < 0");
    if (rays > (int64_t)UINT32_MAX) {
        rlsh::set_error("%s: %s", fn, "rays > 2^32 - 1 (order is 32-bit: route in chunks)");
        return RLS_ERR_UNSUPPORTED;
    }
    RLS_REQUIRE_IN(fn, bins >= 1 && bins <= RLS_ROUTE_MAX_BINS, "bins must be in [1, 16]");
    return RLS_OK;
}

// what gather and scatter check of their arguments, ahead of the m == 0 return
rls_status check_route_planes(const char *fn, const rls_context *ctx, int64_t m, const uint32_t *index, const rls_route_planes *p)
{
    RLS_REQUIRE_IN(fn, ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE_IN(fn, m >= 0, "m < 0");
    RLS_REQUIRE_IN(fn, p != nullptr, "planes is NULL");
    RLS_REQUIRE_IN(fn, p->n_w32 >= 0 && p->n_w32 <= RLS_ROUTE_MAX_W32, "planes.n_w32 must be in [0, 24]");
    RLS_REQUIRE_IN(fn, p->n_u8 >= 0 && p->n_u8 <= RLS_ROUTE_MAX_U8, "planes.n_u8 must be in [0, 8]");
    RLS_REQUIRE_IN(fn, p->n_w32 + p->n_u8 > 0, "planes holds no plane");
    for (int k = 0; k < p->n_w32; k++) {
        RLS_REQUIRE_IN(fn, p->src_w32[k] != nullptr && p->dst_w32[k] != nullptr, "planes.src_w32 or planes.dst_w32 plane is NULL");
        RLS_REQUIRE_IN(fn, p->src_w32[k] != p->dst_w32[k], "a plane's dst is its src");
    }
    for (int k = 0; k < p->n_u8; k++) {
        RLS_REQUIRE_IN(fn, p->src_u8[k] != nullptr && p->dst_u8[k] != nullptr, "planes.src_u8 or planes.dst_u8 plane is NULL");
        RLS_REQUIRE_IN(fn, p->src_u8[k] != p->dst_u8[k], "a plane's dst is its src");
    }
    RLS_REQUIRE_IN(fn, m == 0 || index != nullptr, "index is NULL");
    return RLS_OK;
}
rls_status route_move(const char *fn, rls_context *ctx, int64_t m, const uint32_t *index, const rls_route_planes *p, bool gather)
{
    if (rls_status s = check_route_planes(fn, ctx, m, index, p)) return s;
    if (m == 0) return RLS_OK;
    const RouteMoveIO io = { *p, index, m };
    hipLaunchKernelGGL(gather ? route_gather_kernel : route_scatter_kernel, rlsh::grid_for(ctx, m), dim3(rlsh::kBlock), 0,
                       ctx->stream, io);
    return rlsh::check_launch(fn);
}

} // namespace

extern "C" {

rls_status rls_trace_route_scratch_bytes(int64_t rays, int bins, size_t *bytes)
{
    RLS_REQUIRE(bytes != nullptr, "bytes is NULL");
    if (rls_status s = check_route_size(__func__, rays, bins)) return s;
    *bytes = route_scratch(nullptr, rays, bins).bytes;
    return RLS_OK;
}

rls_status rls_trace_route_hits(rls_context *ctx, int64_t rays, const uint8_t *bin, const rls_hit_routes *r)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(r != nullptr, "routes is NULL");
    if (rls_status s = check_route_size(__func__, rays, r->bins)) return s;
    RLS_REQUIRE(r->offsets != nullptr, "routes.offsets is NULL");
    RLS_REQUIRE(rays == 0 || (bin != nullptr && r->order != nullptr), "bin or routes.order is NULL");
    const RouteScratch sc = route_scratch(r->scratch, rays, r->bins);
    RLS_REQUIRE(r->scratch != nullptr && r->scratch_bytes >= sc.bytes,
                "routes.scratch is NULL or smaller than rls_trace_route_scratch_bytes");
    RouteIO io = {};
    io.bin = bin; io.counts = sc.counts; io.offsets = r->offsets; io.order = r->order; io.slot = r->slot;
    io.rays = rays; io.tiles = sc.tiles; io.bins = r->bins;
    if (rays > 0) {
        hipLaunchKernelGGL(route_count_kernel, rlsh::grid_for(ctx, rays, kRouteTile), dim3(rlsh::kBlock), 0, ctx->stream, io);
        if (rls_status s = rlsh::check_launch("route_count_kernel")) return s;
        if (rls_status s = scan_counts(ctx, sc.counts, sc.cells, sc.totals, scan_tiles(sc.cells))) return s;
    }
    hipLaunchKernelGGL(route_place_kernel, rlsh::grid_for(ctx, rays, kRouteTile), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(__func__);
}

rls_status rls_trace_route_gather(rls_context *ctx, int64_t m, const uint32_t *index, const rls_route_planes *p)
{
    return route_move(__func__, ctx, m, index, p, true);
}

rls_status rls_trace_route_scatter(rls_context *ctx, int64_t m, const uint32_t *index, const rls_route_planes *p)
{
    return route_move(__func__, ctx, m, index, p, false);
}

rls_status rls_trace_route_fill(rls_context *ctx, int64_t m, const uint32_t *index, int n_planes, float *const *dst,
                                const float *value)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(m >= 0, "m < 0");
    RLS_REQUIRE(n_planes >= 1 && n_planes <= RLS_ROUTE_MAX_W32, "n_planes must be in [1, 24]");
    RLS_REQUIRE(dst != nullptr && value != nullptr, "dst or value is NULL");
    RouteFillIO io = {};
    for (int k = 0; k < n_planes; k++) {
        RLS_REQUIRE(dst[k] != nullptr, "dst plane is NULL");
        io.dst[k] = dst[k]; io.value[k] = value[k];
    }
    RLS_REQUIRE(m == 0 || index != nullptr, "index is NULL");
    if (m == 0) return RLS_OK;
    io.index = index; io.m = m; io.n_planes = n_planes;
    hipLaunchKernelGGL(route_fill_kernel, rlsh::grid_for(ctx, m), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(__func__);
}

} // extern "C"

#endif // !RLS_FAST
