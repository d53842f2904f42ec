/*
 * rlshaders_amd_shadow_walk.h -- shadow rays walked on the device (companion library librls_shadow_walk.so).
 *
 * Every light-loop and node resolve of rlshaders_amd_trace.h reads a `visibility` plane, and rls_trace_shadow_visibility folds
 * that plane from a finished list of ALL hits of every shadow ray (rls_shadow_hits).  The calls below form the same plane for a
 * renderer that has a NEAREST-hit query and nothing else: they walk every shadow ray from surface to surface, multiply the
 * opacities in as the fold does, and end a ray where nothing more can change it.
 *
 *   rls_trace_*_direct_emit (or a node's / rls_trace_sss_hits_emit's shadow queue)
 *       -> rls_shadow_walk_begin -> { the renderer's nearest hits -> rls_shadow_walk_step } x at most max_steps
 *       -> rls_trace_*_direct_resolve (or the node's resolve, rls_trace_sss_hits_resolve) on the visibility the walk wrote
 *
 * The state of shadow ray j of an rls_shadow_queue:
 *   T       the transmittance, per channel; starts as base_c[j], or 1 when base is absent; lives in the caller's three
 *           `visibility` planes, indexed by queue ray: exactly the planes the resolves read.  The state is the result, valid
 *           after begin and after every step.  base: all three planes or none; it may alias visibility plane for plane.
 *   left    what is left of the ray's reach; starts as the queue's maxdist[j]; lives in the active list (maxdist)
 *   origin  where the next query starts; starts at O[point[j]], or at O[via[point[j]]] where via is given; lives in the list.
 *           O is a caller table: sg->P per point for a light loop's or a node's queue, or the hit planes of rls_probe_hits
 *           for the shadow queue of an rls_hit_queues, whose point plane indexes the hit LIST: via = hit_element then leads to
 *           the hit's element.  The queue's point plane is NULL-able in the queue; here it is required.
 *   steps   the surfaces the ray may still cross; starts as max_steps, in 1 .. 255; lives in the list (trials)
 *
 * rls_shadow_walk_begin.  rays is a host-side upper bound on the number of rays; count, NULL-able, is a device value (for
 * example &offsets[n] of the queue) and the walk covers the rays j < min(rays, max(*count, 0)); rays at or past that are
 * neither written nor listed.  T is written for every ray of the walk; the rays with maxdist > 0 are listed (a NaN is not
 * listed).  A ray that is not listed keeps base.
 *
 * rls_shadow_walk_step takes, per entry k of the list it reads, the renderer's nearest hit in (0, maxdist] from the entry's
 * origin -- hit (0 / 1), t (the distance from that origin), P (sg->P at the hit) -- and the hit's opacity, given as
 * rls_shadow_hits gives it: three per-entry planes, or index[k] into a table of table_count out_opacity entries (entry
 * min(index[k], table_count - 1) is read; e.g. what rls_trace_ggx_opacity wrote for table_count surfaces).  Per entry:
 *   1. no hit: the ray retires.
 *   2. steps -= 1.
 *   3. T_c = T_c * (1 - o_c) per channel, each operation rounded to float32 by itself: the fold's operation, in visit order.
 *   4. left = left - t and origin = hit.P.
 *   5. the ray survives iff steps > 0 and !(left <= 0) and not (T_r == 0 && T_g == 0 && T_b == 0), an IEEE compare: a T of
 *      +-0 in every channel ends the ray -- no further factor changes it but a non-finite one -- and a NaN does not.
 * A ray whose budget of steps runs out keeps the T it has: the surfaces behind its last hit are not folded in.  No clamp: a
 * non-finite or out-of-range opacity propagates exactly as in rls_trace_shadow_visibility.  So for every ray the walk's T is
 * that call's visibility over the hits the ray visited, in order, bit for bit.  Avoiding self-hits is the tracer's matter, as
 * for every ray the library emits; the step budget bounds a tracer that does not avoid them.  There is no threshold cut-off.
 *
 * The active list is the probe walk's, rls_walk_rays of rlshaders_amd_walk.h: a device count, ray[] ascending, origin, dir,
 * maxdist and the steps left (its `trials` plane) compacted by a stable compaction; two lists ping-ponged by the caller, a step
 * reads one and writes the other.  The type is reused, not restated: a renderer that traces both walks' lists has one
 * nearest-hit entry point over one struct and may share the lists' buffers between the walks.  Only the type is shared:
 * librls_shadow_walk.so links neither librls_walk.so nor librls_trace.so.
 *
 * No call but rls_shadow_walk_active synchronises the host: a step's grid is sized by the caller's bound on the active count,
 * lanes past the device count idle, so a whole walk can be recorded into an rls_graph.
 *
 * Scratch, rls_shadow_walk_scratch_bytes(rays), four parts in this order, each rounded up to 256 bytes, with
 * tiles = max(ceil(rays / 256), 1):
 *   state   uint16 [rays]                   an entry's verdict: survives | steps left << 1 (steps up to 255 need 9 bits)
 *   left    float  [rays]                   an entry's new maxdist
 *   counts  int64  [tiles + 1]              the survivors of every 256-entry tile, scanned in place
 *   totals  int64  [ceil(tiles / 2048)]     the scan's tile sums
 * One step's working set: nothing in it outlives a call.
 *
 * Limits: rays <= 2^32 - 1.  All pointers are device pointers owned by the caller.  Link librls_shadow_walk.so (it needs
 * librlshaders_amd.so, which holds the context and error calls).  Every refusal leaves "<entry point>: <text>" in
 * rls_last_error; the argument checks run before the context is read.
 */
#ifndef RLSHADERS_AMD_SHADOW_WALK_H
#define RLSHADERS_AMD_SHADOW_WALK_H

#include "rlshaders_amd_walk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest budget of steps a ray can carry */
#define RLS_SHADOW_WALK_MAX_STEPS 255

/* The renderer's nearest hit of every entry of the list a step reads, indexed like that list. */
typedef struct rls_shadow_walk_found {
    const uint8_t *hit;      /* required: 0 no hit in (0, maxdist], else a hit; the planes below are read only where set */
    const float *t;          /* required: the distance from the entry's origin */
    rls_cvec3 P;             /* required: sg->P at the hit */
    rls_crgb opacity;        /* required: out_opacity per entry (index == NULL), or a table of table_count entries */
    const uint32_t *index;   /* NULL-able: entry k reads table entry min(index[k], table_count - 1) */
    uint32_t table_count;    /* read only with index; >= 1 */
} rls_shadow_walk_found;

/* One walk: what begin fixes and every step reads. */
typedef struct rls_shadow_walk {
    int64_t rays;            /* a host-side upper bound on the queue's rays */
    const int64_t *count;    /* NULL-able, device: the rays are those below min(rays, max(*count, 0)) */
    int max_steps;           /* 1 .. RLS_SHADOW_WALK_MAX_STEPS */
    rls_cvec3 O;             /* the origins' table */
    const int64_t *via;      /* NULL-able: ray j starts at O[via[point[j]]], not O[point[j]] (rls_hit_queues.hit_element) */
    rls_crgb base;           /* all three planes or none */
    rls_rgb visibility;      /* T: 3 planes indexed by queue ray */
    void *scratch;           /* device, >= rls_shadow_walk_scratch_bytes(rays): an opaque block the calls of one walk share */
    size_t scratch_bytes;
} rls_shadow_walk;

/* Device scratch a walk over at most `rays` shadow rays needs. */
rls_status rls_shadow_walk_scratch_bytes(int64_t rays, size_t *bytes);

/* Start the walk w on the shadow queue q (dir, maxdist and point are read): T = base or 1 for every ray, and the rays with
 * maxdist > 0 listed in `out` with max_steps steps. */
rls_status rls_shadow_walk_begin(rls_context *ctx, const rls_shadow_walk *w, const rls_shadow_queue *q, const rls_walk_rays *out);

/* One step: the decision above for every entry of `in` with its nearest hit, T updated, the survivors listed in `out` (not
 * `in`).  bound: an upper bound on *in->count that sizes the grid, or < 0 for in->capacity; entries at or beyond it are not
 * walked. */
rls_status rls_shadow_walk_step(rls_context *ctx, const rls_shadow_walk *w, const rls_walk_rays *in,
                                const rls_shadow_walk_found *found, int64_t bound, const rls_walk_rays *out);

/* The one call that waits: *host_count = *rays->count once the stream has caught up. */
rls_status rls_shadow_walk_active(rls_context *ctx, const rls_walk_rays *rays, int64_t *host_count);

#ifdef __cplusplus
}
#endif

#endif
