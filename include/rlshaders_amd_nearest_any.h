/*
 * rlshaders_amd_nearest_any.h -- any-hit shadow queries over a nearest-hit scene (companion library librls_nearest_any.so).
 *
 * Shadow rays are the most numerous rays the light loops emit, and their way to a visibility plane on the device is the shadow
 * walk over nearest hits (rlshaders_amd_shadow_walk.h over rlshaders_amd_nearest.h): built for translucent surfaces, it pays a
 * full nearest-hit traversal, a step and an empty second round for a ray that ends on an opaque wall.  The calls below answer
 * "is there any candidate in (0, maxdist]" in one launch, and hand the walk only the rays that touched nothing but translucent
 * surfaces:
 *
 *   rls_nearest_any_opaque (the table of rls_trace_*_opacity -> flags)
 *   rls_nearest_any_hits   (state, visibility = base or base * 0, reach = maxdist of the veiled rays, else 0)
 *   rls_shadow_walk_begin on maxdist = reach, base = visibility -> { rls_nearest_walk_hits -> rls_shadow_walk_step }
 *
 * THE STATEMENT.  The ray, the arithmetic, the box interval, the triangle test, the confinement (t_i) and the candidate rule
 * are those of rlshaders_amd_nearest.h, under the names used there: triangle i is a candidate iff i != skip, its box passes,
 * the test hits, t_i > 0 and t_i <= m.  C is the ray's candidate set.
 *
 * A triangle's class: opaque_i = 1 where the caller gives no flag table (found.opaque NULL), else
 *   opaque_i = flags[min(surface_i, opaque_count - 1)] != 0, surface_i = 0 where the mesh has none
 * -- the clamp rule of rls_shadow_walk_found.index, so one table count serves both calls.
 *
 * state of a ray:  1 (blocked) iff some i in C is opaque;  else 2 (veiled) iff C is not empty;  else 0 (clear).
 * These are two existence statements: neither the tree nor the visiting order is part of the result, and NO BLOCKING PRIMITIVE
 * IS REPORTED, because which one a traversal meets first depends on the tree.
 *
 * The derived planes, each NULL-able, indexed by ray id (the rays' `ray` plane, default the entry k -- as found.last is):
 *   visibility_c[id] = b_c * 0.0f where state is 1, else b_c;  b_c = base_c[id], or 1.0f where base is absent.  All three planes
 *     or none; base may alias visibility plane for plane.  b * 0 is exactly the walk's T * (1 - o) at o == 1, so a -0, an
 *     infinite or a NaN base gives what the walk gives.
 *   reach[id] = m where state is 2, else +0.0f: the maxdist plane a second rls_shadow_walk_begin takes.  Begin lists the rays
 *     with maxdist > 0 and a ray that is not listed keeps base, so only the veiled rays are walked, and they start from the
 *     visibility this call wrote.
 * last is read as the skip and NEVER WRITTEN.  Entries at or past min(rays, max(*count, 0)) are not written, in any plane.
 *
 * The traversal is exact for the reason the nearest-hit one is, less the best-t cull (the argument is written where the cull is
 * coded, csrc_nearest/rls_nearest_any.hpp): a lane ends at its first opaque candidate, a translucent one sets a bit.
 *
 * AGAINST THE FULL WALK.  (a) With every triangle opaque (no flags, or every flag set and every opacity entry exactly 1) this
 * call's visibility equals the shadow walk's final T bit for bit, for every ray and any max_steps >= 1: the walk's first query
 * hits iff C is not empty, and its one factor is base * (1 - 1).  (b) With any table the clear and the veiled rays of the
 * two-phase route (this call, begin on reach, the walk) get the full walk's bytes: it is the same walk from the same start.
 * (c) A blocked ray that passes translucent surfaces first gets base * 0 here and (...(base (1 - o1))...) * 0 from the full
 * walk: for a finite base and opacities in [0, 1] both are a zero of base's sign, but the full walk queries again from moved
 * origins and at grazing geometry may not meet the same opaque surface at all.  NO BIT-FOR-BIT CLAIM joins the two there.
 *
 * No call synchronises the host: the grid is sized by the host bound, lanes past the device count idle, so all three can be
 * recorded into an rls_graph.  Refusals leave "<entry point>: <text>" in rls_last_error; the argument checks run before the
 * context is read.  The scene is BORROWED and must be of this build's layout (a scene of another layout is refused).  Link
 * librls_nearest_any.so (it needs librlshaders_amd.so alone; the scene comes from librls_nearest.so).  Any-hit over instanced
 * scenes is not here.
 */
#ifndef RLSHADERS_AMD_NEAREST_ANY_H
#define RLSHADERS_AMD_NEAREST_ANY_H

#include "rlshaders_amd_nearest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* found.state */
#define RLS_NEAREST_ANY_CLEAR 0
#define RLS_NEAREST_ANY_BLOCKED 1
#define RLS_NEAREST_ANY_VEILED 2

/* What a query writes, device planes.  state is indexed like the rays (by entry); base, visibility, reach and last by ray id. */
typedef struct rls_nearest_any_found {
    uint8_t *state;              /* required: 0 / 1 / 2 */
    const uint8_t *opaque;       /* NULL-able: the flag table, opaque_count entries; NULL: every triangle is opaque */
    uint32_t opaque_count;       /* >= 1 with opaque */
    rls_crgb base;               /* all three planes or none (1); read only with visibility */
    rls_rgb visibility;          /* all three planes or none */
    float *reach;                /* NULL-able */
    const uint32_t *last;        /* NULL-able: read as skip, never written */
} rls_nearest_any_found;

/* The state of every ray. */
rls_status rls_nearest_any_hits(rls_context *ctx, const rls_nearest_scene *scene, const rls_nearest_rays *rays,
                                const rls_nearest_any_found *found);
/* The same over a walk's list (count, ray, origin, dir, maxdist), as rls_nearest_walk_hits: state is indexed by entry, the
 * ray-id planes by list->ray[k].  bound: an upper bound on *list->count that sizes the grid, or < 0 for list->capacity. */
rls_status rls_nearest_any_walk_hits(rls_context *ctx, const rls_nearest_scene *scene, const rls_walk_rays *list, int64_t bound,
                                     const rls_nearest_any_found *found);
/* flags[s] = (o_r == 1 && o_g == 1 && o_b == 1) for s < count, IEEE compares (a NaN gives 0): the table rls_trace_*_opacity
 * wrote becomes the flag table. */
rls_status rls_nearest_any_opaque(rls_context *ctx, const rls_crgb *opacity, uint32_t count, uint8_t *flags);

#ifdef __cplusplus
}
#endif

#endif
