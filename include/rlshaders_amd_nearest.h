/*
 * rlshaders_amd_nearest.h -- nearest-hit queries over a triangle mesh on the device (companion library librls_nearest.so).
 *
 * Every queue of rlshaders_amd_trace.h asks the renderer for a nearest hit, and the two walks (rlshaders_amd_walk.h,
 * rlshaders_amd_shadow_walk.h) turned "all hits of a ray" into "the nearest hit in (0, maxdist] of the rays of this
 * rls_walk_rays list".  The calls below answer that query through a BVH, so that a path from an emit to its resolve stays
 * on the device:
 *
 *   rls_walk_begin        -> { rls_nearest_walk_hits -> rls_walk_step }        (found: hit, t, P, N, Ns, object = surface)
 *   rls_shadow_walk_begin -> { rls_nearest_walk_hits -> rls_shadow_walk_step } (found: hit, t, P, index = surface into a table)
 *   a glossy / diffuse queue -> rls_nearest_hits (via = the queue's point plane over sg->P, no maxdist)
 *                            -> rls_trace_route_hits on `bin` -> rls_trace_route_gather from the found planes
 *
 * THE STATEMENT.  The result is a function of the mesh and the ray alone; the tree is not part of it.  All arithmetic is
 * float32, every operation rounded by itself (no contraction), / and sqrt correctly rounded.  a . b = (ax bx + ay by) + az bz;
 * a x b = (ay bz - az by, az bx - ax bz, ax by - ay bx).  min and max below are the compares written out: a NaN operand
 * never replaces the other.
 *
 * A ray: origin o, direction d, reach m (maxdist absent: +inf), a triangle id `skip` (last absent or 0xFFFFFFFF: none).
 *
 * The box interval of triangle i, vertices v0 v1 v2: lo_c / hi_c the smallest / largest of the three c-components;
 *   inv_c = 1 / d_c;  a_c = (lo_c - o_c) * inv_c,  b_c = (hi_c - o_c) * inv_c, swapped where the sign bit of inv_c is set;
 *   tn = 0, tf = +inf;  for c = x, y, z: if (a_c > tn) tn = a_c;  if (b_c < tf) tf = b_c;     the box passes iff !(tn > tf).
 * The triangle test (Moller-Trumbore, two-sided): e1 = v1 - v0, e2 = v2 - v0, p = d x e2, det = e1 . p; no hit unless
 *   det < 0 || det > 0;  r = 1 / det, s = o - v0, u = (s . p) * r, q = s x e1, v = (d . q) * r, tm = (e2 . q) * r;
 *   hit iff u >= 0 && v >= 0 && u + v <= 1 && tm == tm.
 * The distance: t_i = tm; if (tn > t_i) t_i = tn; if (tf < t_i) t_i = tf -- the parameter confined to the ray's interval
 *   inside the triangle's own box.  (The interval does not end at m: confined to [tn, min(tf, m)] a triangle BEHIND the reach
 *   whose box begins in front of it would be reported at t = m; the reach is tested on t_i alone.)
 * Triangle i is a candidate iff i != skip, its box passes, the test hits, t_i > 0 and t_i <= m.  The result is the candidate
 *   of the smallest t_i, among equal t_i the smallest i; none: hit = 0.
 * The confinement is what lets a tree be exact: rounding is monotone, so a box that contains box i has tn <= tn_i under the
 * same arithmetic and a traversal that skips a node whose box fails, or whose tn is greater than m or than the best t so far,
 * never skips a candidate that would have won (the argument is written out where the cull is coded, rls_nearest_device.hpp).
 *
 * A hit reports t, P = o + t d (a product, then a sum), prim = i, surface[i] (0 where the mesh has none), u, v,
 * N = n / sqrt(n . n) with n = e1 x e2 (a division per component), Ns = the same normalisation of
 * ((1 - u - v) n0 + u n1) + v n2 where the mesh has per-vertex normals (w = (1 - u) - v), else N, T = e1 / sqrt(e1 . e1),
 * wo = -d.  Degenerate triangles never hit (det is 0 or NaN).  Nothing is claimed about watertightness; self-hits are
 * avoided by `skip`, never by an epsilon, and no origin is moved.
 *
 * THE TREE is built on the host by rls_nearest_scene_create (csrc_nearest/rls_nearest_bvh.hpp, no HIP needed): an object-median
 * split on the longest axis of the centroid bounds, ties by triangle index, leaves of at most leaf_size triangles, so its
 * depth is at most ceil(log2(nt / leaf_size)) + 1.  One device allocation, one upload.  The traversal keeps a per-lane stack
 * of RLS_NEAREST_STACK node indices in LDS, which is what the triangle limit comes from: nt <= RLS_NEAREST_MAX_TRIANGLES.
 *
 * Neither query synchronises the host: the grid is sized by the host bound, lanes past the device count idle, so both can be
 * recorded into an rls_graph.  Refusals leave "<entry point>: <text>" in rls_last_error; the argument checks run before the
 * context is read.  Link librls_nearest.so (it needs librlshaders_amd.so alone).
 */
#ifndef RLSHADERS_AMD_NEAREST_H
#define RLSHADERS_AMD_NEAREST_H

#include "rlshaders_amd_walk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the per-lane traversal stack, in node indices, and the largest mesh whose tree fits it at leaf_size 1 */
#define RLS_NEAREST_STACK 24
#define RLS_NEAREST_MAX_TRIANGLES ((int64_t)1 << 22)
#define RLS_NEAREST_MAX_LEAF 8
#define RLS_NEAREST_DEFAULT_LEAF 4
/* found.last: skip nothing */
#define RLS_NEAREST_NO_PRIM 0xFFFFFFFFu

/* A mesh, HOST pointers, read by rls_nearest_scene_create and not kept. */
typedef struct rls_nearest_mesh {
    int64_t nv, nt;              /* vertices, triangles; nt == 0 is a scene every ray misses */
    const float *vertices;       /* [nv * 3] xyz per vertex, finite */
    const uint32_t *triangles;   /* [nt * 3] vertex indices < nv */
    const uint32_t *surface;     /* NULL-able [nt]: the surface id of a triangle, default 0 */
    const float *normals;        /* NULL-able [nv * 3]: per-vertex shading normals */
    int leaf_size;               /* 1 .. RLS_NEAREST_MAX_LEAF; 0: RLS_NEAREST_DEFAULT_LEAF.  The result does not depend on it. */
} rls_nearest_mesh;

typedef struct rls_nearest_scene rls_nearest_scene;

/* What a scene holds, for a caller's records. */
typedef struct rls_nearest_scene_info {
    int64_t nv, nt, nodes;
    int leaf_size, depth;        /* depth: the levels of the tree, 0 for an empty scene */
    size_t device_bytes;         /* the one allocation */
} rls_nearest_scene_info;

/* The rays of a query, device planes.  Entry k < min(rays, max(*count, 0)) is traced; nothing at or past that is written. */
typedef struct rls_nearest_rays {
    int64_t rays;                /* a host-side bound: it sizes the grid */
    const int64_t *count;        /* NULL-able, device: one value */
    rls_cvec3 origin;
    const uint32_t *via;         /* NULL-able: entry k starts at origin[via[k]] (a queue's point plane over sg->P) */
    rls_cvec3 dir;
    const float *maxdist;        /* NULL-able: +inf */
    const uint32_t *ray;         /* NULL-able: the entry's id for found.last, default k; ids of one call are distinct */
} rls_nearest_rays;

/* The hits, writable device planes indexed like the rays.  Planes other than hit (and bin) are written only where hit is set. */
typedef struct rls_nearest_found {
    uint8_t *hit;                /* required: 0 / 1 */
    float *t;                    /* required */
    rls_vec3 P, N, Ns, T, wo;    /* each NULL-able (all three planes or none) */
    uint32_t *prim;              /* NULL-able */
    uint32_t *surface;           /* NULL-able: rls_walk_found.object, rls_shadow_walk_found.index */
    float *u, *v;                /* NULL-able */
    uint8_t *bin;                /* NULL-able: bin_of_surface[min(surface, bin_count - 1)] on a hit, 255 on a miss */
    const uint8_t *bin_of_surface; /* read with bin: bin_count entries */
    uint32_t bin_count;          /* >= 1 with bin */
    uint32_t *last;              /* NULL-able, indexed by ray id: read as skip, written with prim on a hit, left on a miss */
} rls_nearest_found;

/* Build the tree of `mesh` on the host and upload it to ctx's device. */
rls_status rls_nearest_scene_create(rls_context *ctx, const rls_nearest_mesh *mesh, rls_nearest_scene **out);
/* Free a scene (NULL: nothing). */
rls_status rls_nearest_scene_destroy(rls_nearest_scene *scene);
rls_status rls_nearest_scene_get_info(const rls_nearest_scene *scene, rls_nearest_scene_info *info);

/* The nearest hit of every ray. */
rls_status rls_nearest_hits(rls_context *ctx, const rls_nearest_scene *scene, const rls_nearest_rays *rays,
                            const rls_nearest_found *found);
/* The same over a walk's list (count, ray, origin, dir, maxdist; found.last indexed by the list's ray plane).  bound: an upper
 * bound on *list->count that sizes the grid, or < 0 for list->capacity. */
rls_status rls_nearest_walk_hits(rls_context *ctx, const rls_nearest_scene *scene, const rls_walk_rays *list, int64_t bound,
                                 const rls_nearest_found *found);

#ifdef __cplusplus
}
#endif

#endif
