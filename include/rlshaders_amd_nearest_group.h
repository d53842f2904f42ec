/*
 * rlshaders_amd_nearest_group.h -- nearest hits over many placed meshes: instanced scenes (companion library
 * librls_nearest_group.so).
 *
 * rlshaders_amd_nearest.h answers the nearest-hit query over ONE triangle mesh.  A GROUP is a list of instances: each a borrowed
 * rls_nearest_scene placed by an affine transform and given a surface base.  The group has a top-level tree over the
 * instances' world boxes, and one launch walks both levels and answers the same query over all of them.  One scene may stand in
 * any number of instances (a thousand copies cost one mesh of memory); moving an instance rigidly is a matrix write and a refit
 * of at most 2^16 boxes on the stream (rls_nearest_group_update), and no triangle record is touched.
 *
 * THE STATEMENT.  The result is a function of the instances, their meshes and the ray alone; neither tree is part of it.  The
 * arithmetic is that of rlshaders_amd_nearest.h: float32, every operation rounded by itself, / and sqrt correctly rounded, min and
 * max the compares written out, a . b = (ax bx + ay by) + az bz, a x b as stated there.
 *
 * A matrix M is 12 floats, row-major 3 x 4.  A POINT maps as x'_c = ((M[c][0] p_x + M[c][1] p_y) + M[c][2] p_z) + M[c][3]; a
 * VECTOR the same way without the last addition; a NORMAL by the transpose of the linear part,
 * n'_c = (M[0][c] n_x + M[1][c] n_y) + M[2][c] n_z.
 *
 * Instance j: a scene (its mesh, under the statement of rlshaders_amd_nearest.h), to_object A_j, to_world B_j, surface_base.  The
 * library never inverts a matrix and never checks that the two are inverses: B_j shapes the world box and T alone, and whatever
 * the two hold the result is the function stated here.
 *
 * The world box W_j.  lo / hi: the mesh's box -- the union of its triangles' boxes, by value the scene's root node box (after a
 * refit a parked triangle contributes the origin).  Corner k = 0 .. 7 takes hi_x where k & 1, hi_y where k & 2, hi_z where k & 4,
 * else lo; the eight are mapped by B_j as points, and Wlo_c / Whi_c is the smallest / largest c-component, folded from corner 0
 * to corner 7.  Each end is then widened: with m_k = max(|lo_k|, |hi_k|) and
 * e_c = ((|B[c][0]| m_x + |B[c][1]| m_y) + |B[c][2]| m_z) + |B[c][3]|, pad_c = e_c * 2^-21, Wlo_c -= pad_c, Whi_c += pad_c.  The
 * pad covers the corner products' own rounding (three products and three sums, each within 2^-24 relative of a value no larger
 * than e_c), so that W_j encloses the exactly transformed box; it is a stated choice, not a measurement, and the exactness of the
 * traversal does not rest on it (below).
 *
 * An instance is PARKED and never hits when any entry of A_j, B_j or W_j is not finite, or its scene is empty.  A parked
 * instance's box in the top tree is the point at the origin.
 *
 * A ray: origin o, direction d, reach m (maxdist absent: +inf), a skip pair (skip_instance, skip_prim) (last absent: none).
 *   The world interval of instance j: the box interval of W_j against (o, inv = 1 / d) as rlshaders_amd_nearest.h states it, from
 *     tn = 0, tf = +inf -> (tnW, tfW).  The instance takes part iff !(tnW > tfW).
 *   The object ray: o' = A_j o as a point, d' = A_j d as a vector, inv'_c = 1 / d'_c.  The parameter t is shared between the two
 *     spaces: d' is not normalised.
 *   Triangle i of instance j: the box interval and the triangle test of rlshaders_amd_nearest.h with o', d', inv', except that the
 *     interval STARTS FROM tn = tnW, tf = tfW instead of 0, +inf; t_i = tm confined to that interval.  It is a candidate iff
 *     (j, i) is not the skip pair, the instance is not parked and takes part, the box passes, the test hits, t_i > 0 and t_i <= m.
 *   The result: the candidate of the smallest t, among equal t the smallest j, among those the smallest i; none: hit = 0.
 * Both trees are exact by the monotonicity argument of rlshaders_amd_nearest.h applied twice: an object node's box contains its
 * triangles' boxes and sees the same o', inv' and the same starting interval; a top node's box contains its W_j and sees the same
 * o, inv; so tn_top <= tnW_j <= tn_i <= t_i, and the culls "box fails", "tn > m" and "tn > best t" (strict: ties are still
 * visited) hold at both levels (written out where they are coded, csrc_nearest/rls_nearest_group.hpp).
 *
 * A hit reports t, P = o + t d on the WORLD ray, prim = i, instance = j, surface = surface_base_j + surface_j[i] in uint32
 * arithmetic (surface_j[i] = 0 where the mesh has none), u, v, N = normalize(A_j^T n) with n = e1 x e2 in object space,
 * Ns = normalize(A_j^T s) with s = ((1 - u - v) n0 + u n1) + v n2 NOT normalised in between, where the mesh has normals, else N,
 * T = normalize(B_j e1) (e1 mapped as a vector), wo = -d, and bin as rlshaders_amd_nearest.h has it, on the based surface id.
 * normalize(a) = a / sqrt(a . a), a division per component.  A MIRRORING instance reports N as A^T n gives it: there is no flip
 * by the sign of a determinant, and a renderer that wants the winding's side corrects it itself.
 *
 * THE TOP TREE is built on the host by rls_nearest_group_create with the builder of rlshaders_amd_nearest.h over the W_j: object
 * median on the longest axis of the centroid bounds, ties by instance index, the larger half on the left, leaves of at most
 * leaf_size instances, so its depth is at most ceil(log2(count / leaf_size)) + 1 and a per-lane top stack of
 * RLS_NEAREST_GROUP_STACK entries (beside the RLS_NEAREST_STACK of the object level) holds it at RLS_NEAREST_GROUP_MAX_INSTANCES.
 *
 * rls_nearest_group_update runs on ctx's stream, in this order: (1) the instances' matrices are rewritten from the two device
 * planes (skipped when both are NULL); (2) every W_j is recomputed from its scene's root box as it is on the device THEN -- an
 * update issued after a moving-mesh update of a member scene (the box-only one or the tree's rebuild) on the same stream picks up
 * the moved mesh --, and the parked flags with it; (3) every top node's box becomes the exact union of what is below it, bottom-up,
 * links untouched.  No host synchronisation, no allocation, no float atomics: it can be recorded into an rls_graph, and a replay
 * reads the planes as they are then.  Every query afterwards returns the bytes a fresh group created with those matrices over
 * those scenes returns; only the cost drifts (a caller whose instances have scattered far creates the group again).
 *
 * Neither query synchronises the host: the grid is sized by the host bound, so both can be recorded into a graph.  A group
 * BORROWS its scenes: they must outlive it (the Python and C++ wrappers hold references).  Refusals leave
 * "<entry point>: <text>" in rls_last_error; the argument checks run before the context is read.  Link librls_nearest_group.so
 * (it needs librlshaders_amd.so alone; the scenes come from librls_nearest.so, which the caller links for them, and both must be
 * of one build: a scene of another layout is refused).
 */
#ifndef RLSHADERS_AMD_NEAREST_GROUP_H
#define RLSHADERS_AMD_NEAREST_GROUP_H

#include "rlshaders_amd_nearest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the per-lane stack of the top level, in node indices, and the largest group whose top tree fits it at leaf_size 1 */
#define RLS_NEAREST_GROUP_STACK 16
#define RLS_NEAREST_GROUP_MAX_INSTANCES ((int64_t)1 << 16)
#define RLS_NEAREST_GROUP_MAX_LEAF 4
#define RLS_NEAREST_GROUP_DEFAULT_LEAF 2
/* found.last_instance: skip nothing */
#define RLS_NEAREST_NO_INSTANCE 0xFFFFFFFFu

/* One instance, HOST memory, read by rls_nearest_group_create; the scene is borrowed, the matrices are copied. */
typedef struct rls_nearest_instance {
    const rls_nearest_scene *scene;
    float to_object[12];         /* A: world -> object, row-major 3 x 4 */
    float to_world[12];          /* B: object -> world */
    uint32_t surface_base;       /* added to the mesh's surface ids */
} rls_nearest_instance;

typedef struct rls_nearest_group rls_nearest_group;

/* What a group holds, for a caller's records. */
typedef struct rls_nearest_group_info {
    int64_t instances, scenes;   /* scenes: the distinct ones */
    int64_t top_nodes;
    int top_depth;               /* the levels of the top tree, 0 for an empty group */
    int leaf_size;
    size_t device_bytes;         /* the one allocation */
    int64_t updates;             /* rls_nearest_group_update calls accepted so far (a graph's replays are not calls) */
} rls_nearest_group_info;

/* The instances' new matrices, DEVICE planes of [instances * 12] floats each: both, or both NULL (the matrices stay). */
typedef struct rls_nearest_group_moves {
    const float *to_object;
    const float *to_world;
    int64_t *parked;             /* NULL-able, device, one value: written with the number of instances parked */
} rls_nearest_group_moves;

/* The hits: rls_nearest_found and the instance of each.  last_instance is required exactly when found.last is given and is
 * indexed by the same ray id: the pair (last_instance, last) is read as the skip and written on a hit. */
typedef struct rls_nearest_group_found {
    rls_nearest_found found;
    uint32_t *instance;          /* NULL-able: written where hit is set */
    uint32_t *last_instance;
} rls_nearest_group_found;

/* Build the top tree over `count` instances (0 .. RLS_NEAREST_GROUP_MAX_INSTANCES; 0: a group every ray misses) on the host and
 * upload it: one device allocation, one upload; the scenes' root boxes are downloaded first (one synchronisation).  leaf_size:
 * 1 .. RLS_NEAREST_GROUP_MAX_LEAF, 0 for the default; the result does not depend on it. */
rls_status rls_nearest_group_create(rls_context *ctx, const rls_nearest_instance *instances, int64_t count, int leaf_size,
                                    rls_nearest_group **out);
/* Free a group (NULL: nothing).  The scenes are not touched. */
rls_status rls_nearest_group_destroy(rls_nearest_group *group);
rls_status rls_nearest_group_get_info(const rls_nearest_group *group, rls_nearest_group_info *info);
/* Move the instances on ctx's stream (above).  No host synchronisation, no allocation. */
rls_status rls_nearest_group_update(rls_context *ctx, rls_nearest_group *group, const rls_nearest_group_moves *moves);

/* The nearest hit of every ray over all instances. */
rls_status rls_nearest_group_hits(rls_context *ctx, const rls_nearest_group *group, const rls_nearest_rays *rays,
                                  const rls_nearest_group_found *found);
/* The same over a walk's list, as rls_nearest_walk_hits. */
rls_status rls_nearest_group_walk_hits(rls_context *ctx, const rls_nearest_group *group, const rls_walk_rays *list, int64_t bound,
                                       const rls_nearest_group_found *found);

/* HOST arrays, each NULL-able; synchronises.  boxes [top_nodes * 6] lo xyz hi xyz; links [top_nodes * 2] first, meta;
 * order [instances]: the instance ids in leaf order; world [instances * 6]: W_j by instance, lo xyz hi xyz; parked [instances]:
 * 0 / 1 by instance. */
rls_status rls_nearest_group_read_tree(rls_context *ctx, const rls_nearest_group *group, float *boxes, uint32_t *links,
                                       uint32_t *order, float *world, uint8_t *parked);

#ifdef __cplusplus
}
#endif

#endif
