/*
 * rlshaders_amd_nearest_refit.h -- moving meshes: refit the tree of a nearest-hit scene on the device (companion library
 * librls_nearest_refit.so).
 *
 * rls_nearest_scene_create (rlshaders_amd_nearest.h) builds a scene's tree on the host and uploads it once.  A mesh that
 * deforms -- a character under a skin shader, every frame -- keeps its triangles and moves its vertices, and a deformer
 * leaves them on the device.  A refit takes them there: it rewrites the scene's triangle records from the new vertices and
 * makes every node box the union of what is below it again, bottom-up.  The topology of the tree stays.
 *
 *   rls_nearest_scene_create -> rls_nearest_refit_create                          (once)
 *   per frame: the deformer -> rls_nearest_refit_update -> rls_nearest_hits / _walk_hits ... on the same stream
 *
 * WHAT A QUERY RETURNS AFTERWARDS.  The statement of rlshaders_amd_nearest.h makes a query's result a function of the mesh
 * and the ray alone; the tree is not part of it, it only has to contain: every node box contains the boxes below it.  The
 * update restores exactly that, so every query after it returns, bit for bit, what a fresh scene made from the new vertices
 * returns.  Only the cost can drift: the splits were chosen for the first mesh (INTEGRATION.md section 6 has measurements).
 *
 * THE UPDATE does four things, on ctx's stream, in this order:
 *   1. every triangle record is rewritten from mesh.vertices through the scene's own index array; a record's triangle id and
 *      its place in leaf order stay;
 *   2. a triangle with a NaN or an infinity in any of its nine coordinates is PARKED: its record holds three vertices at the
 *      origin, so det == 0 (or NaN) in the triangle test and it is never a candidate, and its box is the point at the
 *      origin.  *mesh.parked, where given, is written with the exact number of parked triangles.  Finite vertices are the
 *      caller's duty for a sensible picture; parking makes the contract total: whatever the vertices hold, the scene is
 *      afterwards a scene of finite triangles, the statement holds for it with parked triangles never hitting, and the
 *      traversal's bounds hold;
 *   3. every node's box becomes the exact union of what is below it: a leaf's from its records (the smallest / largest
 *      component over the three vertices of each, by the compares written out), an inner node's from its two children.  A
 *      node's links (its first child or record, its count and split axis) are not touched;
 *   4. mesh.normals, where given, replace the scene's per-vertex normals (a device-to-device copy).
 * Nothing else of the scene is written: the index array, the surface ids and every size stay.
 *
 * A zero bound can differ in SIGN from the one a fresh scene holds (the builder folds the boxes in another order); no
 * result depends on it, and rls_nearest_refit_read_tree's boxes are to be compared by value (the argument is written where
 * the union is coded, csrc_nearest/rls_nearest_refit.hpp).
 *
 * found.last of a query (the triangle a ray stands on) stays valid across an update: triangle ids do not change.
 *
 * rls_nearest_refit_update never synchronises the host and allocates nothing, so it can be recorded into an rls_graph; a
 * replay reads the vertex (and normal) buffers as they are then.  Queries issued on the same stream afterwards see the new
 * mesh; a query running on ANOTHER stream during an update reads a tree in motion, which is the caller's to order.  One
 * scene takes one refit at a time.
 *
 * A refit BORROWS its scene: the scene must outlive it (the Python and C++ wrappers hold a reference).  Refusals leave
 * "<entry point>: <text>" in rls_last_error; the argument checks run before the context is read.  Link
 * librls_nearest_refit.so (it needs librlshaders_amd.so alone; the scene comes from librls_nearest.so, which the caller
 * links for it, and both libraries must be of one build: a scene of another layout is refused).
 */
#ifndef RLSHADERS_AMD_NEAREST_REFIT_H
#define RLSHADERS_AMD_NEAREST_REFIT_H

#include "rlshaders_amd_nearest.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rls_nearest_refit rls_nearest_refit;

/* What a refit holds, for a caller's records. */
typedef struct rls_nearest_refit_info {
    int64_t nv, nt, nodes;       /* the scene's */
    int levels;                  /* = the scene's depth; 0 for an empty scene */
    int has_normals;             /* the scene was made with per-vertex normals */
    size_t device_bytes;         /* the refit's own allocation: the per-level node lists */
    int64_t updates;             /* rls_nearest_refit_update calls accepted so far (a graph's replays are not calls) */
} rls_nearest_refit_info;

/* The moved mesh, DEVICE pointers. */
typedef struct rls_nearest_refit_mesh {
    int64_t nv;                  /* must equal the scene's */
    const float *vertices;       /* [nv * 3] xyz per vertex */
    const float *normals;        /* NULL-able [nv * 3]: NULL keeps the scene's; refused where the scene was made without normals */
    int64_t *parked;             /* NULL-able, one value: written with the number of triangles parked (above) */
} rls_nearest_refit_mesh;

/* Read the tree of `scene` (one download; it may synchronise) and upload one list of node indices per level.  The scene must
 * live on ctx's device and must outlive the refit.  An empty scene (nt == 0) gives a refit whose update launches nothing. */
rls_status rls_nearest_refit_create(rls_context *ctx, rls_nearest_scene *scene, rls_nearest_refit **out);
/* Free a refit (NULL: nothing).  The scene is not touched. */
rls_status rls_nearest_refit_destroy(rls_nearest_refit *refit);
rls_status rls_nearest_refit_get_info(const rls_nearest_refit *refit, rls_nearest_refit_info *info);
/* Move the scene to `mesh` on ctx's stream (above).  No host synchronisation, no allocation. */
rls_status rls_nearest_refit_update(rls_context *ctx, rls_nearest_refit *refit, const rls_nearest_refit_mesh *mesh);
/* HOST arrays, each NULL-able; synchronises.  boxes [nodes * 6] lo xyz hi xyz; links [nodes * 2] first, meta; prims [nt] the
 * triangle ids in leaf order. */
rls_status rls_nearest_refit_read_tree(rls_context *ctx, const rls_nearest_refit *refit, float *boxes, uint32_t *links,
                                       uint32_t *prims);

#ifdef __cplusplus
}
#endif

#endif
