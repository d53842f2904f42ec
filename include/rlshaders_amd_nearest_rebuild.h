/*
 * rlshaders_amd_nearest_rebuild.h -- moving meshes: rebuild the tree of a nearest-hit scene on the device (companion library
 * librls_nearest_rebuild.so).
 *
 * rls_nearest_scene_create (rlshaders_amd_nearest.h) builds a scene's tree on the host, for the mesh it is given.  A mesh that
 * deforms far from that pose keeps valid boxes under a box-only update, but the splits were chosen for the first mesh and a
 * query pays for it.  A rebuild chooses the splits again, for the moved vertices, where they are:
 * on the device, on the stream, with no download, no allocation and no synchronisation.
 *
 *   rls_nearest_scene_create -> rls_nearest_rebuild_create                          (once)
 *   every so often: the deformer -> rls_nearest_rebuild_update -> rls_nearest_hits / _walk_hits ... on the same stream
 *
 * THE STATEMENT.  After rls_nearest_rebuild_update the scene holds THE TREE THE HOST BUILDER BUILDS FROM THE MOVED MESH
 * (csrc_nearest/rls_nearest_bvh.hpp, nearest_build: what rls_nearest_scene_create would upload for mesh.vertices), with
 * PARKED triangles taken as three vertices at the origin:
 *   - every node's first and meta equal that tree's exactly, the split axis bits included;
 *   - the order of the triangle records (the triangle ids in leaf order) equals that tree's exactly;
 *   - every box equals that tree's by value.  A zero bound can differ in SIGN (the builder folds the boxes in another
 *     order); no result depends on it, and rls_nearest_rebuild_read_tree's boxes are to be compared by value.
 * Consequences: a query returns, bit for bit, what a fresh scene made from the new vertices returns (the statement of
 * rlshaders_amd_nearest.h already makes a result a function of mesh and ray alone); its COST is a fresh scene's cost too, the
 * same nodes opened and the same triangles tested; found.last of a query (the triangle a ray stands on) stays valid across an
 * update, triangle ids do not change; the scene's info (depth, nodes, device_bytes) does not change, and neither does any
 * link between nodes: the shape of the builder's tree is a function of the triangle count and the leaf size alone, so a
 * rebuild rewrites split axes, the order of the records and the boxes, and nothing else.  An update of the box-only kind
 * made for the scene earlier therefore stays valid after a rebuild, and the other way round.
 *
 * A triangle with a NaN or an infinity in any of its nine coordinates is PARKED: its record holds three vertices at the
 * origin, it is never a candidate of a query, its box and its place in the tree are the origin's.  *mesh.parked, where given,
 * is written with the exact number of parked triangles.  mesh.normals, where given, replace the scene's per-vertex normals
 * (a device-to-device copy).  Nothing else of the scene is written: the index array, the surface ids and every size stay.
 *
 * rls_nearest_rebuild_update never synchronises the host and allocates nothing -- its working set (sort keys, three sorted
 * lists and their double, a scan: info.device_bytes) is allocated by rls_nearest_rebuild_create -- so it can be recorded into
 * an rls_graph; a replay reads the vertex (and normal) buffers as they are then.  Queries issued on the same stream
 * afterwards see the new tree; a query running on ANOTHER stream during an update reads a tree in motion, which is the
 * caller's to order.  One scene takes one update at a time.
 *
 * A rebuild BORROWS its scene: the scene must outlive it (the Python and C++ wrappers hold a reference).  Refusals leave
 * "<entry point>: <text>" in rls_last_error; the argument checks run before the context is read.  Link
 * librls_nearest_rebuild.so (it needs librlshaders_amd.so alone; the scene comes from librls_nearest.so, which the caller
 * links for it, and both libraries must be of one build: a scene of another layout is refused).
 */
#ifndef RLSHADERS_AMD_NEAREST_REBUILD_H
#define RLSHADERS_AMD_NEAREST_REBUILD_H

#include "rlshaders_amd_nearest.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rls_nearest_rebuild rls_nearest_rebuild;

/* What a rebuild holds, for a caller's records. */
typedef struct rls_nearest_rebuild_info {
    int64_t nv, nt, nodes;       /* the scene's */
    int levels;                  /* = the scene's depth; 0 for an empty scene */
    int leaf_size;               /* the scene's */
    int has_normals;             /* the scene was made with per-vertex normals */
    size_t device_bytes;         /* the rebuild's own allocation: the working set of an update and the per-node tables */
    int64_t updates;             /* rls_nearest_rebuild_update calls accepted so far (a graph's replays are not calls) */
} rls_nearest_rebuild_info;

/* The moved mesh, DEVICE pointers. */
typedef struct rls_nearest_rebuild_mesh {
    int64_t nv;                  /* must equal the scene's */
    const float *vertices;       /* [nv * 3] xyz per vertex */
    const float *normals;        /* NULL-able [nv * 3]: NULL keeps the scene's; refused where the scene was made without normals */
    int64_t *parked;             /* NULL-able, one value: written with the number of triangles parked (above) */
} rls_nearest_rebuild_mesh;

/* Read the links of `scene` (one download; it may synchronise), refuse a tree that has not the builder's shape, and allocate
 * the working set.  The scene must live on ctx's device and must outlive the rebuild.  An empty scene (nt == 0) gives a
 * rebuild whose update launches nothing. */
rls_status rls_nearest_rebuild_create(rls_context *ctx, rls_nearest_scene *scene, rls_nearest_rebuild **out);
/* Free a rebuild (NULL: nothing).  The scene is not touched. */
rls_status rls_nearest_rebuild_destroy(rls_nearest_rebuild *rebuild);
rls_status rls_nearest_rebuild_get_info(const rls_nearest_rebuild *rebuild, rls_nearest_rebuild_info *info);
/* Rebuild the scene's tree for `mesh` on ctx's stream (above).  No host synchronisation, no allocation. */
rls_status rls_nearest_rebuild_update(rls_context *ctx, rls_nearest_rebuild *rebuild, const rls_nearest_rebuild_mesh *mesh);
/* HOST arrays, each NULL-able; synchronises.  boxes [nodes * 6] lo xyz hi xyz; links [nodes * 2] first, meta; prims [nt] the
 * triangle ids in leaf order. */
rls_status rls_nearest_rebuild_read_tree(rls_context *ctx, const rls_nearest_rebuild *rebuild, float *boxes, uint32_t *links,
                                         uint32_t *prims);

#ifdef __cplusplus
}
#endif

#endif
