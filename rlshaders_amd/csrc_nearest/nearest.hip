// nearest.hip -- nearest-hit queries over a triangle mesh (include/rlshaders_amd_nearest.h): the host side of librls_nearest.so
// -- a scene's creation (the tree of rls_nearest_bvh.hpp, one allocation, one upload), the argument checks (each written
// once), the one launch path of both queries, the C ABI.  The slab test, the triangle test, the traversal and the kernel are in
// rls_nearest_device.hpp.
//
// A fifth companion beside librls_ggx_rr.so, librls_trace.so, librls_walk.so and librls_shadow_walk.so, for the same reason:
// the product's device code and the other libraries' surfaces stay what they are.  Built once (rlshaders_amd/build.py,
// build_nearest_library): the query is mode-free, so there is one code object, compiled with RLS_FAST=0 -- IEEE arithmetic.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "../csrc/rls_internal.hpp"
#include "../../include/rlshaders_amd_nearest.h"

#if RLS_FAST
#error "nearest.hip has no FAST flavour"
#endif

static_assert(RLS_NEAREST_STACK == 24, "the header's stack size is the kernel's");

#include "rls_nearest_device.hpp"

static_assert(kNearestStack == RLS_NEAREST_STACK, "the header's stack size is the kernel's");

#include "rls_nearest_scene.hpp"                    // struct rls_nearest_scene: the layout the refit library shares

namespace {

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline bool all3(rls_vec3 v) { return v.x && v.y && v.z; }
inline bool none3(rls_vec3 v) { return !v.x && !v.y && !v.z; }

// ---- the argument checks, each written once; fn: the entry point its message names ---------------------------------------------
rls_status check_found(const char *fn, const rls_nearest_found *f, int64_t rays)
{
    RLS_REQUIRE_IN(fn, f != nullptr, "found is NULL");
    RLS_REQUIRE_IN(fn, rays == 0 || (f->hit != nullptr && f->t != nullptr), "found.hit or found.t plane is NULL");
    RLS_REQUIRE_IN(fn, (all3(f->P) || none3(f->P)) && (all3(f->N) || none3(f->N)) && (all3(f->Ns) || none3(f->Ns)) &&
                           (all3(f->T) || none3(f->T)) && (all3(f->wo) || none3(f->wo)),
                   "found.P, N, Ns, T or wo is partly NULL: all three planes or none");
    RLS_REQUIRE_IN(fn, f->bin == nullptr || (f->bin_of_surface != nullptr && f->bin_count >= 1),
                   "found.bin is set with found.bin_of_surface NULL or found.bin_count == 0");
    return RLS_OK;
}

// the one launch path: both queries arrive here with their rays in one struct
rls_status launch(const char *fn, rls_context *ctx, const rls_nearest_scene *scene, const rls_nearest_rays &r,
                  const rls_nearest_found *f)
{
    RLS_REQUIRE_IN(fn, r.rays >= 0, "rays < 0");
    RLS_REQUIRE_IN(fn, r.rays <= (int64_t)UINT32_MAX, "rays > 2^32 - 1 (a ray id is 32-bit)");
    RLS_REQUIRE_IN(fn, r.rays == 0 || (rlsh::has3(r.origin) && rlsh::has3(r.dir)), "rays.origin or rays.dir plane is NULL");
    if (rls_status s = check_found(fn, f, r.rays)) return s;
    if (r.rays == 0) return RLS_OK;
    RLS_REQUIRE_IN(fn, scene->device == ctx->device, "the scene lives on another device than ctx");
    NearestIO io = {};
    io.nodes = scene->nodes; io.tris = scene->tris; io.index = scene->index; io.surface = scene->surface;
    io.normals = scene->normals; io.node_count = scene->info.nodes;
    io.r = r; io.f = *f;
    io.tiles = (r.rays + rlsh::kBlock - 1) / rlsh::kBlock;
    hipLaunchKernelGGL(nearest_kernel, rlsh::grid_for(ctx, r.rays), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(fn);
}

} // namespace

extern "C" {

rls_status rls_nearest_scene_create(rls_context *ctx, const rls_nearest_mesh *mesh, rls_nearest_scene **out)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    RLS_REQUIRE(mesh != nullptr, "mesh is NULL");
    RLS_REQUIRE(mesh->nv >= 0 && mesh->nt >= 0, "mesh.nv or mesh.nt < 0");
    RLS_REQUIRE(mesh->nv <= (int64_t)UINT32_MAX, "mesh.nv > 2^32 - 1 (a vertex index is 32-bit)");
    RLS_REQUIRE(mesh->nt <= RLS_NEAREST_MAX_TRIANGLES, "mesh.nt > 2^22: the traversal stack of 24 entries bounds the tree's depth");
    RLS_REQUIRE(mesh->leaf_size >= 0 && mesh->leaf_size <= RLS_NEAREST_MAX_LEAF, "mesh.leaf_size must be in [1, 8], or 0 for the default");
    RLS_REQUIRE(mesh->nv == 0 || mesh->vertices != nullptr, "mesh.vertices is NULL");
    RLS_REQUIRE(mesh->nt == 0 || mesh->triangles != nullptr, "mesh.triangles is NULL");
    const int64_t nv = mesh->nv, nt = mesh->nt;
    for (int64_t i = 0; i < 3 * nt; i++) RLS_REQUIRE((int64_t)mesh->triangles[i] < nv, "mesh.triangles holds an index >= mesh.nv");
    for (int64_t i = 0; i < 3 * nv; i++) RLS_REQUIRE(isfinite(mesh->vertices[i]), "mesh.vertices holds a NaN or an inf");
    const int leaf = mesh->leaf_size ? mesh->leaf_size : RLS_NEAREST_DEFAULT_LEAF;

    NearestBvh bvh;
    rls_nearest_scene *sc = nullptr;
    char *host = nullptr;
    size_t o_nodes = 0, o_tris = 0, o_index = 0, o_surface = 0, o_normals = 0, bytes = 0;
    try {
        nearest_build(mesh->vertices, mesh->triangles, nt, leaf, bvh);
        auto carve = [&](size_t b) { const size_t at = bytes; bytes += align256(b); return at; };
        o_nodes = carve(bvh.nodes.size() * sizeof(NearestNode));
        o_tris = carve(bvh.tris.size() * sizeof(NearestTri));
        o_index = carve((size_t)nt * 3 * sizeof(uint32_t));
        o_surface = carve(mesh->surface ? (size_t)nt * sizeof(uint32_t) : 0);
        o_normals = carve(mesh->normals ? (size_t)nv * 3 * sizeof(float) : 0);
        sc = new rls_nearest_scene();
        if (bytes) host = new char[bytes]();
    } catch (const std::bad_alloc &) {
        delete sc;
        rlsh::set_error("%s: out of host memory", __func__);
        return RLS_ERR_OUT_OF_MEMORY;
    }
    // one sibling per inner level: a tree of `depth` levels needs depth - 1 stack entries
    if (bvh.depth - 1 > RLS_NEAREST_STACK || bvh.depth > nearest_depth_bound(nt, leaf)) {
        delete sc; delete[] host;
        rlsh::set_error("%s: the tree is deeper than its bound", __func__);
        return RLS_ERR_UNSUPPORTED;
    }
    sc->layout = kNearestSceneLayout;
    sc->device = ctx->device;
    sc->o_nodes = o_nodes; sc->o_tris = o_tris; sc->o_index = o_index; sc->o_surface = o_surface; sc->o_normals = o_normals;
    sc->info.nv = nv; sc->info.nt = nt; sc->info.nodes = (int64_t)bvh.nodes.size();
    sc->info.leaf_size = leaf; sc->info.depth = bvh.depth; sc->info.device_bytes = bytes;
    if (bytes) {
        if (!bvh.nodes.empty()) memcpy(host + o_nodes, bvh.nodes.data(), bvh.nodes.size() * sizeof(NearestNode));
        if (!bvh.tris.empty()) memcpy(host + o_tris, bvh.tris.data(), bvh.tris.size() * sizeof(NearestTri));
        if (nt) memcpy(host + o_index, mesh->triangles, (size_t)nt * 3 * sizeof(uint32_t));
        if (mesh->surface && nt) memcpy(host + o_surface, mesh->surface, (size_t)nt * sizeof(uint32_t));
        if (mesh->normals && nv) memcpy(host + o_normals, mesh->normals, (size_t)nv * 3 * sizeof(float));
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipMalloc(&sc->blob, bytes);
        if (e == hipSuccess) {
            e = hipMemcpy(sc->blob, host, bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) (void)hipFree(sc->blob);
        }
        delete[] host;
        if (e != hipSuccess) {
            delete sc;
            return rlsh::hip_fail(e, "rls_nearest_scene_create: the scene's upload");
        }
        char *d = (char *)sc->blob;
        sc->nodes = (const NearestNode *)(d + o_nodes);
        sc->tris = (const NearestTri *)(d + o_tris);
        sc->index = (const uint32_t *)(d + o_index);
        sc->surface = mesh->surface && nt ? (const uint32_t *)(d + o_surface) : nullptr;
        sc->normals = mesh->normals && nv ? (const float *)(d + o_normals) : nullptr;
    }
    *out = sc;
    return RLS_OK;
}

rls_status rls_nearest_scene_destroy(rls_nearest_scene *scene)
{
    if (!scene) return RLS_OK;
    hipError_t e = hipSuccess;
    if (scene->blob) {
        e = hipSetDevice(scene->device);
        if (e == hipSuccess) e = hipFree(scene->blob);
    }
    delete scene;
    if (e != hipSuccess) return rlsh::hip_fail(e, "rls_nearest_scene_destroy");
    return RLS_OK;
}

rls_status rls_nearest_scene_get_info(const rls_nearest_scene *scene, rls_nearest_scene_info *info)
{
    RLS_REQUIRE(scene != nullptr, "scene is NULL");
    RLS_REQUIRE(info != nullptr, "info is NULL");
    *info = scene->info;
    return RLS_OK;
}

rls_status rls_nearest_hits(rls_context *ctx, const rls_nearest_scene *scene, const rls_nearest_rays *rays,
                            const rls_nearest_found *found)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(scene != nullptr, "scene is NULL");
    RLS_REQUIRE(rays != nullptr, "rays is NULL");
    return launch(__func__, ctx, scene, *rays, found);
}

rls_status rls_nearest_walk_hits(rls_context *ctx, const rls_nearest_scene *scene, const rls_walk_rays *list, int64_t bound,
                                 const rls_nearest_found *found)
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

} // extern "C"
