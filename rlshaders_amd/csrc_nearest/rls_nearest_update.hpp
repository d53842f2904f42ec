// rls_nearest_update.hpp -- the host layer the two libraries that move a nearest-hit scene to new vertices share, written once:
// the one that rewrites the boxes of the tree that is there and the one that builds the tree again borrow a scene, check a moved
// mesh, launch the records and the boxes, copy the normals and read a tree back the same way.  Included by each unit after
// csrc/rls_internal.hpp, rls_nearest_scene.hpp and rls_nearest_refit.hpp (the records' and boxes' kernels); each library compiles
// its own copy, and its kernels come out the machine code they were (rlshaders_amd/codeid.py, kernel_digests).
//
// A handle (Handle below) is a unit's own struct.  It LEADS with `info` (the unit's public info struct) and `int device` -- an
// update's checks read nothing else, so the ABI tests reach every refusal over dummy memory -- and has `scene`, `view`, `lists`
// and `offset` under these names.  A check's message names the entry point that refused (fn).  A message that names a library
// or its handle is that unit's literal: the ones the shared layer reports reach it as UpdateTexts.
#ifndef RLS_NEAREST_UPDATE_HPP
#define RLS_NEAREST_UPDATE_HPP

#include <memory>
#include <new>

struct UpdateTexts {
    const char *layout;                                       // the refusal of a scene whose layout tag is another build's
    const char *normals_copy, *nodes_download, *tris_download;  // the HIP calls that read the handle, as a failure names them
};

// The view of a borrowed scene: the parts of its blob an update writes (the scene's own pointers are the queries' and const).
struct SceneView {
    NearestNode *nodes;
    NearestTri *tris;
    const uint32_t *index;
    float *normals;               // NULL: the scene has none
};

static inline SceneView view_of(const rls_nearest_scene *scene)
{
    char *blob = (char *)scene->blob;
    return {(NearestNode *)(blob + scene->o_nodes), (NearestTri *)(blob + scene->o_tris), (const uint32_t *)(blob + scene->o_index),
            scene->normals ? (float *)(blob + scene->o_normals) : nullptr};
}

// A tile is kBlock elements, one per lane.
static inline int64_t tiles_of(int64_t count) { return (count + rlsh::kBlock - 1) / rlsh::kBlock; }

static inline rls_status out_of_host_memory(const char *fn)
{
    rlsh::set_error("%s: out of host memory", fn);
    return RLS_ERR_OUT_OF_MEMORY;
}

// ---- create: the common part ---------------------------------------------------------------------------------------------------
// The argument checks, the handle with the info both kinds have, and for a scene with nodes its view, the nodes downloaded
// (host) and their levels (list, the handle's offset; rls_nearest_refit.hpp).  tree: the nodes are a tree of the depth the
// scene's info states.  `made` owns the handle until the caller releases it into *out, so a return ahead of that leaves nothing
// allocated (the shared part allocates nothing on the device).  On a failure: a status, `made` empty.
template <class Handle>
rls_status begin_create(const char *fn, const UpdateTexts &texts, rls_context *ctx, rls_nearest_scene *scene, Handle **out,
                        std::unique_ptr<Handle> &made, std::vector<NearestNode> &host, std::vector<uint32_t> &list, bool &tree)
{
    RLS_REQUIRE_IN(fn, ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE_IN(fn, out != nullptr, "out is NULL");
    *out = nullptr;
    RLS_REQUIRE_IN(fn, scene != nullptr, "scene is NULL");
    RLS_REQUIRE_IN(fn, scene->layout == kNearestSceneLayout, texts.layout);
    RLS_REQUIRE_IN(fn, scene->device == ctx->device, "the scene lives on another device than ctx");
    const int64_t nodes = scene->info.nodes, nt = scene->info.nt;
    std::unique_ptr<Handle> h;
    try {
        host.resize((size_t)nodes);
        h.reset(new Handle());
        h->offset.assign(1, 0);
    } catch (const std::bad_alloc &) {
        return out_of_host_memory(fn);
    }
    h->scene = scene; h->device = scene->device;
    h->info.nv = scene->info.nv; h->info.nt = nt; h->info.nodes = nodes;
    h->info.levels = scene->info.depth;
    h->info.has_normals = scene->normals != nullptr;
    tree = true;
    if (nodes > 0) {
        h->view = view_of(scene);
        // an update of another handle, or a query, may be in flight on the stream: the links read here (first and the count
        // bits) never change, the boxes are not read
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipMemcpy(host.data(), h->view.nodes, (size_t)nodes * sizeof(NearestNode), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            char what[128];
            snprintf(what, sizeof(what), "%s: the tree's download", fn);
            return rlsh::hip_fail(e, what);
        }
        try {
            tree = refit_levels(host.data(), nodes, nt, list, h->offset) && (int64_t)h->offset.size() - 1 == scene->info.depth;
        } catch (const std::bad_alloc &) {
            return out_of_host_memory(fn);
        }
    }
    made = std::move(h);
    return RLS_OK;
}

// a handle's one device allocation (the member `allocation`; NULL: none) freed on its device, the handle deleted; NULL: nothing
template <class Handle, class T>
rls_status destroy_handle(const char *fn, Handle *h, T *Handle::*allocation)
{
    if (!h) return RLS_OK;
    hipError_t e = hipSuccess;
    if (h->*allocation) {
        e = hipSetDevice(h->device);
        if (e == hipSuccess) e = hipFree(h->*allocation);
    }
    delete h;
    if (e != hipSuccess) return rlsh::hip_fail(e, fn);
    return RLS_OK;
}

// ---- the argument checks of the update, each written once; the two public mesh structs are distinct types of the same members -----
template <class Handle, class Mesh>
rls_status check_mesh(const char *fn, const Handle *h, const Mesh *mesh)
{
    RLS_REQUIRE_IN(fn, mesh != nullptr, "mesh is NULL");
    RLS_REQUIRE_IN(fn, mesh->nv == h->info.nv, "mesh.nv is not the scene's");
    RLS_REQUIRE_IN(fn, mesh->nv == 0 || mesh->vertices != nullptr, "mesh.vertices is NULL");
    RLS_REQUIRE_IN(fn, mesh->normals == nullptr || h->info.has_normals, "mesh.normals is set but the scene was made without normals");
    return RLS_OK;
}

// ---- the update's frame ----------------------------------------------------------------------------------------------------------
// The prologue: the device made current for the calls that are no launches, the parked counter zeroed on the stream.  Then, for a
// scene with triangles, what the unit's update adds (own; none: the tree stays), the records, and the boxes bottom-up -- a launch
// per level, deepest first, for all but the last `folded` levels, and those (the top of the tree; 0: none) in one
// single-workgroup launch.  The epilogue: the normals copied after the launches, the update counted.
template <class Handle, class Mesh, class Own>
rls_status update_mesh(const char *fn, const UpdateTexts &texts, rls_context *ctx, Handle *h, const Mesh *mesh, int folded, Own own)
{
    const SceneView &v = h->view;
    const int64_t nt = h->info.nt;
    if (mesh->parked || (mesh->normals && h->info.nv > 0)) RLS_HIP_TRY(hipSetDevice(ctx->device));
    if (mesh->parked) RLS_HIP_TRY(hipMemsetAsync(mesh->parked, 0, sizeof(int64_t), ctx->stream));
    if (nt > 0) {
        if (rls_status s = own()) return s;
        RefitRecordsIO io = {};
        io.tris = v.tris; io.index = v.index; io.vertices = mesh->vertices;
        io.parked = (unsigned long long *)mesh->parked;
        io.nt = nt; io.tiles = tiles_of(nt);
        hipLaunchKernelGGL(refit_records_kernel, rlsh::grid_for(ctx, nt), dim3(rlsh::kBlock), 0, ctx->stream, io);
        if (rls_status s = rlsh::check_launch(fn)) return s;
        const int wide = h->info.levels - folded;                        // levels launched one by one, deepest first
        for (int l = 0; l < wide; l++) {
            RefitLevelIO lv = {};
            lv.nodes = v.nodes; lv.tris = v.tris; lv.list = h->lists + h->offset[(size_t)l];
            lv.count = h->offset[(size_t)l + 1] - h->offset[(size_t)l];
            lv.tiles = tiles_of(lv.count);
            hipLaunchKernelGGL(refit_level_kernel, rlsh::grid_for(ctx, lv.count), dim3(rlsh::kBlock), 0, ctx->stream, lv);
            if (rls_status s = rlsh::check_launch(fn)) return s;
        }
        if (folded) {
            RefitTopIO top = {};
            top.nodes = v.nodes; top.tris = v.tris; top.list = h->lists + h->offset[(size_t)wide];
            top.levels = folded;
            for (int l = 0; l <= folded; l++) top.offset[l] = (uint32_t)(h->offset[(size_t)(wide + l)] - h->offset[(size_t)wide]);
            (void)rlsh::grid_for(ctx, 1);                                // the device made current, as ahead of every launch
            hipLaunchKernelGGL(refit_top_kernel, dim3(1), dim3(rlsh::kBlock), 0, ctx->stream, top);
            if (rls_status s = rlsh::check_launch(fn)) return s;
        }
    }
    if (mesh->normals && h->info.nv > 0) {
        hipError_t e = hipMemcpyAsync(v.normals, mesh->normals, (size_t)h->info.nv * 3 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) return rlsh::hip_fail(e, texts.normals_copy);
    }
    h->info.updates++;
    return RLS_OK;
}

// ---- the tree read back: boxes [nodes, 6], links [nodes, 2], prims [nt], each NULL-able; synchronises ----------------------------
static inline rls_status read_tree(const char *fn, const UpdateTexts &texts, rls_context *ctx, int64_t nodes, int64_t nt, const SceneView &v,
                                   float *boxes, uint32_t *links, uint32_t *prims)
{
    if (nodes == 0 || (!boxes && !links && !prims)) return RLS_OK;
    std::vector<NearestNode> hn;
    std::vector<NearestTri> ht;
    try {
        if (boxes || links) hn.resize((size_t)nodes);
        if (prims) ht.resize((size_t)nt);
    } catch (const std::bad_alloc &) {
        return out_of_host_memory(fn);
    }
    RLS_HIP_TRY(hipSetDevice(ctx->device));
    RLS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    hipError_t e = hn.empty() ? hipSuccess : hipMemcpy(hn.data(), v.nodes, hn.size() * sizeof(NearestNode), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return rlsh::hip_fail(e, texts.nodes_download);
    e = ht.empty() ? hipSuccess : hipMemcpy(ht.data(), v.tris, ht.size() * sizeof(NearestTri), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return rlsh::hip_fail(e, texts.tris_download);
    for (size_t n = 0; n < hn.size(); n++) {
        if (boxes)
            for (int c = 0; c < 3; c++) { boxes[6 * n + c] = hn[n].lo[c]; boxes[6 * n + 3 + c] = hn[n].hi[c]; }
        if (links) { links[2 * n] = hn[n].first; links[2 * n + 1] = hn[n].meta; }
    }
    for (size_t k = 0; k < ht.size(); k++) prims[k] = ht[k].prim;
    return RLS_OK;
}

#endif
