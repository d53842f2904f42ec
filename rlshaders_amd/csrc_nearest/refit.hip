// refit.hip -- moving meshes (include/rlshaders_amd_nearest_refit.h): the host side of librls_nearest_refit.so -- a refit's
// creation (the scene's nodes downloaded once, one list of node indices per level uploaded in one allocation), the argument
// checks (each written once), the update's launches, the C ABI.  The record, the boxes, the levels and the kernels are in
// rls_nearest_refit.hpp.
//
// A sixth companion beside librls_ggx_rr.so, librls_trace.so, librls_walk.so, librls_shadow_walk.so and librls_nearest.so, for
// the same reason: the other libraries' device code and surfaces stay what they are.  It reads a scene through
// rls_nearest_scene.hpp alone and calls nothing of librls_nearest.so.  Built once (rlshaders_amd/build.py,
// build_nearest_refit_library): mode-free, one code object, compiled with RLS_FAST=0.
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "../csrc/rls_internal.hpp"
#include "../../include/rlshaders_amd_nearest_refit.h"

#if RLS_FAST
#error "refit.hip has no FAST flavour"
#endif

#include "rls_nearest_scene.hpp"
#include "rls_nearest_refit.hpp"

static_assert(kRefitTopLevels >= RLS_NEAREST_STACK + 1, "a tree of the deepest scene fits the single-workgroup launch's offsets");

// info and device lead the struct: the update's checks read nothing else, so tests/test_nearest_refit_abi.py can lay the public
// info struct over dummy memory and reach every refusal without a device
struct rls_nearest_refit {
    rls_nearest_refit_info info;
    int device;
    rls_nearest_scene *scene;     // borrowed
    NearestNode *nodes;           // the scene's blob, writable
    NearestTri *tris;
    const uint32_t *index;
    float *normals;               // NULL: the scene has none
    uint32_t *lists;              // the refit's one device allocation: every node once, deepest level first
    std::vector<int64_t> offset;  // [levels + 1] into lists
    int folded;                   // the last `folded` levels (the top of the tree) run in one single-workgroup launch; 0: none
};

namespace {

// RLS_NEAREST_REFIT_FOLD=0: one launch per level all the way up (the measurement in INTEGRATION.md section 6 compares the two)
bool fold_enabled()
{
    const char *e = getenv("RLS_NEAREST_REFIT_FOLD");
    return !(e && e[0] == '0');
}

// ---- the argument checks of the update, each written once ----------------------------------------------------------------------
rls_status check_mesh(const char *fn, const rls_nearest_refit *refit, const rls_nearest_refit_mesh *mesh)
{
    RLS_REQUIRE_IN(fn, mesh != nullptr, "mesh is NULL");
    RLS_REQUIRE_IN(fn, mesh->nv == refit->info.nv, "mesh.nv is not the scene's");
    RLS_REQUIRE_IN(fn, mesh->nv == 0 || mesh->vertices != nullptr, "mesh.vertices is NULL");
    RLS_REQUIRE_IN(fn, mesh->normals == nullptr || refit->info.has_normals, "mesh.normals is set but the scene was made without normals");
    return RLS_OK;
}

} // namespace

extern "C" {

rls_status rls_nearest_refit_create(rls_context *ctx, rls_nearest_scene *scene, rls_nearest_refit **out)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    RLS_REQUIRE(scene != nullptr, "scene is NULL");
    RLS_REQUIRE(scene->layout == kNearestSceneLayout, "scene is not a scene of this build's layout (librls_nearest.so and librls_nearest_refit.so must be of one build)");
    RLS_REQUIRE(scene->device == ctx->device, "the scene lives on another device than ctx");
    const int64_t nodes = scene->info.nodes, nt = scene->info.nt;
    std::vector<NearestNode> host;
    std::vector<uint32_t> list;
    rls_nearest_refit *r = nullptr;
    try {
        host.resize((size_t)nodes);
        r = new rls_nearest_refit();
    } catch (const std::bad_alloc &) {
        rlsh::set_error("%s: out of host memory", __func__);
        return RLS_ERR_OUT_OF_MEMORY;
    }
    r->scene = scene;
    r->device = scene->device;
    r->info.nv = scene->info.nv; r->info.nt = nt; r->info.nodes = nodes;
    r->info.levels = scene->info.depth;
    r->info.has_normals = scene->normals != nullptr;
    r->offset.assign(1, 0);
    if (nodes > 0) {
        char *blob = (char *)scene->blob;
        r->nodes = (NearestNode *)(blob + scene->o_nodes);
        r->tris = (NearestTri *)(blob + scene->o_tris);
        r->index = (const uint32_t *)(blob + scene->o_index);
        r->normals = scene->normals ? (float *)(blob + scene->o_normals) : nullptr;
        // an update of another refit, or a query, may be in flight on the stream: the links read here never change, the
        // boxes are not read
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipMemcpy(host.data(), r->nodes, (size_t)nodes * sizeof(NearestNode), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            delete r;
            return rlsh::hip_fail(e, "rls_nearest_refit_create: the tree's download");
        }
        bool tree = false;
        try {
            tree = refit_levels(host.data(), nodes, nt, list, r->offset);
        } catch (const std::bad_alloc &) {
            delete r;
            rlsh::set_error("%s: out of host memory", __func__);
            return RLS_ERR_OUT_OF_MEMORY;
        }
        if (!tree || (int64_t)r->offset.size() - 1 != scene->info.depth || scene->info.depth > kRefitTopLevels) {
            delete r;
            rlsh::set_error("%s: the scene's nodes are not the tree its info describes", __func__);
            return RLS_ERR_UNSUPPORTED;
        }
        const size_t bytes = (size_t)nodes * sizeof(uint32_t);
        e = hipMalloc((void **)&r->lists, bytes);
        if (e == hipSuccess) {
            e = hipMemcpy(r->lists, list.data(), bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) (void)hipFree(r->lists);
        }
        if (e != hipSuccess) {
            delete r;
            return rlsh::hip_fail(e, "rls_nearest_refit_create: the level lists' upload");
        }
        r->info.device_bytes = bytes;
        // the top of the tree: the trailing levels of at most kBlock nodes each; one level alone gains nothing
        const int levels = r->info.levels;
        int folded = 0;
        while (folded < levels && r->offset[(size_t)(levels - folded)] - r->offset[(size_t)(levels - folded - 1)] <= rlsh::kBlock) folded++;
        r->folded = fold_enabled() && folded >= 2 ? folded : 0;
    }
    *out = r;
    return RLS_OK;
}

rls_status rls_nearest_refit_destroy(rls_nearest_refit *refit)
{
    if (!refit) return RLS_OK;
    hipError_t e = hipSuccess;
    if (refit->lists) {
        e = hipSetDevice(refit->device);
        if (e == hipSuccess) e = hipFree(refit->lists);
    }
    delete refit;
    if (e != hipSuccess) return rlsh::hip_fail(e, "rls_nearest_refit_destroy");
    return RLS_OK;
}

rls_status rls_nearest_refit_get_info(const rls_nearest_refit *refit, rls_nearest_refit_info *info)
{
    RLS_REQUIRE(refit != nullptr, "refit is NULL");
    RLS_REQUIRE(info != nullptr, "info is NULL");
    *info = refit->info;
    return RLS_OK;
}

rls_status rls_nearest_refit_update(rls_context *ctx, rls_nearest_refit *refit, const rls_nearest_refit_mesh *mesh)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(refit != nullptr, "refit is NULL");
    if (rls_status s = check_mesh(__func__, refit, mesh)) return s;
    RLS_REQUIRE(refit->device == ctx->device, "the refit's scene lives on another device than ctx");
    const int64_t nt = refit->info.nt;
    const int levels = refit->info.levels;
    if (mesh->parked || (mesh->normals && refit->info.nv > 0)) RLS_HIP_TRY(hipSetDevice(ctx->device));
    if (mesh->parked) RLS_HIP_TRY(hipMemsetAsync(mesh->parked, 0, sizeof(int64_t), ctx->stream));
    if (nt > 0) {
        RefitRecordsIO io = {};
        io.tris = refit->tris; io.index = refit->index; io.vertices = mesh->vertices;
        io.parked = (unsigned long long *)mesh->parked;
        io.nt = nt; io.tiles = (nt + rlsh::kBlock - 1) / rlsh::kBlock;
        hipLaunchKernelGGL(refit_records_kernel, rlsh::grid_for(ctx, nt), dim3(rlsh::kBlock), 0, ctx->stream, io);
        if (rls_status s = rlsh::check_launch(__func__)) return s;
        const int wide = levels - refit->folded;                     // levels launched one by one, deepest first
        for (int l = 0; l < wide; l++) {
            RefitLevelIO lv = {};
            lv.nodes = refit->nodes; lv.tris = refit->tris; lv.list = refit->lists + refit->offset[(size_t)l];
            lv.count = refit->offset[(size_t)l + 1] - refit->offset[(size_t)l];
            lv.tiles = (lv.count + rlsh::kBlock - 1) / rlsh::kBlock;
            hipLaunchKernelGGL(refit_level_kernel, rlsh::grid_for(ctx, lv.count), dim3(rlsh::kBlock), 0, ctx->stream, lv);
            if (rls_status s = rlsh::check_launch(__func__)) return s;
        }
        if (refit->folded) {
            RefitTopIO top = {};
            top.nodes = refit->nodes; top.tris = refit->tris; top.list = refit->lists + refit->offset[(size_t)wide];
            top.levels = refit->folded;
            for (int l = 0; l <= refit->folded; l++) top.offset[l] = (uint32_t)(refit->offset[(size_t)(wide + l)] - refit->offset[(size_t)wide]);
            (void)rlsh::grid_for(ctx, 1);                                // the device made current, as ahead of every launch
            hipLaunchKernelGGL(refit_top_kernel, dim3(1), dim3(rlsh::kBlock), 0, ctx->stream, top);
            if (rls_status s = rlsh::check_launch(__func__)) return s;
        }
    }
    if (mesh->normals && refit->info.nv > 0)
        RLS_HIP_TRY(hipMemcpyAsync(refit->normals, mesh->normals, (size_t)refit->info.nv * 3 * sizeof(float), hipMemcpyDeviceToDevice,
                                   ctx->stream));
    refit->info.updates++;
    return RLS_OK;
}

rls_status rls_nearest_refit_read_tree(rls_context *ctx, const rls_nearest_refit *refit, float *boxes, uint32_t *links, uint32_t *prims)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(refit != nullptr, "refit is NULL");
    RLS_REQUIRE(refit->device == ctx->device, "the refit's scene lives on another device than ctx");
    const int64_t nodes = refit->info.nodes, nt = refit->info.nt;
    if (nodes == 0 || (!boxes && !links && !prims)) return RLS_OK;
    std::vector<NearestNode> hn;
    std::vector<NearestTri> ht;
    try {
        if (boxes || links) hn.resize((size_t)nodes);
        if (prims) ht.resize((size_t)nt);
    } catch (const std::bad_alloc &) {
        rlsh::set_error("%s: out of host memory", __func__);
        return RLS_ERR_OUT_OF_MEMORY;
    }
    RLS_HIP_TRY(hipSetDevice(ctx->device));
    RLS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!hn.empty()) RLS_HIP_TRY(hipMemcpy(hn.data(), refit->nodes, hn.size() * sizeof(NearestNode), hipMemcpyDeviceToHost));
    if (!ht.empty()) RLS_HIP_TRY(hipMemcpy(ht.data(), refit->tris, ht.size() * sizeof(NearestTri), hipMemcpyDeviceToHost));
    for (size_t n = 0; n < hn.size(); n++) {
        if (boxes)
            for (int c = 0; c < 3; c++) { boxes[6 * n + c] = hn[n].lo[c]; boxes[6 * n + 3 + c] = hn[n].hi[c]; }
        if (links) { links[2 * n] = hn[n].first; links[2 * n + 1] = hn[n].meta; }
    }
    for (size_t k = 0; k < ht.size(); k++) prims[k] = ht[k].prim;
    return RLS_OK;
}

} // extern "C"
