// refit.hip -- moving meshes (include/rlshaders_amd_nearest_refit.h): the host side of librls_nearest_refit.so -- the refit's
// handle, what its creation adds to the common part (one list of node indices per level uploaded in one allocation, the plan
// of the update's launches), and the C ABI.  The record, the boxes, the levels and the kernels are in rls_nearest_refit.hpp;
// the borrowed scene's view, the common part of a creation, the mesh checks (each written once), the update's launches and the
// tree's read-back are in rls_nearest_update.hpp, which the library that builds the tree again states its host side by too.
//
// A sixth companion beside librls_ggx_rr.so, librls_trace.so, librls_walk.so, librls_shadow_walk.so and librls_nearest.so, for
// the same reason: the other libraries' device code and surfaces stay what they are.  It reads a scene through
// rls_nearest_scene.hpp alone and calls nothing of librls_nearest.so.  Built once (rlshaders_amd/build.py,
// build_nearest_refit_library): mode-free, one code object, compiled with RLS_FAST=0.
#include <stdlib.h>

#include "../csrc/rls_internal.hpp"
#include "../../include/rlshaders_amd_nearest_refit.h"

#if RLS_FAST
#error "refit.hip has no FAST flavour"
#endif

#include "rls_nearest_scene.hpp"
#include "rls_nearest_refit.hpp"
#include "rls_nearest_update.hpp"

static_assert(kRefitTopLevels >= RLS_NEAREST_STACK + 1, "a tree of the deepest scene fits the single-workgroup launch's offsets");

// info and device lead the struct: the update's checks read nothing else, so tests/test_nearest_refit_abi.py can lay the public
// info struct over dummy memory and reach every refusal without a device
struct rls_nearest_refit {
    rls_nearest_refit_info info;
    int device;
    rls_nearest_scene *scene;     // borrowed
    SceneView view;               // the scene's blob, writable
    uint32_t *lists;              // the refit's one device allocation: every node once, deepest level first
    std::vector<int64_t> offset;  // [levels + 1] into lists
    int folded;                   // the last `folded` levels (the top of the tree) run in one single-workgroup launch; 0: none
};

namespace {

// what the shared layer reports in this library's words: the layout refusal, three HIP calls as a failure has always named them
const UpdateTexts kTexts = {
    "scene is not a scene of this build's layout (librls_nearest.so and librls_nearest_refit.so must be of one build)",
    "hipMemcpyAsync(refit->normals, mesh->normals, (size_t)refit->info.nv * 3 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream)",
    "hipMemcpy(hn.data(), refit->nodes, hn.size() * sizeof(NearestNode), hipMemcpyDeviceToHost)",
    "hipMemcpy(ht.data(), refit->tris, ht.size() * sizeof(NearestTri), hipMemcpyDeviceToHost)"};

// RLS_NEAREST_REFIT_FOLD=0: one launch per level all the way up (the measurement in INTEGRATION.md section 6 compares the two)
bool fold_enabled()
{
    const char *e = getenv("RLS_NEAREST_REFIT_FOLD");
    return !(e && e[0] == '0');
}

} // namespace

extern "C" {

rls_status rls_nearest_refit_create(rls_context *ctx, rls_nearest_scene *scene, rls_nearest_refit **out)
{
    std::vector<NearestNode> host;
    std::vector<uint32_t> list;
    std::unique_ptr<rls_nearest_refit> r;
    bool tree = false;
    if (rls_status s = begin_create(__func__, kTexts, ctx, scene, out, r, host, list, tree)) return s;
    const int64_t nodes = r->info.nodes;
    if (nodes > 0) {
        if (!tree || r->info.levels > kRefitTopLevels) {
            rlsh::set_error("%s: the scene's nodes are not the tree its info describes", __func__);
            return RLS_ERR_UNSUPPORTED;
        }
        const size_t bytes = (size_t)nodes * sizeof(uint32_t);
        hipError_t e = hipMalloc((void **)&r->lists, bytes);
        if (e == hipSuccess) {
            e = hipMemcpy(r->lists, list.data(), bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) (void)hipFree(r->lists);
        }
        if (e != hipSuccess) return rlsh::hip_fail(e, "rls_nearest_refit_create: the level lists' upload");
        r->info.device_bytes = bytes;
        // the top of the tree: the trailing levels of at most kBlock nodes each; one level alone gains nothing
        const int levels = r->info.levels;
        int folded = 0;
        while (folded < levels && r->offset[(size_t)(levels - folded)] - r->offset[(size_t)(levels - folded - 1)] <= rlsh::kBlock) folded++;
        r->folded = fold_enabled() && folded >= 2 ? folded : 0;
    }
    *out = r.release();
    return RLS_OK;
}

rls_status rls_nearest_refit_destroy(rls_nearest_refit *refit)
{
    return destroy_handle(__func__, refit, &rls_nearest_refit::lists);
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
    return update_mesh(__func__, kTexts, ctx, refit, mesh, refit->folded, [] { return RLS_OK; });   // the tree stays: nothing of its own
}

rls_status rls_nearest_refit_read_tree(rls_context *ctx, const rls_nearest_refit *refit, float *boxes, uint32_t *links, uint32_t *prims)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(refit != nullptr, "refit is NULL");
    RLS_REQUIRE(refit->device == ctx->device, "the refit's scene lives on another device than ctx");
    return read_tree(__func__, kTexts, ctx, refit->info.nodes, refit->info.nt, refit->view, boxes, links, prims);
}

} // extern "C"
