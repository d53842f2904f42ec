// rebuild.hip -- rebuilding a scene's tree on the device (include/rlshaders_amd_nearest_rebuild.h): the host side of
// librls_nearest_rebuild.so -- a rebuild's creation (the scene's nodes downloaded once, held to the builder's shape; the
// per-node ranges, the per-level node lists and the update's working set in ONE allocation), the argument checks (each
// written once), the update's launches, the C ABI.  The algorithm, its one-element functions and the kernels are in
// rls_nearest_rebuild.hpp; the records and the boxes are the refit's (rls_nearest_refit.hpp), included there.
//
// A seventh companion beside librls_ggx_rr.so, librls_trace.so, librls_walk.so, librls_shadow_walk.so, librls_nearest.so and
// librls_nearest_refit.so, for the same reason: the other libraries' device code and surfaces stay what they are.  It reads a
// scene through rls_nearest_scene.hpp alone and calls nothing of the two other nearest libraries.  Built once
// (rlshaders_amd/build.py, build_nearest_rebuild_library): mode-free, one code object, compiled with RLS_FAST=0.
#include <stdlib.h>
#include <string.h>

#include <new>
#include <utility>
#include <vector>

#include "../csrc/rls_internal.hpp"
#include "../../include/rlshaders_amd_nearest_rebuild.h"

#if RLS_FAST
#error "rebuild.hip has no FAST flavour"
#endif

#include "rls_nearest_scene.hpp"
#include "rls_nearest_rebuild.hpp"

static_assert(kRebuildMaxLeaf == RLS_NEAREST_MAX_LEAF, "a leaf's ids fit the leaf kernel's registers");
static_assert(3 * RLS_NEAREST_MAX_TRIANGLES < ((int64_t)1 << 32), "a position in the three lists fits 32 bits");

// info and device lead the struct: the update's checks read nothing else, so tests/test_nearest_rebuild_abi.py can lay the
// public info struct over dummy memory and reach every refusal without a device
struct rls_nearest_rebuild {
    rls_nearest_rebuild_info info;
    int device;
    rls_nearest_scene *scene;     // borrowed
    float *normals;               // the scene's, writable; NULL: the scene has none
    void *blob;                   // the rebuild's one device allocation
    RebuildWork work;             // its parts and the scene's (vertices: an update's)
    uint32_t *lists;              // every node once, deepest level first (refit_levels)
    uint32_t *counts, *sums;      // the sort's [3][digits][tpa] counts; a scan's tile sums
    int64_t tpa;                  // tiles of one list
    std::vector<int64_t> offset;  // [levels + 1] into lists
};

namespace {

// ---- the argument checks of the update, each written once ----------------------------------------------------------------------
rls_status check_mesh(const char *fn, const rls_nearest_rebuild *rebuild, const rls_nearest_rebuild_mesh *mesh)
{
    RLS_REQUIRE_IN(fn, mesh != nullptr, "mesh is NULL");
    RLS_REQUIRE_IN(fn, mesh->nv == rebuild->info.nv, "mesh.nv is not the scene's");
    RLS_REQUIRE_IN(fn, mesh->nv == 0 || mesh->vertices != nullptr, "mesh.vertices is NULL");
    RLS_REQUIRE_IN(fn, mesh->normals == nullptr || rebuild->info.has_normals, "mesh.normals is set but the scene was made without normals");
    return RLS_OK;
}

int64_t tiles_of(int64_t count) { return (count + kRebuildTile - 1) / kRebuildTile; }

// the three launches of an exclusive scan over `count` values (rls_nearest_rebuild.hpp)
rls_status launch_scan(rls_context *ctx, const char *fn, RebuildScanIO io)
{
    io.tiles = tiles_of(io.count);
    hipLaunchKernelGGL(rebuild_scan_reduce_kernel, rlsh::grid_for(ctx, io.count), dim3(rlsh::kBlock), 0, ctx->stream, io);
    if (rls_status s = rlsh::check_launch(fn)) return s;
    (void)rlsh::grid_for(ctx, 1);                                        // the device made current, as ahead of every launch
    hipLaunchKernelGGL(rebuild_scan_sums_kernel, dim3(1), dim3(rlsh::kBlock), 0, ctx->stream, io);
    if (rls_status s = rlsh::check_launch(fn)) return s;
    hipLaunchKernelGGL(rebuild_scan_apply_kernel, rlsh::grid_for(ctx, io.count), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(fn);
}

template <class Kernel>
rls_status launch_over(rls_context *ctx, const char *fn, Kernel kernel, const RebuildWork &w, int64_t count)
{
    RebuildIO io = {};
    io.w = w; io.count = count; io.tiles = tiles_of(count);
    hipLaunchKernelGGL(kernel, rlsh::grid_for(ctx, count), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(fn);
}

size_t aligned(size_t bytes) { return (bytes + 255u) & ~(size_t)255u; }

} // namespace

extern "C" {

rls_status rls_nearest_rebuild_create(rls_context *ctx, rls_nearest_scene *scene, rls_nearest_rebuild **out)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    RLS_REQUIRE(scene != nullptr, "scene is NULL");
    RLS_REQUIRE(scene->layout == kNearestSceneLayout, "scene is not a scene of this build's layout (librls_nearest.so and librls_nearest_rebuild.so must be of one build)");
    RLS_REQUIRE(scene->device == ctx->device, "the scene lives on another device than ctx");
    const int64_t nodes = scene->info.nodes, nt = scene->info.nt;
    std::vector<NearestNode> host;
    std::vector<uint32_t> list;
    std::vector<RebuildRange> range;
    rls_nearest_rebuild *r = nullptr;
    try {
        host.resize((size_t)nodes);
        r = new rls_nearest_rebuild();
    } catch (const std::bad_alloc &) {
        rlsh::set_error("%s: out of host memory", __func__);
        return RLS_ERR_OUT_OF_MEMORY;
    }
    r->scene = scene;
    r->device = scene->device;
    r->info.nv = scene->info.nv; r->info.nt = nt; r->info.nodes = nodes;
    r->info.levels = scene->info.depth;
    r->info.leaf_size = scene->info.leaf_size;
    r->info.has_normals = scene->normals != nullptr;
    r->offset.assign(1, 0);
    if (nodes > 0) {
        char *sblob = (char *)scene->blob;
        RebuildWork &w = r->work;
        w.nodes = (NearestNode *)(sblob + scene->o_nodes);
        w.tris = (NearestTri *)(sblob + scene->o_tris);
        w.index = (const uint32_t *)(sblob + scene->o_index);
        w.nt = (uint32_t)nt; w.leaf = (uint32_t)scene->info.leaf_size;
        r->normals = scene->normals ? (float *)(sblob + scene->o_normals) : nullptr;
        // an update or a query may be in flight on the stream: first and the count bits read here never change
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipMemcpy(host.data(), w.nodes, (size_t)nodes * sizeof(NearestNode), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            delete r;
            return rlsh::hip_fail(e, "rls_nearest_rebuild_create: the tree's download");
        }
        bool tree = false;
        try {
            tree = nt <= RLS_NEAREST_MAX_TRIANGLES && refit_levels(host.data(), nodes, nt, list, r->offset) &&
                   rebuild_shape(host.data(), nodes, nt, scene->info.leaf_size, range);
        } catch (const std::bad_alloc &) {
            delete r;
            rlsh::set_error("%s: out of host memory", __func__);
            return RLS_ERR_OUT_OF_MEMORY;
        }
        if (!tree || (int64_t)r->offset.size() - 1 != scene->info.depth) {
            delete r;
            rlsh::set_error("%s: the scene's nodes are not the builder's tree of its triangle count and leaf size", __func__);
            return RLS_ERR_UNSUPPORTED;
        }
        r->tpa = tiles_of(nt);
        const int64_t count_entries = 3 * (int64_t)kRebuildDigits * r->tpa;
        const int64_t sum_entries = std::max(tiles_of(3 * nt), tiles_of(count_entries));
        // the parts of the one allocation, each on a 256-byte boundary
        const size_t b_range = aligned((size_t)nodes * sizeof(RebuildRange)), b_lists = aligned((size_t)nodes * sizeof(uint32_t));
        const size_t b_plane = aligned(3 * (size_t)nt * sizeof(uint32_t)), b_at = aligned((size_t)nt * sizeof(uint32_t));
        const size_t b_flag = aligned((size_t)nt), b_counts = aligned((size_t)count_entries * sizeof(uint32_t));
        const size_t b_sums = aligned((size_t)sum_entries * sizeof(uint32_t));
        const size_t bytes = b_range + b_lists + 4 * b_plane + b_at + b_flag + b_counts + b_sums;
        e = hipMalloc(&r->blob, bytes);
        if (e == hipSuccess) {
            char *p = (char *)r->blob;
            w.range = (const RebuildRange *)p; p += b_range;
            r->lists = (uint32_t *)p; p += b_lists;
            w.key = (uint32_t *)p; p += b_plane;
            w.list = (uint32_t *)p; p += b_plane;
            w.other = (uint32_t *)p; p += b_plane;
            w.scan = (uint32_t *)p; p += b_plane;
            w.node_at = (uint32_t *)p; p += b_at;
            w.flag = (uint8_t *)p; p += b_flag;
            r->counts = (uint32_t *)p; p += b_counts;
            r->sums = (uint32_t *)p;
            e = hipMemset(r->blob, 0, bytes);                            // every list entry is a triangle id from the first update on
            if (e == hipSuccess) e = hipMemcpy((void *)w.range, range.data(), (size_t)nodes * sizeof(RebuildRange), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(r->lists, list.data(), (size_t)nodes * sizeof(uint32_t), hipMemcpyHostToDevice);
            if (e != hipSuccess) (void)hipFree(r->blob);
        }
        if (e != hipSuccess) {
            delete r;
            return rlsh::hip_fail(e, "rls_nearest_rebuild_create: the working set");
        }
        r->info.device_bytes = bytes;
    }
    *out = r;
    return RLS_OK;
}

rls_status rls_nearest_rebuild_destroy(rls_nearest_rebuild *rebuild)
{
    if (!rebuild) return RLS_OK;
    hipError_t e = hipSuccess;
    if (rebuild->blob) {
        e = hipSetDevice(rebuild->device);
        if (e == hipSuccess) e = hipFree(rebuild->blob);
    }
    delete rebuild;
    if (e != hipSuccess) return rlsh::hip_fail(e, "rls_nearest_rebuild_destroy");
    return RLS_OK;
}

rls_status rls_nearest_rebuild_get_info(const rls_nearest_rebuild *rebuild, rls_nearest_rebuild_info *info)
{
    RLS_REQUIRE(rebuild != nullptr, "rebuild is NULL");
    RLS_REQUIRE(info != nullptr, "info is NULL");
    *info = rebuild->info;
    return RLS_OK;
}

rls_status rls_nearest_rebuild_update(rls_context *ctx, rls_nearest_rebuild *rebuild, const rls_nearest_rebuild_mesh *mesh)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(rebuild != nullptr, "rebuild is NULL");
    if (rls_status s = check_mesh(__func__, rebuild, mesh)) return s;
    RLS_REQUIRE(rebuild->device == ctx->device, "the rebuild's scene lives on another device than ctx");
    const int64_t nt = rebuild->info.nt, nodes = rebuild->info.nodes;
    const int levels = rebuild->info.levels;
    if (mesh->parked || (mesh->normals && rebuild->info.nv > 0)) RLS_HIP_TRY(hipSetDevice(ctx->device));
    if (mesh->parked) RLS_HIP_TRY(hipMemsetAsync(mesh->parked, 0, sizeof(int64_t), ctx->stream));
    if (nt > 0) {
        RebuildWork w = rebuild->work;                                   // list / other change places below: every update starts alike
        w.vertices = mesh->vertices;
        // 0: keys, the lists in id order, the root over every position
        if (rls_status s = launch_over(ctx, __func__, rebuild_init_kernel, w, nt)) return s;
        if (levels > 1) {
            // 1: the three lists sorted by (key, id), a digit a pass: count, scan, scatter
            RebuildSortIO sort = {};
            sort.counts = rebuild->counts; sort.tpa = rebuild->tpa; sort.tiles = 3 * rebuild->tpa;
            RebuildScanIO counts = {};
            counts.in = counts.out = rebuild->counts; counts.sums = rebuild->sums;
            counts.count = 3 * (int64_t)kRebuildDigits * rebuild->tpa;
            for (int pass = 0; pass < kRebuildPasses; pass++) {
                sort.w = w; sort.shift = pass * kRebuildDigitBits;
                hipLaunchKernelGGL(rebuild_sort_count_kernel, rlsh::grid_for(ctx, sort.tiles * kRebuildTile), dim3(rlsh::kBlock), 0, ctx->stream, sort);
                if (rls_status s = rlsh::check_launch(__func__)) return s;
                if (rls_status s = launch_scan(ctx, __func__, counts)) return s;
                hipLaunchKernelGGL(rebuild_sort_scatter_kernel, rlsh::grid_for(ctx, sort.tiles * kRebuildTile), dim3(rlsh::kBlock), 0, ctx->stream, sort);
                if (rls_status s = rlsh::check_launch(__func__)) return s;
                std::swap(w.list, w.other);
            }
            // 2: top-down, a level a round; the deepest level holds leaves alone
            for (int level = 1; level < levels; level++) {
                if (rls_status s = launch_over(ctx, __func__, rebuild_mark_kernel, w, nt)) return s;
                RebuildScanIO flags = {};
                flags.via = w.list; flags.flag = w.flag; flags.out = w.scan; flags.sums = rebuild->sums; flags.count = 3 * nt;
                if (rls_status s = launch_scan(ctx, __func__, flags)) return s;
                if (rls_status s = launch_over(ctx, __func__, rebuild_partition_kernel, w, nt)) return s;
                std::swap(w.list, w.other);
            }
        }
        // 3: the leaves' ids ascending into the records
        if (rls_status s = launch_over(ctx, __func__, rebuild_leaf_kernel, w, nodes)) return s;
        // 4: the refit's records and boxes, the deepest level first
        RefitRecordsIO io = {};
        io.tris = w.tris; io.index = w.index; io.vertices = mesh->vertices;
        io.parked = (unsigned long long *)mesh->parked;
        io.nt = nt; io.tiles = tiles_of(nt);
        hipLaunchKernelGGL(refit_records_kernel, rlsh::grid_for(ctx, nt), dim3(rlsh::kBlock), 0, ctx->stream, io);
        if (rls_status s = rlsh::check_launch(__func__)) return s;
        for (int l = 0; l < levels; l++) {
            RefitLevelIO lv = {};
            lv.nodes = w.nodes; lv.tris = w.tris; lv.list = rebuild->lists + rebuild->offset[(size_t)l];
            lv.count = rebuild->offset[(size_t)l + 1] - rebuild->offset[(size_t)l];
            lv.tiles = tiles_of(lv.count);
            hipLaunchKernelGGL(refit_level_kernel, rlsh::grid_for(ctx, lv.count), dim3(rlsh::kBlock), 0, ctx->stream, lv);
            if (rls_status s = rlsh::check_launch(__func__)) return s;
        }
    }
    if (mesh->normals && rebuild->info.nv > 0)
        RLS_HIP_TRY(hipMemcpyAsync(rebuild->normals, mesh->normals, (size_t)rebuild->info.nv * 3 * sizeof(float), hipMemcpyDeviceToDevice,
                                   ctx->stream));
    rebuild->info.updates++;
    return RLS_OK;
}

rls_status rls_nearest_rebuild_read_tree(rls_context *ctx, const rls_nearest_rebuild *rebuild, float *boxes, uint32_t *links, uint32_t *prims)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(rebuild != nullptr, "rebuild is NULL");
    RLS_REQUIRE(rebuild->device == ctx->device, "the rebuild's scene lives on another device than ctx");
    const int64_t nodes = rebuild->info.nodes, nt = rebuild->info.nt;
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
    if (!hn.empty()) RLS_HIP_TRY(hipMemcpy(hn.data(), rebuild->work.nodes, hn.size() * sizeof(NearestNode), hipMemcpyDeviceToHost));
    if (!ht.empty()) RLS_HIP_TRY(hipMemcpy(ht.data(), rebuild->work.tris, ht.size() * sizeof(NearestTri), hipMemcpyDeviceToHost));
    for (size_t n = 0; n < hn.size(); n++) {
        if (boxes)
            for (int c = 0; c < 3; c++) { boxes[6 * n + c] = hn[n].lo[c]; boxes[6 * n + 3 + c] = hn[n].hi[c]; }
        if (links) { links[2 * n] = hn[n].first; links[2 * n + 1] = hn[n].meta; }
    }
    for (size_t k = 0; k < ht.size(); k++) prims[k] = ht[k].prim;
    return RLS_OK;
}

} // extern "C"
