// rebuild.hip -- rebuilding a scene's tree on the device (include/rlshaders_amd_nearest_rebuild.h): the host side of
// librls_nearest_rebuild.so -- the rebuild's handle, what its creation adds to the common part (the nodes held to the builder's
// shape; the per-node ranges, the per-level node lists and the update's working set in ONE allocation), what its update adds
// (steps 0 to 3), and the C ABI.  The algorithm, its one-element functions and the kernels are in rls_nearest_rebuild.hpp; the
// records and the boxes are the refit's (rls_nearest_refit.hpp), included there; the host layer both libraries state once (the
// scene's view, the common part of a creation, the mesh checks, the update's frame, the read-back) is rls_nearest_update.hpp.
//
// A seventh companion beside librls_ggx_rr.so, librls_trace.so, librls_walk.so, librls_shadow_walk.so, librls_nearest.so and
// librls_nearest_refit.so, for the same reason: the other libraries' device code and surfaces stay what they are.  It reads a
// scene through rls_nearest_scene.hpp alone and calls nothing of the two other nearest libraries.  Built once
// (rlshaders_amd/build.py, build_nearest_rebuild_library): mode-free, one code object, compiled with RLS_FAST=0.
#include <utility>

#include "../csrc/rls_internal.hpp"
#include "../../include/rlshaders_amd_nearest_rebuild.h"

#if RLS_FAST
#error "rebuild.hip has no FAST flavour"
#endif

#include "rls_nearest_scene.hpp"
#include "rls_nearest_rebuild.hpp"
#include "rls_nearest_update.hpp"

static_assert(kRebuildMaxLeaf == RLS_NEAREST_MAX_LEAF, "a leaf's ids fit the leaf kernel's registers");
static_assert(3 * RLS_NEAREST_MAX_TRIANGLES < ((int64_t)1 << 32), "a position in the three lists fits 32 bits");

// info and device lead the struct: the update's checks read nothing else, so tests/test_nearest_rebuild_abi.py can lay the
// public info struct over dummy memory and reach every refusal without a device
struct rls_nearest_rebuild {
    rls_nearest_rebuild_info info;
    int device;
    rls_nearest_scene *scene;     // borrowed
    SceneView view;               // the scene's blob, writable
    void *blob;                   // the rebuild's one device allocation
    RebuildWork work;             // its parts and the view's nodes, tris and index (vertices: an update's)
    uint32_t *lists;              // every node once, deepest level first (refit_levels)
    uint32_t *counts, *sums;      // the sort's [3][digits][tpa] counts; a scan's tile sums
    int64_t tpa;                  // tiles of one list
    std::vector<int64_t> offset;  // [levels + 1] into lists
};

namespace {

// what the shared layer reports in this library's words: the layout refusal, three HIP calls as a failure has always named them
const UpdateTexts kTexts = {
    "scene is not a scene of this build's layout (librls_nearest.so and librls_nearest_rebuild.so must be of one build)",
    "hipMemcpyAsync(rebuild->normals, mesh->normals, (size_t)rebuild->info.nv * 3 * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream)",
    "hipMemcpy(hn.data(), rebuild->work.nodes, hn.size() * sizeof(NearestNode), hipMemcpyDeviceToHost)",
    "hipMemcpy(ht.data(), rebuild->work.tris, ht.size() * sizeof(NearestTri), hipMemcpyDeviceToHost)"};

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
    std::vector<NearestNode> host;
    std::vector<uint32_t> list;
    std::vector<RebuildRange> range;
    std::unique_ptr<rls_nearest_rebuild> r;
    bool tree = false;
    if (rls_status s = begin_create(__func__, kTexts, ctx, scene, out, r, host, list, tree)) return s;
    const int64_t nodes = r->info.nodes, nt = r->info.nt;
    r->info.leaf_size = scene->info.leaf_size;
    if (nodes > 0) {
        try {
            tree = tree && nt <= RLS_NEAREST_MAX_TRIANGLES && rebuild_shape(host.data(), nodes, nt, scene->info.leaf_size, range);
        } catch (const std::bad_alloc &) {
            return out_of_host_memory(__func__);
        }
        if (!tree) {
            rlsh::set_error("%s: the scene's nodes are not the builder's tree of its triangle count and leaf size", __func__);
            return RLS_ERR_UNSUPPORTED;
        }
        RebuildWork &w = r->work;
        w.nodes = r->view.nodes; w.tris = r->view.tris; w.index = r->view.index;
        w.nt = (uint32_t)nt; w.leaf = (uint32_t)scene->info.leaf_size;
        r->tpa = tiles_of(nt);
        const int64_t count_entries = 3 * (int64_t)kRebuildDigits * r->tpa;
        const int64_t sum_entries = std::max(tiles_of(3 * nt), tiles_of(count_entries));
        // the parts of the one allocation, each on a 256-byte boundary
        const size_t b_range = aligned((size_t)nodes * sizeof(RebuildRange)), b_lists = aligned((size_t)nodes * sizeof(uint32_t));
        const size_t b_plane = aligned(3 * (size_t)nt * sizeof(uint32_t)), b_at = aligned((size_t)nt * sizeof(uint32_t));
        const size_t b_flag = aligned((size_t)nt), b_counts = aligned((size_t)count_entries * sizeof(uint32_t));
        const size_t b_sums = aligned((size_t)sum_entries * sizeof(uint32_t));
        const size_t bytes = b_range + b_lists + 4 * b_plane + b_at + b_flag + b_counts + b_sums;
        hipError_t e = hipMalloc(&r->blob, bytes);
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
        if (e != hipSuccess) return rlsh::hip_fail(e, "rls_nearest_rebuild_create: the working set");
        r->info.device_bytes = bytes;
    }
    *out = r.release();
    return RLS_OK;
}

rls_status rls_nearest_rebuild_destroy(rls_nearest_rebuild *rebuild)
{
    return destroy_handle(__func__, rebuild, &rls_nearest_rebuild::blob);
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
    const char *fn = __func__;
    // steps 0 to 3 ahead of the shared 4: the refit's records and boxes, the deepest level first, a launch a level
    return update_mesh(fn, kTexts, ctx, rebuild, mesh, 0, [&]() -> rls_status {
        RebuildWork w = rebuild->work;                                   // list / other change places below: every update starts alike
        w.vertices = mesh->vertices;
        // 0: keys, the lists in id order, the root over every position
        if (rls_status s = launch_over(ctx, fn, rebuild_init_kernel, w, nt)) return s;
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
                if (rls_status s = rlsh::check_launch(fn)) return s;
                if (rls_status s = launch_scan(ctx, fn, counts)) return s;
                hipLaunchKernelGGL(rebuild_sort_scatter_kernel, rlsh::grid_for(ctx, sort.tiles * kRebuildTile), dim3(rlsh::kBlock), 0, ctx->stream, sort);
                if (rls_status s = rlsh::check_launch(fn)) return s;
                std::swap(w.list, w.other);
            }
            // 2: top-down, a level a round; the deepest level holds leaves alone
            for (int level = 1; level < levels; level++) {
                if (rls_status s = launch_over(ctx, fn, rebuild_mark_kernel, w, nt)) return s;
                RebuildScanIO flags = {};
                flags.via = w.list; flags.flag = w.flag; flags.out = w.scan; flags.sums = rebuild->sums; flags.count = 3 * nt;
                if (rls_status s = launch_scan(ctx, fn, flags)) return s;
                if (rls_status s = launch_over(ctx, fn, rebuild_partition_kernel, w, nt)) return s;
                std::swap(w.list, w.other);
            }
        }
        // 3: the leaves' ids ascending into the records
        return launch_over(ctx, fn, rebuild_leaf_kernel, w, nodes);
    });
}

rls_status rls_nearest_rebuild_read_tree(rls_context *ctx, const rls_nearest_rebuild *rebuild, float *boxes, uint32_t *links, uint32_t *prims)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(rebuild != nullptr, "rebuild is NULL");
    RLS_REQUIRE(rebuild->device == ctx->device, "the rebuild's scene lives on another device than ctx");
    return read_tree(__func__, kTexts, ctx, rebuild->info.nodes, rebuild->info.nt, rebuild->view, boxes, links, prims);
}

} // extern "C"
