// group.hip -- instanced scenes (include/rlshaders_amd_nearest_group.h): the host side of librls_nearest_group.so -- a group's
// creation (the world boxes and the top tree on the host, one allocation, one upload), the argument checks (each written once),
// the one launch path of both queries, the update's launches, the read-back, the C ABI.  The maps, the boxes, both levels of the
// traversal and the kernels are in rls_nearest_group.hpp.
//
// An eighth companion beside librls_ggx_rr.so, librls_trace.so, librls_walk.so, librls_shadow_walk.so, librls_nearest.so,
// librls_nearest_refit.so and librls_nearest_rebuild.so, for the same reason: the other libraries' device code and surfaces stay
// what they are.  It reads a scene through rls_nearest_scene.hpp alone and calls nothing of librls_nearest.so.  Built once
// (rlshaders_amd/build.py, build_nearest_group_library): mode-free, one code object, compiled with RLS_FAST=0.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>

#include "../csrc/rls_internal.hpp"
#include "../../include/rlshaders_amd_nearest_group.h"

#if RLS_FAST
#error "group.hip has no FAST flavour"
#endif

#include "rls_nearest_scene.hpp"
#include "rls_nearest_group.hpp"

static_assert(kNearestStack == RLS_NEAREST_STACK && kGroupStack == RLS_NEAREST_GROUP_STACK, "the headers' stack sizes are the kernel's");
static_assert(sizeof(GroupInstance) == 96 && sizeof(GroupPlacement) == 160, "the records are whole 16-byte loads");
static_assert(kGroupTopLevels >= RLS_NEAREST_GROUP_STACK + 1, "the deepest top tree fits the single-workgroup launch's offsets");

// info and device lead the struct, as in the moving-mesh handles: the checks of update and read_tree read nothing else
struct rls_nearest_group {
    rls_nearest_group_info info;
    int device;
    void *blob;                   // the one device allocation: top nodes, records, placements, level lists
    NearestNode *top;
    GroupInstance *recs;          // [instances] in leaf order
    GroupPlacement *place;        // [instances] by instance
    uint32_t *lists;              // every top node once, deepest level first
    std::vector<int64_t> offset;  // [top_depth + 1] into lists
    int folded;                   // the last `folded` levels run in one single-workgroup launch; 0: none
};

namespace {

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline bool all3(rls_vec3 v) { return v.x && v.y && v.z; }
inline bool none3(rls_vec3 v) { return !v.x && !v.y && !v.z; }
inline int64_t tiles_of(int64_t count) { return (count + rlsh::kBlock - 1) / rlsh::kBlock; }

const char *const kLayoutText =
    "an instance's scene is not a scene of this build's layout (librls_nearest.so and librls_nearest_group.so must be of one build)";

rls_status out_of_host_memory(const char *fn)
{
    rlsh::set_error("%s: out of host memory", fn);
    return RLS_ERR_OUT_OF_MEMORY;
}

// ---- the argument checks, each written once; fn: the entry point its message names ---------------------------------------------
rls_status check_found(const char *fn, const rls_nearest_group_found *gf, int64_t rays)
{
    RLS_REQUIRE_IN(fn, gf != nullptr, "found is NULL");
    const rls_nearest_found *f = &gf->found;
    RLS_REQUIRE_IN(fn, rays == 0 || (f->hit != nullptr && f->t != nullptr), "found.hit or found.t plane is NULL");
    RLS_REQUIRE_IN(fn, (all3(f->P) || none3(f->P)) && (all3(f->N) || none3(f->N)) && (all3(f->Ns) || none3(f->Ns)) &&
                           (all3(f->T) || none3(f->T)) && (all3(f->wo) || none3(f->wo)),
                   "found.P, N, Ns, T or wo is partly NULL: all three planes or none");
    RLS_REQUIRE_IN(fn, f->bin == nullptr || (f->bin_of_surface != nullptr && f->bin_count >= 1),
                   "found.bin is set with found.bin_of_surface NULL or found.bin_count == 0");
    RLS_REQUIRE_IN(fn, (f->last != nullptr) == (gf->last_instance != nullptr),
                   "found.last and last_instance are a pair: both or neither");
    return RLS_OK;
}

// the one launch path: both queries arrive here with their rays in one struct
rls_status launch(const char *fn, rls_context *ctx, const rls_nearest_group *group, const rls_nearest_rays &r,
                  const rls_nearest_group_found *f)
{
    RLS_REQUIRE_IN(fn, r.rays >= 0, "rays < 0");
    RLS_REQUIRE_IN(fn, r.rays <= (int64_t)UINT32_MAX, "rays > 2^32 - 1 (a ray id is 32-bit)");
    RLS_REQUIRE_IN(fn, r.rays == 0 || (rlsh::has3(r.origin) && rlsh::has3(r.dir)), "rays.origin or rays.dir plane is NULL");
    if (rls_status s = check_found(fn, f, r.rays)) return s;
    if (r.rays == 0) return RLS_OK;
    RLS_REQUIRE_IN(fn, group->device == ctx->device, "the group lives on another device than ctx");
    GroupIO io = {};
    io.top = group->top; io.recs = group->recs; io.place = group->place; io.top_count = group->info.top_nodes;
    io.r = r; io.f = f->found; io.instance = f->instance; io.last_instance = f->last_instance;
    io.tiles = tiles_of(r.rays);
    hipLaunchKernelGGL(group_kernel, rlsh::grid_for(ctx, r.rays), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(fn);
}

} // namespace

extern "C" {

rls_status rls_nearest_group_create(rls_context *ctx, const rls_nearest_instance *instances, int64_t count, int leaf_size,
                                    rls_nearest_group **out)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    RLS_REQUIRE(count >= 0, "count < 0");
    RLS_REQUIRE(count <= RLS_NEAREST_GROUP_MAX_INSTANCES, "count > 2^16: the top stack of 16 entries bounds the top tree's depth");
    RLS_REQUIRE(leaf_size >= 0 && leaf_size <= RLS_NEAREST_GROUP_MAX_LEAF, "leaf_size must be in [1, 4], or 0 for the default");
    RLS_REQUIRE(count == 0 || instances != nullptr, "instances is NULL");
    for (int64_t j = 0; j < count; j++) {
        RLS_REQUIRE(instances[j].scene != nullptr, "an instance's scene is NULL");
        RLS_REQUIRE(instances[j].scene->layout == kNearestSceneLayout, kLayoutText);
        RLS_REQUIRE(instances[j].scene->device == ctx->device, "an instance's scene lives on another device than ctx");
    }
    const int leaf = leaf_size ? leaf_size : RLS_NEAREST_GROUP_DEFAULT_LEAF;

    std::unique_ptr<rls_nearest_group> g;
    std::vector<const rls_nearest_scene *> scenes;                       // the distinct ones, sorted
    std::vector<NearestNode> roots;                                      // their root nodes
    std::vector<GroupPlacement> place;
    std::vector<GroupInstance> recs;
    std::vector<float> world;
    std::vector<uint32_t> order, list;
    std::vector<char> host;
    NearestBvh bvh;
    size_t o_top = 0, o_recs = 0, o_place = 0, o_lists = 0, bytes = 0;
    try {
        g.reset(new rls_nearest_group());
        g->offset.assign(1, 0);
        for (int64_t j = 0; j < count; j++) scenes.push_back(instances[j].scene);
        std::sort(scenes.begin(), scenes.end());
        scenes.erase(std::unique(scenes.begin(), scenes.end()), scenes.end());
        roots.resize(scenes.size());
        place.resize((size_t)count);
        recs.resize((size_t)count);
        world.resize(6 * (size_t)count);
    } catch (const std::bad_alloc &) {
        return out_of_host_memory(__func__);
    }
    // the root boxes as they are on the device now: a refit or a rebuild of a member scene may be in flight on the stream
    if (!scenes.empty()) {
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        for (size_t s = 0; s < scenes.size() && e == hipSuccess; s++)
            if (scenes[s]->info.nodes > 0) e = hipMemcpy(&roots[s], scenes[s]->nodes, sizeof(NearestNode), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return rlsh::hip_fail(e, "rls_nearest_group_create: the root boxes' download");
    }
    for (int64_t j = 0; j < count; j++) {
        const rls_nearest_scene *sc = instances[j].scene;
        GroupPlacement &p = place[(size_t)j];
        p = GroupPlacement();
        memcpy(p.A, instances[j].to_object, sizeof p.A);
        memcpy(p.B, instances[j].to_world, sizeof p.B);
        p.nodes = sc->nodes; p.tris = sc->tris; p.index = sc->index; p.surface = sc->surface; p.normals = sc->normals;
        p.node_count = (uint32_t)sc->info.nodes;
        p.surface_base = instances[j].surface_base;
        const NearestNode &root = roots[(size_t)(std::lower_bound(scenes.begin(), scenes.end(), sc) - scenes.begin())];
        float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 0.0f, 0.0f, 0.0f };
        if (p.node_count)
            for (int c = 0; c < 3; c++) { lo[c] = root.lo[c]; hi[c] = root.hi[c]; }
        GroupInstance rec;
        group_record(p, lo, hi, (uint32_t)j, rec);
        for (int c = 0; c < 3; c++) { world[6 * (size_t)j + c] = rec.lo[c]; world[6 * (size_t)j + 3 + c] = rec.hi[c]; }
        recs[(size_t)j] = rec;                                           // by instance for now
    }
    bool tree = true;
    try {
        group_build(world.data(), count, leaf, bvh, order);
        tree = refit_levels(bvh.nodes.data(), (int64_t)bvh.nodes.size(), count, list, g->offset);
        auto carve = [&](size_t b) { const size_t at = bytes; bytes += align256(b); return at; };
        o_top = carve(bvh.nodes.size() * sizeof(NearestNode));
        o_recs = carve((size_t)count * sizeof(GroupInstance));
        o_place = carve((size_t)count * sizeof(GroupPlacement));
        o_lists = carve(bvh.nodes.size() * sizeof(uint32_t));
        host.assign(bytes, 0);
    } catch (const std::bad_alloc &) {
        return out_of_host_memory(__func__);
    }
    // one sibling per inner level: a top tree of `depth` levels needs depth - 1 stack entries
    if (!tree || bvh.depth - 1 > RLS_NEAREST_GROUP_STACK || bvh.depth > nearest_depth_bound(count, leaf) ||
        (int64_t)g->offset.size() - 1 != bvh.depth) {
        rlsh::set_error("%s: the top tree is deeper than its bound", __func__);
        return RLS_ERR_UNSUPPORTED;
    }
    g->device = ctx->device;
    g->info.instances = count; g->info.scenes = (int64_t)scenes.size(); g->info.top_nodes = (int64_t)bvh.nodes.size();
    g->info.top_depth = bvh.depth; g->info.leaf_size = leaf; g->info.device_bytes = bytes;
    if (count > 0) {
        memcpy(host.data() + o_top, bvh.nodes.data(), bvh.nodes.size() * sizeof(NearestNode));
        GroupInstance *hr = (GroupInstance *)(host.data() + o_recs);
        for (size_t k = 0; k < (size_t)count; k++) {
            hr[k] = recs[order[k]];
            place[order[k]].slot = (uint32_t)k;
        }
        memcpy(host.data() + o_place, place.data(), (size_t)count * sizeof(GroupPlacement));
        memcpy(host.data() + o_lists, list.data(), list.size() * sizeof(uint32_t));
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipMalloc(&g->blob, bytes);
        if (e == hipSuccess) {
            e = hipMemcpy(g->blob, host.data(), bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) (void)hipFree(g->blob);
        }
        if (e != hipSuccess) return rlsh::hip_fail(e, "rls_nearest_group_create: the group's upload");
        char *d = (char *)g->blob;
        g->top = (NearestNode *)(d + o_top);
        g->recs = (GroupInstance *)(d + o_recs);
        g->place = (GroupPlacement *)(d + o_place);
        g->lists = (uint32_t *)(d + o_lists);
        // the top of the tree: the trailing levels of at most kBlock nodes each; one level alone gains nothing
        const int levels = bvh.depth;
        int folded = 0;
        while (folded < levels && g->offset[(size_t)(levels - folded)] - g->offset[(size_t)(levels - folded - 1)] <= rlsh::kBlock) folded++;
        g->folded = folded >= 2 ? folded : 0;
    }
    *out = g.release();
    return RLS_OK;
}

rls_status rls_nearest_group_destroy(rls_nearest_group *group)
{
    if (!group) return RLS_OK;
    hipError_t e = hipSuccess;
    if (group->blob) {
        e = hipSetDevice(group->device);
        if (e == hipSuccess) e = hipFree(group->blob);
    }
    delete group;
    if (e != hipSuccess) return rlsh::hip_fail(e, "rls_nearest_group_destroy");
    return RLS_OK;
}

rls_status rls_nearest_group_get_info(const rls_nearest_group *group, rls_nearest_group_info *info)
{
    RLS_REQUIRE(group != nullptr, "group is NULL");
    RLS_REQUIRE(info != nullptr, "info is NULL");
    *info = group->info;
    return RLS_OK;
}

rls_status rls_nearest_group_update(rls_context *ctx, rls_nearest_group *group, const rls_nearest_group_moves *moves)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(group != nullptr, "group is NULL");
    RLS_REQUIRE(moves != nullptr, "moves is NULL");
    RLS_REQUIRE((moves->to_object != nullptr) == (moves->to_world != nullptr), "moves.to_object and moves.to_world: both planes or neither");
    RLS_REQUIRE(group->device == ctx->device, "the group lives on another device than ctx");
    const int64_t count = group->info.instances;
    if (moves->parked) {
        RLS_HIP_TRY(hipSetDevice(ctx->device));
        RLS_HIP_TRY(hipMemsetAsync(moves->parked, 0, sizeof(int64_t), ctx->stream));
    }
    if (count > 0) {
        GroupRecordsIO io = {};
        io.recs = group->recs; io.place = group->place; io.to_object = moves->to_object; io.to_world = moves->to_world;
        io.parked = (unsigned long long *)moves->parked;
        io.count = count; io.tiles = tiles_of(count);
        hipLaunchKernelGGL(group_records_kernel, rlsh::grid_for(ctx, count), dim3(rlsh::kBlock), 0, ctx->stream, io);
        if (rls_status s = rlsh::check_launch(__func__)) return s;
        const int wide = group->info.top_depth - group->folded;          // levels launched one by one, deepest first
        for (int l = 0; l < wide; l++) {
            GroupLevelIO lv = {};
            lv.top = group->top; lv.recs = group->recs; lv.list = group->lists + group->offset[(size_t)l];
            lv.count = group->offset[(size_t)l + 1] - group->offset[(size_t)l];
            lv.tiles = tiles_of(lv.count);
            hipLaunchKernelGGL(group_level_kernel, rlsh::grid_for(ctx, lv.count), dim3(rlsh::kBlock), 0, ctx->stream, lv);
            if (rls_status s = rlsh::check_launch(__func__)) return s;
        }
        if (group->folded) {
            GroupTopIO top = {};
            top.top = group->top; top.recs = group->recs; top.list = group->lists + group->offset[(size_t)wide];
            top.levels = group->folded;
            for (int l = 0; l <= group->folded; l++) top.offset[l] = (uint32_t)(group->offset[(size_t)(wide + l)] - group->offset[(size_t)wide]);
            (void)rlsh::grid_for(ctx, 1);                                // the device made current, as ahead of every launch
            hipLaunchKernelGGL(group_top_kernel, dim3(1), dim3(rlsh::kBlock), 0, ctx->stream, top);
            if (rls_status s = rlsh::check_launch(__func__)) return s;
        }
    }
    group->info.updates++;
    return RLS_OK;
}

rls_status rls_nearest_group_hits(rls_context *ctx, const rls_nearest_group *group, const rls_nearest_rays *rays,
                                  const rls_nearest_group_found *found)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(group != nullptr, "group is NULL");
    RLS_REQUIRE(rays != nullptr, "rays is NULL");
    return launch(__func__, ctx, group, *rays, found);
}

rls_status rls_nearest_group_walk_hits(rls_context *ctx, const rls_nearest_group *group, const rls_walk_rays *list, int64_t bound,
                                       const rls_nearest_group_found *found)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(group != nullptr, "group is NULL");
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
    return launch(__func__, ctx, group, r, found);
}

rls_status rls_nearest_group_read_tree(rls_context *ctx, const rls_nearest_group *group, float *boxes, uint32_t *links,
                                       uint32_t *order, float *world, uint8_t *parked)
{
    RLS_REQUIRE(ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE(group != nullptr, "group is NULL");
    RLS_REQUIRE(group->device == ctx->device, "the group lives on another device than ctx");
    const int64_t nodes = group->info.top_nodes, count = group->info.instances;
    if (count == 0 || (!boxes && !links && !order && !world && !parked)) return RLS_OK;
    std::vector<NearestNode> hn;
    std::vector<GroupInstance> hr;
    try {
        if (boxes || links) hn.resize((size_t)nodes);
        if (order || world || parked) hr.resize((size_t)count);
    } catch (const std::bad_alloc &) {
        return out_of_host_memory(__func__);
    }
    RLS_HIP_TRY(hipSetDevice(ctx->device));
    RLS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!hn.empty()) RLS_HIP_TRY(hipMemcpy(hn.data(), group->top, hn.size() * sizeof(NearestNode), hipMemcpyDeviceToHost));
    if (!hr.empty()) RLS_HIP_TRY(hipMemcpy(hr.data(), group->recs, hr.size() * sizeof(GroupInstance), hipMemcpyDeviceToHost));
    for (size_t n = 0; n < hn.size(); n++) {
        if (boxes)
            for (int c = 0; c < 3; c++) { boxes[6 * n + c] = hn[n].lo[c]; boxes[6 * n + 3 + c] = hn[n].hi[c]; }
        if (links) { links[2 * n] = hn[n].first; links[2 * n + 1] = hn[n].meta; }
    }
    for (size_t k = 0; k < hr.size(); k++) {
        const size_t j = hr[k].instance;
        if (order) order[k] = hr[k].instance;
        if (world)
            for (int c = 0; c < 3; c++) { world[6 * j + c] = hr[k].lo[c]; world[6 * j + 3 + c] = hr[k].hi[c]; }
        if (parked) parked[j] = hr[k].node_count == 0;
    }
    return RLS_OK;
}

} // extern "C"
