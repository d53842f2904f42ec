// rls_nearest_any.hpp -- the any-hit query of librls_nearest_any.so (include/rlshaders_amd_nearest_any.h): a triangle's class,
// the candidate predicate, the statement as a brute force, the traversal, each written once as host + device functions, and
// (under hipcc) the two kernels around them.  tests/native/nearest_any_host_check.cpp compiles the same functions for the CPU
// and holds the traversal to the brute force in state, for every ray.
//
// The ray, the slab test and the triangle test are those of rls_nearest_device.hpp, included here without its kernel; the node
// and triangle records are those of rls_nearest_bvh.hpp.  nearest_candidate and nearest_traverse are not used: they keep a best.
//
// float32 throughout, every operation by itself (-ffp-contract=off), / and sqrt correctly rounded.
#ifndef RLS_NEAREST_ANY_HPP
#define RLS_NEAREST_ANY_HPP

#define RLS_NEAREST_DEVICE_NO_KERNEL 1
#include "rls_nearest_device.hpp"

constexpr uint32_t kAnyClear = 0u, kAnyBlocked = 1u, kAnyVeiled = 2u;   // RLS_NEAREST_ANY_CLEAR, _BLOCKED, _VEILED

// The classes of a mesh's triangles: surface [nt] or NULL (every surface 0), flags [count] or NULL (every triangle opaque).
struct AnyClasses {
    const uint32_t *surface;
    const uint8_t *flags;
    uint32_t count;                                   // >= 1 with flags
};

// opaque_i: 1 without a table, else flags[min(surface_i, count - 1)] != 0 -- the clamp of rls_shadow_walk_found.index
RLS_NEAREST_HD bool any_opaque(const AnyClasses &c, uint32_t prim)
{
    if (!c.flags) return true;
    const uint32_t s = c.surface ? c.surface[prim] : 0u;
    return c.flags[s < c.count ? s : c.count - 1] != 0;
}

// The statement's candidate rule for one triangle record (nearest_candidate without its order: there is no best here).  Every
// clause is evaluated and the answers are joined at the end: the same truth value as nearest_candidate's early returns give, with
// one level of divergence in a leaf's loop instead of five.
RLS_NEAREST_HD bool any_candidate(const NearestTri &tr, const NearestRay &r)
{
    float lo[3], hi[3], tn, tf, tm = 0.0f, u = 0.0f, v = 0.0f;
    for (int c = 0; c < 3; c++) {
        lo[c] = nearest_minf(nearest_minf(tr.v0[c], tr.v1[c]), tr.v2[c]);
        hi[c] = nearest_maxf(nearest_maxf(tr.v0[c], tr.v1[c]), tr.v2[c]);
    }
    const bool box = nearest_slab(lo, hi, r, tn, tf);
    const bool hit = nearest_triangle(tr.v0, tr.v1, tr.v2, r, tm, u, v);
    float t = tm;
    if (tn > t) t = tn;
    if (tf < t) t = tf;
    return (tr.prim != r.skip) & box & hit & (t > 0.0f) & (t <= r.m);
}

// blocked iff some candidate is opaque, else veiled iff there is a candidate, else clear
RLS_NEAREST_HD uint32_t any_state(bool blocked, bool veiled) { return blocked ? kAnyBlocked : veiled ? kAnyVeiled : kAnyClear; }

// the statement itself: every triangle, no tree, no early end
RLS_NEAREST_HD uint32_t any_brute(const NearestTri *tris, int64_t nt, const AnyClasses &cls, const NearestRay &r)
{
    bool blocked = false, veiled = false;
    for (int64_t k = 0; k < nt; k++) {
        if (!any_candidate(tris[k], r)) continue;
        if (any_opaque(cls, tris[k].prim)) blocked = true;
        else veiled = true;
    }
    return any_state(blocked, veiled);
}

// The traversal.  stack(i): a reference to the lane's i-th stack word, as nearest_traverse takes it; the loop bound on `visits`
// and the guard on `sp` are nearest_traverse's, for its reasons: every node is visited at most once, and the stack holds one
// sibling per inner level.
//
// THE CULL, and why it is exact: the argument written at nearest_traverse (rls_nearest_device.hpp), as far as it needs no best.
// A node is skipped only when its box fails -- part (1) of that argument: it holds no triangle whose box passes, so no
// candidate -- or when its tn > m -- the m half of part (2): every candidate below it has t_i >= tn_i >= tn_node > m, and a
// candidate has t_i <= m.  There is no cull against a best t because there is no best: the state is two existence statements
// over the candidate set, and every candidate lies under nodes this loop opens.  A lane returns at the first OPAQUE candidate
// (blocked holds whatever else there is); a translucent candidate sets a bit and the lane goes on, since an opaque one may
// follow anywhere in the tree.  The compare with m is strict and a NaN reach culls nothing (and admits no candidate).  Which
// child goes first -- the one on the ray's side of the split axis -- changes the work and which opaque candidate ends the
// lane, never the state; that is why no primitive is reported.
//
// kTable: the caller has seen a flag table.  Without one every candidate is opaque and the loop reads neither a surface nor a
// flag; the two bodies are chosen once a ray (any_traverse below), which also keeps the table's registers out of the other body.
template <bool kTable, class Stack, class Stats>
RLS_NEAREST_HD uint32_t any_traverse_as(const NearestNode *nodes, int64_t node_count, const NearestTri *tris, const AnyClasses &cls,
                                        const NearestRay &r, Stack &&stack, Stats &stats)
{
    bool veiled = false;
    if (node_count <= 0) return kAnyClear;
    uint32_t node = 0;
    int sp = 0;
    for (int64_t visits = 0; visits < node_count; visits++) {
        const NearestNode n = nodes[node];
        nearest_count_node(stats);
        float tn, tf;
        bool open = nearest_slab(n.lo, n.hi, r, tn, tf);
        if (tn > r.m) open = false;
        if (open) {
            const uint32_t count = n.meta & kNearestCountMask;
            if (count == 0) {
                const uint32_t axis = n.meta >> kNearestAxisShift;
                const float da = axis == 0 ? r.d[0] : axis == 1 ? r.d[1] : r.d[2];
                const uint32_t near = nearest_sign(da) ? 1u : 0u;      // a heuristic only
                if (sp < kNearestStack) {
                    stack(sp++) = n.first + (1u - near);
                    nearest_count_push(stats, sp);
                }
                node = n.first + near;
                continue;
            }
            for (uint32_t k = 0; k < count; k++) {
                nearest_count_tri(stats);
                const NearestTri tr = tris[n.first + k];
                if (!any_candidate(tr, r)) continue;
                if (!kTable || any_opaque(cls, tr.prim)) return kAnyBlocked;
                veiled = true;
            }
        }
        if (sp == 0) break;
        node = stack(--sp);
    }
    return any_state(false, veiled);
}
template <class Stack, class Stats>
RLS_NEAREST_HD uint32_t any_traverse(const NearestNode *nodes, int64_t node_count, const NearestTri *tris, const AnyClasses &cls,
                                     const NearestRay &r, Stack &&stack, Stats &stats)
{
    return cls.flags ? any_traverse_as<true>(nodes, node_count, tris, cls, r, stack, stats)
                     : any_traverse_as<false>(nodes, node_count, tris, cls, r, stack, stats);
}

// flags[s] of an opacity entry: every channel exactly 1 (IEEE compares: a NaN gives 0)
RLS_NEAREST_HD uint8_t any_flag(float r, float g, float b) { return (r == 1.0f && g == 1.0f && b == 1.0f) ? 1 : 0; }

#if defined(__HIPCC__)
// ---- the kernels: one ray per lane over the companions' tile skeleton ----------------------------------------------------------
struct AnyIO {
    const NearestNode *nodes;
    const NearestTri *tris;
    AnyClasses cls;
    int64_t node_count;
    rls_nearest_rays r;
    rls_nearest_any_found f;
    int64_t tiles;
};

__global__ __launch_bounds__(rlsh::kBlock) void any_kernel(AnyIO a)
{
    // the lanes' stacks as nearest_kernel lays them out, word i of lane l at [i][l]: no bank conflict, no scratch memory
    __shared__ uint32_t stacks[kNearestStack][rlsh::kBlock];
    int64_t bound = a.r.rays;
    if (a.r.count) {
        const int64_t c = *a.r.count;
        bound = c < 0 ? 0 : c < bound ? c : bound;
    }
    const uint32_t m = (uint32_t)bound, tiles = (uint32_t)a.tiles;   // rays <= 2^32 - 1: the host layer refuses more
    // which optional planes there are, one bit each.  The bits are tested inside the tile loop through an empty asm: hoisted out of
    // it, every test would hold a lane mask in two scalar registers across the traversal, more than the register file has
    const uint32_t planes = (a.r.via ? 1u : 0u) | (a.r.maxdist ? 2u : 0u) | (a.r.ray ? 4u : 0u) | (a.f.last ? 8u : 0u) |
                            (a.f.visibility.r ? 16u : 0u) | (a.f.base.r ? 32u : 0u) | (a.f.reach ? 64u : 0u);
    const unsigned lane = threadIdx.x;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t k = tile * rlsh::kBlock + lane;               // below 2^32: tile < ceil(rays / kBlock)
        if (k >= m) continue;                                        // (no barrier in this kernel)
        uint32_t has = planes;
        asm volatile("" : "+s"(has));
        const int64_t from = (has & 1u) ? (int64_t)a.r.via[k] : (int64_t)k;
        const float o[3] = { a.r.origin.x[from], a.r.origin.y[from], a.r.origin.z[from] };
        const float d[3] = { a.r.dir.x[k], a.r.dir.y[k], a.r.dir.z[k] };
        const int64_t id = (has & 4u) ? (int64_t)a.r.ray[k] : (int64_t)k;
        const float reach = (has & 2u) ? a.r.maxdist[k] : __builtin_inff();
        const NearestRay r = nearest_ray(o, d, reach, (has & 8u) ? a.f.last[id] : kNearestNoPrim);
        NearestNoStats none;
        const uint32_t state = any_traverse(a.nodes, a.node_count, a.tris, a.cls, r,
                                            [&](int i) -> uint32_t & { return stacks[i][lane]; }, none);
        a.f.state[k] = (uint8_t)state;
        if (has & 16u) {
            // base may alias visibility plane for plane: each entry is read before it is written, by the lane that writes it
            float b[3] = { 1.0f, 1.0f, 1.0f };
            if (has & 32u) { b[0] = a.f.base.r[id]; b[1] = a.f.base.g[id]; b[2] = a.f.base.b[id]; }
            const bool blocked = state == kAnyBlocked;
            a.f.visibility.r[id] = blocked ? b[0] * 0.0f : b[0];
            a.f.visibility.g[id] = blocked ? b[1] * 0.0f : b[1];
            a.f.visibility.b[id] = blocked ? b[2] * 0.0f : b[2];
        }
        if (has & 64u) a.f.reach[id] = state == kAnyVeiled ? reach : 0.0f;
    }
}

struct AnyFlagsIO {
    rls_crgb opacity;
    uint8_t *flags;
    int64_t count, tiles;
};

__global__ __launch_bounds__(rlsh::kBlock) void any_flags_kernel(AnyFlagsIO a)
{
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t s = tile * rlsh::kBlock + threadIdx.x;
        if (s < a.count) a.flags[s] = any_flag(a.opacity.r[s], a.opacity.g[s], a.opacity.b[s]);
    }
}
#endif // __HIPCC__

#endif
