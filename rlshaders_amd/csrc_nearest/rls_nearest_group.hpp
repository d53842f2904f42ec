// rls_nearest_group.hpp -- the two-level nearest-hit query of librls_nearest_group.so (include/rlshaders_amd_nearest_group.h):
// the matrix maps, an instance's world box and record, the slab test from a given interval, the candidate rule, both levels of
// the traversal, a hit's frame and the top tree's boxes, each written once as host + device functions, and (under hipcc) the
// kernels around them.  tests/native/nearest_group_host_check.cpp compiles the same functions for the CPU and holds the
// traversal to a brute force over the statement, bit for bit.
//
// The triangle test, the slab test from [0, +inf), the dot and cross products and the normalisation are those of
// rls_nearest_device.hpp, included here without its kernel; the node and triangle records are those of rls_nearest_bvh.hpp, and
// the top tree is a tree of the same nodes whose leaves hold instance records.
//
// float32 throughout, every operation by itself (-ffp-contract=off), / and sqrt correctly rounded.
#ifndef RLS_NEAREST_GROUP_HPP
#define RLS_NEAREST_GROUP_HPP

#define RLS_NEAREST_DEVICE_NO_KERNEL 1
#include "rls_nearest_device.hpp"
#define RLS_NEAREST_REFIT_NO_KERNELS 1
#include "rls_nearest_refit.hpp"                      // refit_finite, refit_union, refit_levels

constexpr int kGroupStack = 16;                       // RLS_NEAREST_GROUP_STACK: top node indices a lane can hold
constexpr uint32_t kGroupNoInstance = 0xFFFFFFFFu;
constexpr float kGroupPad = 4.76837158203125e-07f;    // 2^-21

// An instance as the traversal reads it, 96 bytes, six 16-byte loads, in the top tree's leaf order so that a leaf reads
// consecutive records: the world box with the instance's id and its scene's node count beside it (0: PARKED -- the box is then
// the point at the origin), to_object, the scene's nodes and triangle records.
struct alignas(16) GroupInstance {
    float lo[3];
    uint32_t instance;
    float hi[3];
    uint32_t node_count;
    float A[12];
    const NearestNode *nodes;
    const NearestTri *tris;
};
// An instance as the update and a hit's report read it, by instance id: both matrices, the scene's parts, where its record is.
struct alignas(16) GroupPlacement {
    float A[12], B[12];
    const NearestNode *nodes;
    const NearestTri *tris;
    const uint32_t *index, *surface;
    const float *normals;
    uint32_t node_count;                              // the scene's; 0: an empty scene
    uint32_t surface_base;
    uint32_t slot;                                    // its GroupInstance
    uint32_t pad;
};

struct GroupRay {
    NearestRay w;                                     // the world ray; w.skip: the triangle to skip in skip_instance
    uint32_t skip_instance;
};
struct GroupBest {
    float t, u, v;
    uint32_t prim, slot;                              // slot: the winner's triangle record in its scene
    uint32_t instance;                                // kGroupNoInstance: no candidate yet
};
// per ray: top nodes, instances entered, object nodes, triangles; the most entries either stack held at once
struct GroupStats { int64_t top_nodes = 0, instances = 0, nodes = 0, tris = 0; int max_top = 0, max_stack = 0; };
struct GroupNoStats {};
RLS_NEAREST_HD void group_count_top(GroupStats &s) { s.top_nodes++; }
RLS_NEAREST_HD void group_count_instance(GroupStats &s) { s.instances++; }
RLS_NEAREST_HD void group_count_top_push(GroupStats &s, int held) { if (held > s.max_top) s.max_top = held; }
RLS_NEAREST_HD void nearest_count_node(GroupStats &s) { s.nodes++; }
RLS_NEAREST_HD void nearest_count_tri(GroupStats &s) { s.tris++; }
RLS_NEAREST_HD void nearest_count_push(GroupStats &s, int held) { if (held > s.max_stack) s.max_stack = held; }
RLS_NEAREST_HD void group_count_top(GroupNoStats &) {}
RLS_NEAREST_HD void group_count_instance(GroupNoStats &) {}
RLS_NEAREST_HD void group_count_top_push(GroupNoStats &, int) {}
RLS_NEAREST_HD void nearest_count_node(GroupNoStats &) {}
RLS_NEAREST_HD void nearest_count_tri(GroupNoStats &) {}
RLS_NEAREST_HD void nearest_count_push(GroupNoStats &, int) {}

// ---- a matrix: 12 floats, row-major 3 x 4 ---------------------------------------------------------------------------------------
RLS_NEAREST_HD void group_vector(const float (&M)[12], const float (&p)[3], float (&out)[3])
{
    for (int c = 0; c < 3; c++) out[c] = (M[4 * c] * p[0] + M[4 * c + 1] * p[1]) + M[4 * c + 2] * p[2];
}
RLS_NEAREST_HD void group_point(const float (&M)[12], const float (&p)[3], float (&out)[3])
{
    for (int c = 0; c < 3; c++) out[c] = ((M[4 * c] * p[0] + M[4 * c + 1] * p[1]) + M[4 * c + 2] * p[2]) + M[4 * c + 3];
}
// by the transpose of the linear part
RLS_NEAREST_HD void group_normal(const float (&M)[12], const float (&n)[3], float (&out)[3])
{
    for (int c = 0; c < 3; c++) out[c] = (M[c] * n[0] + M[4 + c] * n[1]) + M[8 + c] * n[2];
}

// The world box of a mesh box [lo, hi] under B, widened by the stated pad.  -> false where an end is not finite.
RLS_NEAREST_HD bool group_world_box(const float (&B)[12], const float (&lo)[3], const float (&hi)[3], float (&wlo)[3], float (&whi)[3])
{
    for (int k = 0; k < 8; k++) {
        const float p[3] = { (k & 1) ? hi[0] : lo[0], (k & 2) ? hi[1] : lo[1], (k & 4) ? hi[2] : lo[2] };
        float q[3];
        group_point(B, p, q);
        for (int c = 0; c < 3; c++) {
            wlo[c] = k == 0 ? q[c] : nearest_minf(wlo[c], q[c]);
            whi[c] = k == 0 ? q[c] : nearest_maxf(whi[c], q[c]);
        }
    }
    const float m[3] = { nearest_maxf(__builtin_fabsf(lo[0]), __builtin_fabsf(hi[0])), nearest_maxf(__builtin_fabsf(lo[1]), __builtin_fabsf(hi[1])),
                         nearest_maxf(__builtin_fabsf(lo[2]), __builtin_fabsf(hi[2])) };
    bool finite = true;
    for (int c = 0; c < 3; c++) {
        const float e = ((__builtin_fabsf(B[4 * c]) * m[0] + __builtin_fabsf(B[4 * c + 1]) * m[1]) + __builtin_fabsf(B[4 * c + 2]) * m[2]) +
                        __builtin_fabsf(B[4 * c + 3]);
        const float pad = e * kGroupPad;
        wlo[c] = wlo[c] - pad;
        whi[c] = whi[c] + pad;
        finite = finite && refit_finite(wlo[c]) && refit_finite(whi[c]);
    }
    return finite;
}

// The record of instance j from its placement and its scene's root box (read only where the scene has nodes).  -> true where
// the instance is PARKED: a non-finite entry of A, B or W, or an empty scene.
RLS_NEAREST_HD bool group_record(const GroupPlacement &p, const float (&lo)[3], const float (&hi)[3], uint32_t j, GroupInstance &rec)
{
    bool live = p.node_count != 0;
    for (int k = 0; k < 12; k++) {
        rec.A[k] = p.A[k];
        live = live && refit_finite(p.A[k]) && refit_finite(p.B[k]);
    }
    float wlo[3] = { 0.0f, 0.0f, 0.0f }, whi[3] = { 0.0f, 0.0f, 0.0f };
    if (live) live = group_world_box(p.B, lo, hi, wlo, whi);
    for (int c = 0; c < 3; c++) { rec.lo[c] = live ? wlo[c] : 0.0f; rec.hi[c] = live ? whi[c] : 0.0f; }
    rec.instance = j;
    rec.node_count = live ? p.node_count : 0u;
    rec.nodes = p.nodes;
    rec.tris = p.tris;
    return !live;
}

// ---- the object level ------------------------------------------------------------------------------------------------------------
// nearest_slab from a given interval instead of [0, +inf): the one change to the slab routine
RLS_NEAREST_HD bool group_slab(const float (&lo)[3], const float (&hi)[3], const NearestRay &r, float tn0, float tf0, float &tn, float &tf)
{
    tn = tn0;
    tf = tf0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 3; c++) {
        float a = (lo[c] - r.o[c]) * r.inv[c], b = (hi[c] - r.o[c]) * r.inv[c];
        if (nearest_sign(r.inv[c])) { const float s = a; a = b; b = s; }
        if (a > tn) tn = a;
        if (b < tf) tf = b;
    }
    return !(tn > tf);
}

// nearest_candidate with the interval started at the instance's world interval; r: the object ray, r.m the reach it runs with
RLS_NEAREST_HD void group_candidate(const NearestTri &tr, uint32_t slot, const NearestRay &r, float tn0, float tf0, NearestBest &best)
{
    if (tr.prim == r.skip) return;
    float lo[3], hi[3], tn, tf, tm, u, v;
    for (int c = 0; c < 3; c++) {
        lo[c] = nearest_minf(nearest_minf(tr.v0[c], tr.v1[c]), tr.v2[c]);
        hi[c] = nearest_maxf(nearest_maxf(tr.v0[c], tr.v1[c]), tr.v2[c]);
    }
    if (!group_slab(lo, hi, r, tn0, tf0, tn, tf)) return;
    if (!nearest_triangle(tr.v0, tr.v1, tr.v2, r, tm, u, v)) return;
    float t = tm;
    if (tn > t) t = tn;
    if (tf < t) t = tf;
    if (!(t > 0.0f && t <= r.m)) return;
    if (best.prim == kNearestNoPrim || t < best.t || (t == best.t && tr.prim < best.prim)) {
        best.t = t; best.u = u; best.v = v; best.prim = tr.prim; best.slot = slot;
    }
}

// The traversal of one instance's tree: nearest_traverse (rls_nearest_device.hpp) with every interval started at (tn0, tf0).
// THE CULL is the one argued there, unchanged by the start: a node's box contains the box of every triangle below it, both
// run the same operations from the same (tn0, tf0), a rounded subtraction and a rounded product by a fixed factor are monotone
// and so is the fold `if (a > tn) tn = a` in its start, hence tn_node <= tn_i and tf_node >= tf_i; a NaN end constrains nothing
// in either.  So a node whose box fails holds no triangle whose box passes, and every candidate below a node has
// t_i >= tn_i >= tn_node: a node with tn_node > r.m (the reach this instance runs with) or > best.t holds no candidate that
// would be taken.  Strict compares: ties are visited, a NaN reach culls nothing (and admits no candidate).
template <class Stack, class Stats>
RLS_NEAREST_HD NearestBest group_bottom(const NearestNode *nodes, uint32_t node_count, const NearestTri *tris, const NearestRay &r, float tn0,
                                        float tf0, Stack &&stack, Stats &stats)
{
    NearestBest best = { 0.0f, 0.0f, 0.0f, kNearestNoPrim, 0u };
    uint32_t node = 0;
    int sp = 0;
    for (uint32_t visits = 0; visits < node_count; visits++) {
        const NearestNode n = nodes[node];
        nearest_count_node(stats);
        float tn, tf;
        bool open = group_slab(n.lo, n.hi, r, tn0, tf0, tn, tf);
        if (tn > r.m || (best.prim != kNearestNoPrim && tn > best.t)) open = false;
        if (open) {
            const uint32_t count = n.meta & kNearestCountMask;
            if (count == 0) {
                const uint32_t axis = n.meta >> kNearestAxisShift;
                const float da = axis == 0 ? r.d[0] : axis == 1 ? r.d[1] : r.d[2];
                const uint32_t near = nearest_sign(da) ? 1u : 0u;
                if (sp < kNearestStack) {
                    stack(sp++) = n.first + (1u - near);
                    nearest_count_push(stats, sp);
                }
                node = n.first + near;
                continue;
            }
            for (uint32_t k = 0; k < count; k++) {
                nearest_count_tri(stats);
                group_candidate(tris[n.first + k], n.first + k, r, tn0, tf0, best);
            }
        }
        if (sp == 0) break;
        node = stack(--sp);
    }
    return best;
}

// ---- the top level ---------------------------------------------------------------------------------------------------------------
// One instance record against the ray.  Its world interval (tnW, tfW) is nearest_slab of W_j against the world ray; every
// triangle interval below starts there, so every candidate of the instance has t_i >= tn_i >= tnW: an instance whose box fails,
// or with tnW > m, or with tnW > best.t (strict: an instance that could TIE the best so far is still entered, and wins the tie
// where its index is smaller) holds no candidate that would win.  Its tree runs with the reach min(m, best.t), a compare written
// so that a NaN m stays the reach (no candidate); a candidate past the best so far could not win, one AT it is compared by
// (t, instance).
template <class Stack, class Stats>
RLS_NEAREST_HD void group_enter(const GroupInstance &rec, const GroupRay &g, GroupBest &best, Stack &&stack, Stats &stats)
{
    if (rec.node_count == 0) return;                                     // parked
    float tnW, tfW;
    if (!nearest_slab(rec.lo, rec.hi, g.w, tnW, tfW)) return;
    const bool have = best.instance != kGroupNoInstance;
    if (tnW > g.w.m || (have && tnW > best.t)) return;
    group_count_instance(stats);
    NearestRay r;
    group_point(rec.A, g.w.o, r.o);
    group_vector(rec.A, g.w.d, r.d);
    for (int c = 0; c < 3; c++) r.inv[c] = 1.0f / r.d[c];
    r.m = g.w.m;
    if (have && best.t < r.m) r.m = best.t;
    r.skip = rec.instance == g.skip_instance ? g.w.skip : kNearestNoPrim;
    const NearestBest b = group_bottom(rec.nodes, rec.node_count, rec.tris, r, tnW, tfW, stack, stats);
    if (b.prim == kNearestNoPrim) return;
    if (!have || b.t < best.t || (b.t == best.t && rec.instance < best.instance)) {
        best.t = b.t; best.u = b.u; best.v = b.v; best.prim = b.prim; best.slot = b.slot; best.instance = rec.instance;
    }
}

// the statement itself: every instance, every triangle, no tree
RLS_NEAREST_HD GroupBest group_brute(const GroupInstance *recs, int64_t count, const GroupRay &g)
{
    GroupBest best = { 0.0f, 0.0f, 0.0f, kNearestNoPrim, 0u, kGroupNoInstance };
    for (int64_t k = 0; k < count; k++) {
        const GroupInstance &rec = recs[k];
        if (rec.node_count == 0) continue;
        float tnW, tfW;
        if (!nearest_slab(rec.lo, rec.hi, g.w, tnW, tfW)) continue;
        NearestRay r;
        group_point(rec.A, g.w.o, r.o);
        group_vector(rec.A, g.w.d, r.d);
        for (int c = 0; c < 3; c++) r.inv[c] = 1.0f / r.d[c];
        r.m = g.w.m;
        r.skip = rec.instance == g.skip_instance ? g.w.skip : kNearestNoPrim;
        // the triangle records of a tree are all of them below the root: the root is a leaf, or its leaves partition the records
        NearestBest b = { 0.0f, 0.0f, 0.0f, kNearestNoPrim, 0u };
        int64_t nt = 0;
        for (uint32_t n = 0; n < rec.node_count; n++) nt += rec.nodes[n].meta & kNearestCountMask;
        for (int64_t i = 0; i < nt; i++) group_candidate(rec.tris[i], (uint32_t)i, r, tnW, tfW, b);
        if (b.prim == kNearestNoPrim) continue;
        if (best.instance == kGroupNoInstance || b.t < best.t || (b.t == best.t && rec.instance < best.instance)) {
            best.t = b.t; best.u = b.u; best.v = b.v; best.prim = b.prim; best.slot = b.slot; best.instance = rec.instance;
        }
    }
    return best;
}

// The traversal of the top tree: its nodes are NearestNodes whose leaves hold instance records.  stack(i): the lane's i-th word;
// words 0 .. kGroupStack - 1 are the top level's, the kNearestStack after them the object level's.  Every top node is visited
// at most once (`visits`), the stack holds one sibling per inner level: at most top depth - 1 <= kGroupStack entries (creation
// refuses deeper trees).
//
// THE CULL: a top node's box contains W_j of every instance below it and sees the same o, inv from the same [0, +inf), so by
// the monotonicity argued in rls_nearest_device.hpp tn_top <= tnW_j, and with group_enter's tnW_j <= tn_i <= t_i: a top node
// whose box fails holds no instance that takes part, and one with tn_top > m or tn_top > best.t no candidate that would win.
template <class Stack, class Stats>
RLS_NEAREST_HD GroupBest group_traverse(const NearestNode *top, int64_t top_count, const GroupInstance *recs, const GroupRay &g, Stack &&stack,
                                        Stats &stats)
{
    GroupBest best = { 0.0f, 0.0f, 0.0f, kNearestNoPrim, 0u, kGroupNoInstance };
    if (top_count <= 0) return best;
    uint32_t node = 0;
    int sp = 0;
    for (int64_t visits = 0; visits < top_count; visits++) {
        const NearestNode n = top[node];
        group_count_top(stats);
        float tn, tf;
        bool open = nearest_slab(n.lo, n.hi, g.w, tn, tf);
        if (tn > g.w.m || (best.instance != kGroupNoInstance && tn > best.t)) open = false;
        if (open) {
            const uint32_t count = n.meta & kNearestCountMask;
            if (count == 0) {
                const uint32_t axis = n.meta >> kNearestAxisShift;
                const float da = axis == 0 ? g.w.d[0] : axis == 1 ? g.w.d[1] : g.w.d[2];
                const uint32_t near = nearest_sign(da) ? 1u : 0u;
                if (sp < kGroupStack) {
                    stack(sp++) = n.first + (1u - near);
                    group_count_top_push(stats, sp);
                }
                node = n.first + near;
                continue;
            }
            for (uint32_t k = 0; k < count; k++)
                group_enter(recs[n.first + k], g, best, [&](int i) -> uint32_t & { return stack(kGroupStack + i); }, stats);
        }
        if (sp == 0) break;
        node = stack(--sp);
    }
    return best;
}

// A hit's frame: N = normalize(A^T (e1 x e2)), Ns = normalize(A^T s) of the interpolated vertex normals s (not normalised in
// between) where nrm is given, else N, T = normalize(B e1).  No flip under a mirroring A.
RLS_NEAREST_HD void group_frame(const NearestTri &tr, float u, float v, const float *n0, const float *n1, const float *n2, const float (&A)[12],
                                const float (&B)[12], float (&N)[3], float (&Ns)[3], float (&T)[3])
{
    const float e1[3] = { tr.v1[0] - tr.v0[0], tr.v1[1] - tr.v0[1], tr.v1[2] - tr.v0[2] };
    const float e2[3] = { tr.v2[0] - tr.v0[0], tr.v2[1] - tr.v0[1], tr.v2[2] - tr.v0[2] };
    float n[3], wn[3], we[3];
    nearest_cross(e1, e2, n);
    group_normal(A, n, wn);
    nearest_normalize(wn, N);
    group_vector(B, e1, we);
    nearest_normalize(we, T);
    if (n0) {
        const float w = (1.0f - u) - v;
        const float s[3] = { (w * n0[0] + u * n1[0]) + v * n2[0], (w * n0[1] + u * n1[1]) + v * n2[1],
                             (w * n0[2] + u * n1[2]) + v * n2[2] };
        float ws[3];
        group_normal(A, s, ws);
        nearest_normalize(ws, Ns);
    } else {
        Ns[0] = N[0]; Ns[1] = N[1]; Ns[2] = N[2];
    }
}

// ---- the top tree's boxes, for the update: only compares and copies (the sign of a zero bound: rls_nearest_refit.hpp) ---------
// One top node's box from what is below it, written back; first and meta are not written.
RLS_NEAREST_HD void group_node(NearestNode *top, const GroupInstance *recs, uint32_t node)
{
    const uint32_t first = top[node].first, count = top[node].meta & kNearestCountMask;
    float lo[3], hi[3];
    if (count) {
        for (uint32_t k = 0; k < count; k++)
            for (int c = 0; c < 3; c++) {
                lo[c] = k == 0 ? recs[first].lo[c] : nearest_minf(lo[c], recs[first + k].lo[c]);
                hi[c] = k == 0 ? recs[first].hi[c] : nearest_maxf(hi[c], recs[first + k].hi[c]);
            }
    } else {
        refit_union(top[first], top[first + 1], lo, hi);
    }
    for (int c = 0; c < 3; c++) { top[node].lo[c] = lo[c]; top[node].hi[c] = hi[c]; }
}

// The top tree over the records' world boxes by the builder of rls_nearest_bvh.hpp (the boxes given, not read from vertices):
// `order`: the instance of every record slot.  world: [count * 6] lo xyz hi xyz by instance.
inline void group_build(const float *world, int64_t count, int leaf, NearestBvh &out, std::vector<uint32_t> &order)
{
    out.nodes.clear();
    out.tris.clear();
    out.depth = 0;
    order.clear();
    if (count <= 0) return;
    nearest_detail::Builder b;
    b.V = nullptr; b.tri = nullptr; b.leaf = leaf; b.out = &out;
    b.lo.resize(3 * (size_t)count); b.hi.resize(3 * (size_t)count); b.key.resize(3 * (size_t)count); b.order.resize((size_t)count);
    for (size_t i = 0; i < (size_t)count; i++) {
        b.order[i] = (uint32_t)i;
        for (int c = 0; c < 3; c++) {
            b.lo[3 * i + c] = world[6 * i + c];
            b.hi[3 * i + c] = world[6 * i + 3 + c];
            b.key[3 * i + c] = nearest_order_key(b.lo[3 * i + c] + b.hi[3 * i + c]);
        }
    }
    out.nodes.reserve(2 * (size_t)count);
    out.nodes.resize(1);
    b.build(0, 0, count, 1);
    order = b.order;
}

#if defined(__HIPCC__)
// ---- the query kernel: one ray per lane over the companions' tile skeleton --------------------------------------------------------
struct GroupIO {
    const NearestNode *top;
    const GroupInstance *recs;
    const GroupPlacement *place;
    int64_t top_count;
    rls_nearest_rays r;
    rls_nearest_found f;
    uint32_t *instance, *last_instance;
    int64_t tiles;
};

__device__ __forceinline__ void group_store3(const rls_vec3 &p, int64_t k, const float (&a)[3])
{
    if (p.x) { p.x[k] = a[0]; p.y[k] = a[1]; p.z[k] = a[2]; }
}

__global__ __launch_bounds__(rlsh::kBlock) void group_kernel(GroupIO a)
{
    // both stacks of every lane, word i of lane l at [i][l]: consecutive lanes in consecutive banks, 40 KiB a workgroup, no
    // spill to scratch memory
    __shared__ uint32_t stacks[kGroupStack + kNearestStack][rlsh::kBlock];
    int64_t m = a.r.rays;
    if (a.r.count) {
        const int64_t c = *a.r.count;
        m = c < 0 ? 0 : c < m ? c : m;
    }
    const unsigned lane = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t k = tile * rlsh::kBlock + lane;
        if (k >= m) continue;                                        // (no barrier in this kernel)
        const int64_t from = a.r.via ? (int64_t)a.r.via[k] : k;
        const float o[3] = { a.r.origin.x[from], a.r.origin.y[from], a.r.origin.z[from] };
        const float d[3] = { a.r.dir.x[k], a.r.dir.y[k], a.r.dir.z[k] };
        const int64_t id = a.r.ray ? (int64_t)a.r.ray[k] : k;
        GroupRay g;
        g.w = nearest_ray(o, d, a.r.maxdist ? a.r.maxdist[k] : __builtin_inff(), a.f.last ? a.f.last[id] : kNearestNoPrim);
        g.skip_instance = a.f.last ? a.last_instance[id] : kGroupNoInstance;
        GroupNoStats none;
        const GroupBest b = group_traverse(a.top, a.top_count, a.recs, g, [&](int i) -> uint32_t & { return stacks[i][lane]; }, none);
        const bool hit = b.instance != kGroupNoInstance;
        a.f.hit[k] = hit ? 1 : 0;
        if (!hit) {
            if (a.f.bin) a.f.bin[k] = 255;
            continue;
        }
        a.f.t[k] = b.t;
        const GroupPlacement &p = a.place[b.instance];
        const uint32_t surface = p.surface_base + (p.surface ? p.surface[b.prim] : 0u);
        if (a.f.prim) a.f.prim[k] = b.prim;
        if (a.instance) a.instance[k] = b.instance;
        if (a.f.surface) a.f.surface[k] = surface;
        if (a.f.u) a.f.u[k] = b.u;
        if (a.f.v) a.f.v[k] = b.v;
        if (a.f.bin) a.f.bin[k] = a.f.bin_of_surface[surface < a.f.bin_count ? surface : a.f.bin_count - 1];
        if (a.f.last) { a.f.last[id] = b.prim; a.last_instance[id] = b.instance; }
        const float P[3] = { o[0] + b.t * d[0], o[1] + b.t * d[1], o[2] + b.t * d[2] }, wo[3] = { -d[0], -d[1], -d[2] };
        group_store3(a.f.P, k, P);
        group_store3(a.f.wo, k, wo);
        if (a.f.N.x || a.f.Ns.x || a.f.T.x) {
            const NearestTri tr = p.tris[b.slot];
            const float *n0 = nullptr, *n1 = nullptr, *n2 = nullptr;
            if (p.normals && a.f.Ns.x) {
                n0 = p.normals + 3 * (int64_t)p.index[3 * (int64_t)b.prim];
                n1 = p.normals + 3 * (int64_t)p.index[3 * (int64_t)b.prim + 1];
                n2 = p.normals + 3 * (int64_t)p.index[3 * (int64_t)b.prim + 2];
            }
            float N[3], Ns[3], T[3];
            group_frame(tr, b.u, b.v, n0, n1, n2, p.A, p.B, N, Ns, T);
            group_store3(a.f.N, k, N);
            group_store3(a.f.Ns, k, Ns);
            group_store3(a.f.T, k, T);
        }
    }
}

// ---- the update's kernels: one lane per instance, then one lane per top node of a level ------------------------------------------
struct GroupRecordsIO {
    GroupInstance *recs;
    GroupPlacement *place;
    const float *to_object, *to_world;    // [count * 12] each, or both NULL: the matrices stay
    unsigned long long *parked;           // NULL-able: zeroed on the stream ahead of the launch
    int64_t count, tiles;
};

// The matrices into the placement, the scene's root box as it is now, the record.  The parked instances are counted as the
// refit counts its parked triangles: a register a lane, a sum over the workgroup, one integer atomic per workgroup that parked any.
__global__ __launch_bounds__(rlsh::kBlock) void group_records_kernel(GroupRecordsIO a)
{
    __shared__ unsigned wave_parked[rlsh::kBlock / 64];
    unsigned mine = 0;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t j = tile * rlsh::kBlock + threadIdx.x;
        if (j >= a.count) continue;
        GroupPlacement &p = a.place[j];
        if (a.to_object)
            for (int k = 0; k < 12; k++) { p.A[k] = a.to_object[12 * j + k]; p.B[k] = a.to_world[12 * j + k]; }
        float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 0.0f, 0.0f, 0.0f };
        if (p.node_count)
            for (int c = 0; c < 3; c++) { lo[c] = p.nodes[0].lo[c]; hi[c] = p.nodes[0].hi[c]; }
        GroupInstance rec;
        mine += group_record(p, lo, hi, (uint32_t)j, rec) ? 1u : 0u;
        a.recs[p.slot] = rec;
    }
    if (!a.parked) return;                                               // (uniform: no lane waits at the barrier below)
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_down(mine, d, 64);
    if ((threadIdx.x & 63u) == 0) wave_parked[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned sum = 0;
        for (int w = 0; w < rlsh::kBlock / 64; w++) sum += wave_parked[w];
        if (sum) atomicAdd(a.parked, (unsigned long long)sum);
    }
}

struct GroupLevelIO {
    NearestNode *top;
    const GroupInstance *recs;
    const uint32_t *list;                 // this level's run of the node lists
    int64_t count, tiles;
};

// one level: every node of it reads records or nodes of a deeper level, which an earlier launch finished
__global__ __launch_bounds__(rlsh::kBlock) void group_level_kernel(GroupLevelIO a)
{
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t k = tile * rlsh::kBlock + threadIdx.x;
        if (k < a.count) group_node(a.top, a.recs, a.list[k]);
    }
}

// the top of the tree in one launch of ONE workgroup: `levels` runs of at most kBlock nodes each, deepest first, a barrier
// between them
constexpr int kGroupTopLevels = kGroupStack + 1;
struct GroupTopIO {
    NearestNode *top;
    const GroupInstance *recs;
    const uint32_t *list;
    int levels;
    uint32_t offset[kGroupTopLevels + 1];   // into list
};

__global__ __launch_bounds__(rlsh::kBlock) void group_top_kernel(GroupTopIO a)
{
    for (int l = 0; l < a.levels; l++) {
        const uint32_t k = a.offset[l] + threadIdx.x;
        if (k < a.offset[l + 1]) group_node(a.top, a.recs, a.list[k]);
        __syncthreads();
    }
}
#endif // __HIPCC__

#endif
