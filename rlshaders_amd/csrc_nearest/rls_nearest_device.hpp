// rls_nearest_device.hpp -- the nearest-hit query of librls_nearest.so (include/rlshaders_amd_nearest.h): the slab test, the
// triangle test, the traversal and a hit's frame, each written once as host + device functions, and (under hipcc) the kernel
// around them.  tests/native/nearest_host_check.cpp compiles the same functions for the CPU and holds the traversal to a brute
// force over the statement, bit for bit; nearest_stats.cpp beside this file counts the nodes and triangles a ray visits through
// NearestStats, and the most stack entries it holds (rlshaders_amd.nearest.host_stats; tools/trace_bench.py --closure nearest,
// tests/test_gpu_nearest_edges.py and tests/test_nearest_deep.py use it).
//
// float32 throughout, every operation by itself (-ffp-contract=off), / and sqrt correctly rounded; min and max are compares
// written out, so a NaN never replaces the other operand.
#ifndef RLS_NEAREST_DEVICE_HPP
#define RLS_NEAREST_DEVICE_HPP

#include <math.h>

#include "rls_nearest_bvh.hpp"

#if defined(__HIPCC__)
#define RLS_NEAREST_HD __host__ __device__ __forceinline__
#else
#define RLS_NEAREST_HD inline
#endif

constexpr int kNearestStack = 24;                 // RLS_NEAREST_STACK: node indices a lane can hold
constexpr uint32_t kNearestNoPrim = 0xFFFFFFFFu;

struct NearestRay {
    float o[3], d[3], inv[3];
    float m;                                      // the reach, +inf where there is none
    uint32_t skip;
};
struct NearestBest {
    float t, u, v;
    uint32_t prim;                                // kNearestNoPrim: no candidate yet
    uint32_t slot;                                // the winner's triangle record
};
struct NearestStats { int64_t nodes = 0, tris = 0; int max_stack = 0; };   // max_stack: the most entries the ray held at once
struct NearestNoStats {};
RLS_NEAREST_HD void nearest_count_node(NearestStats &s) { s.nodes++; }
RLS_NEAREST_HD void nearest_count_tri(NearestStats &s) { s.tris++; }
RLS_NEAREST_HD void nearest_count_push(NearestStats &s, int held) { if (held > s.max_stack) s.max_stack = held; }
RLS_NEAREST_HD void nearest_count_node(NearestNoStats &) {}
RLS_NEAREST_HD void nearest_count_tri(NearestNoStats &) {}
RLS_NEAREST_HD void nearest_count_push(NearestNoStats &, int) {}

RLS_NEAREST_HD bool nearest_sign(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (__float_as_uint(f) >> 31) != 0;
#else
    uint32_t b;
    memcpy(&b, &f, sizeof b);
    return (b >> 31) != 0;
#endif
}
RLS_NEAREST_HD float nearest_dot(const float (&a)[3], const float (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
RLS_NEAREST_HD void nearest_cross(const float (&a)[3], const float (&b)[3], float (&c)[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

RLS_NEAREST_HD NearestRay nearest_ray(const float (&o)[3], const float (&d)[3], float m, uint32_t skip)
{
    NearestRay r;
    for (int c = 0; c < 3; c++) { r.o[c] = o[c]; r.d[c] = d[c]; r.inv[c] = 1.0f / d[c]; }
    r.m = m; r.skip = skip;
    return r;
}

// The ray's interval inside a box, [0, +inf) confined by the three slabs.  A NaN fails both compares and constrains nothing.  The
// reach is not part of it: a triangle behind the reach must not be pulled in front of it by the confinement (nearest_candidate).
RLS_NEAREST_HD bool nearest_slab(const float (&lo)[3], const float (&hi)[3], const NearestRay &r, float &tn, float &tf)
{
    tn = 0.0f;
    tf = __builtin_inff();
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

// Moller-Trumbore, two-sided
RLS_NEAREST_HD bool nearest_triangle(const float (&v0)[3], const float (&v1)[3], const float (&v2)[3], const NearestRay &r, float &tm,
                                     float &u, float &v)
{
    const float e1[3] = { v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2] }, e2[3] = { v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2] };
    float p[3], q[3];
    nearest_cross(r.d, e2, p);
    const float det = nearest_dot(e1, p);
    if (!(det < 0.0f || det > 0.0f)) return false;
    const float rd = 1.0f / det;
    const float s[3] = { r.o[0] - v0[0], r.o[1] - v0[1], r.o[2] - v0[2] };
    u = nearest_dot(s, p) * rd;
    nearest_cross(s, e1, q);
    v = nearest_dot(r.d, q) * rd;
    tm = nearest_dot(e2, q) * rd;
    return u >= 0.0f && v >= 0.0f && u + v <= 1.0f && tm == tm;
}

// One triangle record against the ray: the statement's candidate rule and its order (smaller t, then smaller index).
RLS_NEAREST_HD void nearest_candidate(const NearestTri &tr, uint32_t slot, const NearestRay &r, NearestBest &best)
{
    if (tr.prim == r.skip) return;
    float lo[3], hi[3], tn, tf, tm, u, v;
    for (int c = 0; c < 3; c++) {
        lo[c] = nearest_minf(nearest_minf(tr.v0[c], tr.v1[c]), tr.v2[c]);
        hi[c] = nearest_maxf(nearest_maxf(tr.v0[c], tr.v1[c]), tr.v2[c]);
    }
    if (!nearest_slab(lo, hi, r, tn, tf)) return;
    if (!nearest_triangle(tr.v0, tr.v1, tr.v2, r, tm, u, v)) return;
    float t = tm;
    if (tn > t) t = tn;
    if (tf < t) t = tf;
    if (!(t > 0.0f && t <= r.m)) return;
    if (best.prim == kNearestNoPrim || t < best.t || (t == best.t && tr.prim < best.prim)) {
        best.t = t; best.u = u; best.v = v; best.prim = tr.prim; best.slot = slot;
    }
}

// the statement itself: every triangle, no tree
RLS_NEAREST_HD NearestBest nearest_brute(const NearestTri *tris, int64_t nt, const NearestRay &r)
{
    NearestBest best = { 0.0f, 0.0f, 0.0f, kNearestNoPrim, 0u };
    for (int64_t k = 0; k < nt; k++) nearest_candidate(tris[k], (uint32_t)k, r, best);
    return best;
}

// The traversal.  stack(i): a reference to the lane's i-th stack word (LDS on the device, an array on the host).
//
// Every node is visited at most once -- a node is pushed only by its parent's visit -- so the loop runs at most node_count
// times whatever the ray holds (NaN, inf, zero); the guard on `visits` states that bound in the loop itself.  The stack holds
// one sibling per inner level on the way down: at most depth - 1 <= kNearestStack entries (scene creation refuses deeper trees).
//
// THE CULL, and why it is exact.  A node's box contains the box of every triangle i below it: lo_node <= lo_i, hi_i <= hi_node
// per axis.  The slab test runs the same three operations on both: x -> (x - o) * inv.  A rounded subtraction and a rounded
// product by a fixed factor are monotone (non-decreasing for inv >= 0, non-increasing for inv < 0, where the test swaps the
// ends), so the node's near end a_node <= a_i and its far end b_node >= b_i wherever both are numbers, hence tn_node <= tn_i
// and tf_node >= tf_i.  Where an end is NaN it constrains nothing, which only matters if the TRIANGLE's end is NaN and the
// node's is a number that constrains: a NaN end is 0 * inf -- (x_i - o) == 0 under inv = +-inf, where the node's near end is
// then (<= 0) * (+inf) or (>= 0) * (-inf): -inf or NaN, no constraint on tn >= 0, and its far end +inf or NaN, none on tf; or
// (+-inf) * (+-0) under a direction component of +-inf, and such a ray has no candidate at all: p = d x e2 then holds an inf
// or a NaN in two components, det is +-inf or NaN, r is +-0 or NaN and u = (s . p) * r is NaN.  A NaN in o or d makes every
// end, and det, NaN: no candidate either.  So (1) a node whose box fails (tn > tf) holds no triangle whose box passes, and
// (2) every candidate below a node has t_i >= tn_i >= tn_node (t_i is confined to [tn_i, tf_i]), so a node with
// tn_node > best.t holds no candidate that beats or ties the best so far, and a node with tn_node > m none at all (t_i <= m).
// The compares are strict: a tie at the same t with a smaller index is still visited, and a NaN reach culls nothing.  Which
// child goes first (the one on the ray's side of the split axis) changes the work only.
template <class Stack, class Stats>
RLS_NEAREST_HD NearestBest nearest_traverse(const NearestNode *nodes, int64_t node_count, const NearestTri *tris, const NearestRay &r,
                                            Stack &&stack, Stats &stats)
{
    NearestBest best = { 0.0f, 0.0f, 0.0f, kNearestNoPrim, 0u };
    if (node_count <= 0) return best;
    uint32_t node = 0;
    int sp = 0;
    for (int64_t visits = 0; visits < node_count; visits++) {
        const NearestNode n = nodes[node];
        nearest_count_node(stats);
        float tn, tf;
        bool open = nearest_slab(n.lo, n.hi, r, tn, tf);
        if (tn > r.m || (best.prim != kNearestNoPrim && tn > best.t)) open = false;
        if (open) {
            const uint32_t count = n.meta & kNearestCountMask;
            if (count == 0) {
                const uint32_t axis = n.meta >> kNearestAxisShift;
                const float da = axis == 0 ? r.d[0] : axis == 1 ? r.d[1] : r.d[2];
                const uint32_t near = nearest_sign(da) ? 1u : 0u;      // the left child holds the smaller centroids
                if (sp < kNearestStack) {
                    stack(sp++) = n.first + (1u - near);
                    nearest_count_push(stats, sp);
                }
                node = n.first + near;
                continue;
            }
            for (uint32_t k = 0; k < count; k++) {
                nearest_count_tri(stats);
                nearest_candidate(tris[n.first + k], n.first + k, r, best);
            }
        }
        if (sp == 0) break;
        node = stack(--sp);
    }
    return best;
}

// A hit's frame: N, Ns (the interpolated vertex normals where nrm is given, else N), T.
RLS_NEAREST_HD void nearest_normalize(const float (&a)[3], float (&out)[3])
{
    const float l = sqrtf(nearest_dot(a, a));
    out[0] = a[0] / l; out[1] = a[1] / l; out[2] = a[2] / l;
}
RLS_NEAREST_HD void nearest_frame(const NearestTri &tr, float u, float v, const float *n0, const float *n1, const float *n2,
                                  float (&N)[3], float (&Ns)[3], float (&T)[3])
{
    const float e1[3] = { tr.v1[0] - tr.v0[0], tr.v1[1] - tr.v0[1], tr.v1[2] - tr.v0[2] };
    const float e2[3] = { tr.v2[0] - tr.v0[0], tr.v2[1] - tr.v0[1], tr.v2[2] - tr.v0[2] };
    float n[3];
    nearest_cross(e1, e2, n);
    nearest_normalize(n, N);
    nearest_normalize(e1, T);
    if (n0) {
        const float w = (1.0f - u) - v;
        const float s[3] = { (w * n0[0] + u * n1[0]) + v * n2[0], (w * n0[1] + u * n1[1]) + v * n2[1],
                             (w * n0[2] + u * n1[2]) + v * n2[2] };
        nearest_normalize(s, Ns);
    } else {
        Ns[0] = N[0]; Ns[1] = N[1]; Ns[2] = N[2];
    }
}

#if defined(__HIPCC__) && !defined(RLS_NEAREST_DEVICE_NO_KERNEL)   // (the group library takes the functions above alone)
// ---- the kernel: one ray per lane over the companions' tile skeleton -----------------------------------------------------------
struct NearestIO {
    const NearestNode *nodes;
    const NearestTri *tris;
    const uint32_t *index;            // [nt * 3]: the mesh's vertex indices, for the normals
    const uint32_t *surface;          // [nt] or NULL
    const float *normals;             // [nv * 3] or NULL
    int64_t node_count;
    rls_nearest_rays r;
    rls_nearest_found f;
    int64_t tiles;
};

__device__ __forceinline__ void nearest_store3(const rls_vec3 &p, int64_t k, const float (&a)[3])
{
    if (p.x) { p.x[k] = a[0]; p.y[k] = a[1]; p.z[k] = a[2]; }
}

__global__ __launch_bounds__(rlsh::kBlock) void nearest_kernel(NearestIO a)
{
    // the lanes' stacks, word i of lane l at [i][l]: consecutive lanes in consecutive banks, no spill to scratch memory
    __shared__ uint32_t stacks[kNearestStack][rlsh::kBlock];
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
        const NearestRay r = nearest_ray(o, d, a.r.maxdist ? a.r.maxdist[k] : __builtin_inff(),
                                         a.f.last ? a.f.last[id] : kNearestNoPrim);
        NearestNoStats none;
        const NearestBest b = nearest_traverse(a.nodes, a.node_count, a.tris, r,
                                               [&](int i) -> uint32_t & { return stacks[i][lane]; }, none);
        const bool hit = b.prim != kNearestNoPrim;
        a.f.hit[k] = hit ? 1 : 0;
        if (!hit) {
            if (a.f.bin) a.f.bin[k] = 255;
            continue;
        }
        a.f.t[k] = b.t;
        const uint32_t surface = a.surface ? a.surface[b.prim] : 0u;
        if (a.f.prim) a.f.prim[k] = b.prim;
        if (a.f.surface) a.f.surface[k] = surface;
        if (a.f.u) a.f.u[k] = b.u;
        if (a.f.v) a.f.v[k] = b.v;
        if (a.f.bin) a.f.bin[k] = a.f.bin_of_surface[surface < a.f.bin_count ? surface : a.f.bin_count - 1];
        if (a.f.last) a.f.last[id] = b.prim;
        const float P[3] = { o[0] + b.t * d[0], o[1] + b.t * d[1], o[2] + b.t * d[2] }, wo[3] = { -d[0], -d[1], -d[2] };
        nearest_store3(a.f.P, k, P);
        nearest_store3(a.f.wo, k, wo);
        if (a.f.N.x || a.f.Ns.x || a.f.T.x) {
            const NearestTri tr = a.tris[b.slot];
            const float *n0 = nullptr, *n1 = nullptr, *n2 = nullptr;
            if (a.normals && a.f.Ns.x) {
                n0 = a.normals + 3 * (int64_t)a.index[3 * (int64_t)b.prim];
                n1 = a.normals + 3 * (int64_t)a.index[3 * (int64_t)b.prim + 1];
                n2 = a.normals + 3 * (int64_t)a.index[3 * (int64_t)b.prim + 2];
            }
            float N[3], Ns[3], T[3];
            nearest_frame(tr, b.u, b.v, n0, n1, n2, N, Ns, T);
            nearest_store3(a.f.N, k, N);
            nearest_store3(a.f.Ns, k, Ns);
            nearest_store3(a.f.T, k, T);
        }
    }
}
#endif // __HIPCC__

#endif
