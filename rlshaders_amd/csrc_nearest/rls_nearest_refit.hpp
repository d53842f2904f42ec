// rls_nearest_refit.hpp -- the refit of librls_nearest_refit.so (include/rlshaders_amd_nearest_refit.h): a triangle record from
// moved vertices, a leaf's box from its records, an inner node's box from its two children, and the levels of a tree that is
// there -- each written once as host + device functions, and (under hipcc) the kernels around them.
// tests/native/nearest_refit_host_check.cpp compiles the same functions for the CPU and holds a refit tree to the exact
// union, to the untouched links and to the brute force over the statement.
//
// Only compares and copies: no arithmetic rounds here, so the CPU and the device agree whatever the flags.
//
// THE SIGN OF A ZERO BOUND.  A bound is the smallest (largest) of a set of floats by nearest_minf (nearest_maxf).  As a value
// that is unique; where the set holds both -0 and +0 the one kept depends on the order of the fold, and the builder
// (rls_nearest_bvh.hpp) folds a node's triangles in an order the refit does not have.  So a refit box == the builder's box
// bound for bound, but a zero bound may differ in sign.  No result depends on it.  A node's box enters a query in
// nearest_slab alone (rls_nearest_device.hpp), as (bound - o) * inv per axis, whose results are compared (a > tn, b < tf,
// tn > tf, and the traversal's tn > m, tn > best.t) and never reported: a hit's t is confined to the interval of the
// TRIANGLE's own box, computed from its record.  (1) o != 0: -0 - o and +0 - o are the same float.  (2) o == +-0: the
// difference is +0 or -0; times a finite inv it is a zero of either sign, and every compare above reads -0 and +0 alike, as
// does the next compare against a tn or tf that was set to such a zero; (3) times an infinite inv it is NaN whatever the
// sign, and constrains nothing either way.  The swap of a and b under a negative inv exchanges values, not signs.  So the
// nodes opened, their order and the candidates tested are the same under both boxes, and the cost is too.
#ifndef RLS_NEAREST_REFIT_HPP
#define RLS_NEAREST_REFIT_HPP

#include <stdint.h>

#include <vector>

#include "rls_nearest_bvh.hpp"

#if defined(__HIPCC__)
#define RLS_REFIT_HD __host__ __device__ __forceinline__
#else
#define RLS_REFIT_HD inline
#endif

// neither a NaN nor an infinity (a NaN fails the compare)
RLS_REFIT_HD bool refit_finite(float f) { return __builtin_fabsf(f) <= 3.40282346638528859812e+38f; }

// The record of triangle `prim` from the moved vertices V through its three indices.  A NaN or an infinity in any of the nine
// coordinates PARKS it: three vertices at the origin, so e1 = e2 = 0 and det = e1 . p is 0 (or NaN under a non-finite
// direction) -- never a candidate -- and its box is the point at the origin.  -> true where parked.
RLS_REFIT_HD bool refit_record(const float *V, uint32_t i0, uint32_t i1, uint32_t i2, uint32_t prim, NearestTri &t)
{
    const float *a = V + 3 * (int64_t)i0, *b = V + 3 * (int64_t)i1, *c = V + 3 * (int64_t)i2;
    bool finite = true;
    for (int k = 0; k < 3; k++) {
        t.v0[k] = a[k]; t.v1[k] = b[k]; t.v2[k] = c[k];
        finite = finite && refit_finite(a[k]) && refit_finite(b[k]) && refit_finite(c[k]);
    }
    if (!finite)
        for (int k = 0; k < 3; k++) t.v0[k] = t.v1[k] = t.v2[k] = 0.0f;
    t.prim = prim; t.pad1 = 0u; t.pad2 = 0u;
    return !finite;
}

// a leaf's box: the union over its records of the smallest / largest component of each record's three vertices
RLS_REFIT_HD void refit_leaf_box(const NearestTri *tris, uint32_t first, uint32_t count, float (&lo)[3], float (&hi)[3])
{
    for (uint32_t k = 0; k < count; k++) {
        const NearestTri &t = tris[first + k];
        for (int c = 0; c < 3; c++) {
            const float l = nearest_minf(nearest_minf(t.v0[c], t.v1[c]), t.v2[c]);
            const float h = nearest_maxf(nearest_maxf(t.v0[c], t.v1[c]), t.v2[c]);
            lo[c] = k == 0 ? l : nearest_minf(lo[c], l);
            hi[c] = k == 0 ? h : nearest_maxf(hi[c], h);
        }
    }
}

// an inner node's box: the union of its two children's
RLS_REFIT_HD void refit_union(const NearestNode &a, const NearestNode &b, float (&lo)[3], float (&hi)[3])
{
    for (int c = 0; c < 3; c++) {
        lo[c] = nearest_minf(a.lo[c], b.lo[c]);
        hi[c] = nearest_maxf(a.hi[c], b.hi[c]);
    }
}

// One node's box from what is below it, written back; first and meta are not written.
RLS_REFIT_HD void refit_node(NearestNode *nodes, const NearestTri *tris, uint32_t node)
{
    const uint32_t first = nodes[node].first, count = nodes[node].meta & kNearestCountMask;
    float lo[3], hi[3];
    if (count) refit_leaf_box(tris, first, count, lo, hi);
    else refit_union(nodes[first], nodes[first + 1], lo, hi);
    for (int c = 0; c < 3; c++) { nodes[node].lo[c] = lo[c]; nodes[node].hi[c] = hi[c]; }
}

// The levels of a tree that is there, read from its nodes' links (the builder is not replayed): `list` holds every node once,
// the deepest level first and the root last, and `offset` [levels + 1] where each level's run begins.  A node is on the level
// after its parent's, so every node's children stand in an earlier run.  -> false where the links are not a tree over
// `nodes` nodes and `nt` records (a child out of range or met twice, a leaf past the records, an unreachable node).
inline bool refit_levels(const NearestNode *nodes, int64_t node_count, int64_t nt, std::vector<uint32_t> &list, std::vector<int64_t> &offset)
{
    list.clear();
    offset.assign(1, 0);
    if (node_count <= 0) return node_count == 0;
    std::vector<uint32_t> level((size_t)node_count, 0u), order;
    order.reserve((size_t)node_count);
    order.push_back(0u);
    level[0] = 1u;
    uint32_t depth = 1;
    for (size_t at = 0; at < order.size(); at++) {                       // breadth first: `order` is sorted by level
        const NearestNode &n = nodes[order[at]];
        const uint32_t count = n.meta & kNearestCountMask;
        if (count) {
            if ((int64_t)n.first + count > nt) return false;
            continue;
        }
        if ((int64_t)n.first + 1 >= node_count) return false;
        for (uint32_t c = n.first; c <= n.first + 1; c++) {
            if (level[c]) return false;
            level[c] = level[order[at]] + 1;
            if (level[c] > depth) depth = level[c];
            order.push_back(c);
        }
    }
    if ((int64_t)order.size() != node_count) return false;
    std::vector<int64_t> count((size_t)depth + 1, 0);
    for (uint32_t n : order) count[level[n]]++;
    offset.assign((size_t)depth + 1, 0);
    for (uint32_t l = depth, k = 0; l >= 1; l--, k++) offset[k + 1] = offset[k] + count[l];
    list.resize((size_t)node_count);
    std::vector<int64_t> at(offset.begin(), offset.end() - 1);
    for (uint32_t n : order) list[(size_t)at[depth - level[n]]++] = n;
    return true;
}

// the whole refit on the host, for the CPU check: the records, then the levels bottom-up.  -> the triangles parked
inline int64_t refit_host(NearestNode *nodes, NearestTri *tris, int64_t nt, const uint32_t *index, const float *V,
                          const std::vector<uint32_t> &list)
{
    int64_t parked = 0;
    for (int64_t k = 0; k < nt; k++) {
        const uint32_t prim = tris[k].prim;
        parked += refit_record(V, index[3 * (int64_t)prim], index[3 * (int64_t)prim + 1], index[3 * (int64_t)prim + 2], prim, tris[k]);
    }
    for (uint32_t n : list) refit_node(nodes, tris, n);
    return parked;
}

#if defined(__HIPCC__) && !defined(RLS_NEAREST_REFIT_NO_KERNELS)   // (the group library takes the functions above alone)
// ---- the kernels: one lane per triangle slot, then one lane per node of a level, over the companions' tile skeleton ------------
struct RefitRecordsIO {
    NearestTri *tris;
    const uint32_t *index;            // [nt * 3]: the scene's vertex indices
    const float *vertices;            // [nv * 3]: the moved mesh
    unsigned long long *parked;       // NULL-able: zeroed on the stream ahead of the launch
    int64_t nt, tiles;
};

// Gather three indices and nine floats a slot, write the 48-byte record as three 16-byte stores.  The parked triangles are
// counted in a register a lane, summed over the workgroup in LDS after the tile loop, and added by one atomic per workgroup
// that parked any: none on the hot path, and exact (integers).
__global__ __launch_bounds__(rlsh::kBlock) void refit_records_kernel(RefitRecordsIO a)
{
    __shared__ unsigned wave_parked[rlsh::kBlock / 64];
    unsigned mine = 0;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t k = tile * rlsh::kBlock + threadIdx.x;
        if (k >= a.nt) continue;
        const uint32_t prim = a.tris[k].prim;
        const uint32_t *ix = a.index + 3 * (int64_t)prim;
        NearestTri t;
        mine += refit_record(a.vertices, ix[0], ix[1], ix[2], prim, t) ? 1u : 0u;
        float4 *out = reinterpret_cast<float4 *>(a.tris + k);
        out[0] = make_float4(t.v0[0], t.v0[1], t.v0[2], __uint_as_float(t.prim));
        out[1] = make_float4(t.v1[0], t.v1[1], t.v1[2], 0.0f);
        out[2] = make_float4(t.v2[0], t.v2[1], t.v2[2], 0.0f);
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

struct RefitLevelIO {
    NearestNode *nodes;
    const NearestTri *tris;
    const uint32_t *list;             // this level's run of the node lists
    int64_t count, tiles;
};

// one level: every node of it reads records or nodes of a deeper level, which an earlier launch finished
__global__ __launch_bounds__(rlsh::kBlock) void refit_level_kernel(RefitLevelIO a)
{
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t k = tile * rlsh::kBlock + threadIdx.x;
        if (k < a.count) refit_node(a.nodes, a.tris, a.list[k]);
    }
}

// The top of the tree in one launch of ONE workgroup: `levels` runs of at most kBlock nodes each, deepest first, a barrier
// between them (a workgroup's stores to global memory are visible to its own lanes after __syncthreads).
constexpr int kRefitTopLevels = 32;
struct RefitTopIO {
    NearestNode *nodes;
    const NearestTri *tris;
    const uint32_t *list;
    int levels;
    uint32_t offset[kRefitTopLevels + 1];   // into list
};

__global__ __launch_bounds__(rlsh::kBlock) void refit_top_kernel(RefitTopIO a)
{
    for (int l = 0; l < a.levels; l++) {
        const uint32_t k = a.offset[l] + threadIdx.x;
        if (k < a.offset[l + 1]) refit_node(a.nodes, a.tris, a.list[k]);
        __syncthreads();
    }
}
#endif // __HIPCC__

#endif
