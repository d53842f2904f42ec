// rls_nearest_bvh.hpp -- the tree of librls_nearest.so (include/rlshaders_amd_nearest.h): its node and triangle records and the
// host builder.  Plain C++14, no HIP: nearest.hip builds a scene with it, tests/native/nearest_host_check.cpp checks it on the CPU.
//
// The builder is deterministic: an object-median split on the longest axis of the centroid bounds, the triangles ordered by
// (centroid, index) -- a total order, so the two halves of a split are sets the inputs fix -- the larger half on the left,
// leaves of at most `leaf` triangles sorted by index.  A range of n triangles splits into ceil(n / 2) and floor(n / 2), so
// after k splits no range holds more than ceil(n / 2^k): the depth is at most ceil(log2(nt / leaf)) + 1 levels
// (nearest_depth_bound), and a traversal that holds one sibling per inner level needs a stack of depth - 1 entries.
//
// The result of a query does not depend on the tree (the statement in the public header), only its cost does.
#ifndef RLS_NEAREST_BVH_HPP
#define RLS_NEAREST_BVH_HPP

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

// 32 bytes, two 16-byte loads.  Inner node: first = its left child, the right one is first + 1; leaf: first = its first
// triangle record.  meta: the leaf's triangle count (0: an inner node) | the split axis << 8.
struct alignas(16) NearestNode {
    float lo[3];
    uint32_t first;
    float hi[3];
    uint32_t meta;
};
// 48 bytes, three 16-byte loads: a triangle's vertices in leaf order, so that a leaf reads consecutive records
struct alignas(16) NearestTri {
    float v0[3];
    uint32_t prim;
    float v1[3];
    uint32_t pad1;
    float v2[3];
    uint32_t pad2;
};

constexpr uint32_t kNearestCountMask = 0xFFu;
constexpr int kNearestAxisShift = 8;

struct NearestBvh {
    std::vector<NearestNode> nodes;
    std::vector<NearestTri> tris;
    int depth = 0;
};

// levels of the tree at most: ceil(log2(nt / leaf)) + 1; 0 for no triangles
inline int nearest_depth_bound(int64_t nt, int leaf)
{
    if (nt <= 0) return 0;
    int k = 0;
    while (((int64_t)leaf << k) < nt) k++;
    return k + 1;
}

// the smaller / larger of two floats by the compare written out (the statement's min and max)
constexpr float nearest_minf(float a, float b) { return b < a ? b : a; }
constexpr float nearest_maxf(float a, float b) { return b > a ? b : a; }

// a float's bits as an unsigned key of the same order (a total order: the sort below never sees an unordered pair)
inline uint32_t nearest_order_key(float f)
{
    uint32_t b;
    memcpy(&b, &f, sizeof b);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

namespace nearest_detail {

struct Builder {
    const float *V;
    const uint32_t *tri;
    int leaf;
    std::vector<float> lo, hi;            // [3 * nt]: the triangles' boxes
    std::vector<uint32_t> key;            // [3 * nt]: the centroids' order keys (lo + hi: twice the centre)
    std::vector<uint32_t> order;
    NearestBvh *out;

    void build(uint32_t node, int64_t begin, int64_t end, int level)
    {
        out->depth = std::max(out->depth, level);
        NearestNode n;
        float cmin[3], cmax[3];
        for (int c = 0; c < 3; c++) {
            const uint32_t i0 = order[(size_t)begin];
            n.lo[c] = lo[3 * (size_t)i0 + c];
            n.hi[c] = hi[3 * (size_t)i0 + c];
            cmin[c] = cmax[c] = n.lo[c] + n.hi[c];
            for (int64_t k = begin + 1; k < end; k++) {
                const size_t i = order[(size_t)k];
                n.lo[c] = nearest_minf(n.lo[c], lo[3 * i + c]);
                n.hi[c] = nearest_maxf(n.hi[c], hi[3 * i + c]);
                const float ctr = lo[3 * i + c] + hi[3 * i + c];
                cmin[c] = nearest_minf(cmin[c], ctr);
                cmax[c] = nearest_maxf(cmax[c], ctr);
            }
        }
        const int64_t count = end - begin;
        if (count <= leaf) {
            std::sort(order.begin() + begin, order.begin() + end);
            n.first = (uint32_t)begin;
            n.meta = (uint32_t)count;
            out->nodes[node] = n;
            return;
        }
        int axis = 0;
        float ext = cmax[0] - cmin[0];
        for (int c = 1; c < 3; c++)
            if (cmax[c] - cmin[c] > ext) { ext = cmax[c] - cmin[c]; axis = c; }
        const int64_t mid = begin + (count + 1) / 2;
        const uint32_t *k = key.data();
        std::nth_element(order.begin() + begin, order.begin() + mid, order.begin() + end, [k, axis](uint32_t a, uint32_t b) {
            const uint32_t ka = k[3 * (size_t)a + axis], kb = k[3 * (size_t)b + axis];
            return ka != kb ? ka < kb : a < b;
        });
        const uint32_t left = (uint32_t)out->nodes.size();
        out->nodes.resize(out->nodes.size() + 2);
        n.first = left;
        n.meta = (uint32_t)axis << kNearestAxisShift;
        out->nodes[node] = n;
        build(left, begin, mid, level + 1);
        build(left + 1, mid, end, level + 1);
    }
};

} // namespace nearest_detail

// V: [nv * 3] finite vertices, tri: [nt * 3] indices below nv (the caller has checked both), leaf: 1 .. 8
inline void nearest_build(const float *V, const uint32_t *tri, int64_t nt, int leaf, NearestBvh &out)
{
    out.nodes.clear();
    out.tris.clear();
    out.depth = 0;
    if (nt <= 0) return;
    nearest_detail::Builder b;
    b.V = V; b.tri = tri; b.leaf = leaf; b.out = &out;
    b.lo.resize(3 * (size_t)nt); b.hi.resize(3 * (size_t)nt); b.key.resize(3 * (size_t)nt); b.order.resize((size_t)nt);
    for (size_t i = 0; i < (size_t)nt; i++) {
        b.order[i] = (uint32_t)i;
        const float *v0 = V + 3 * (size_t)tri[3 * i], *v1 = V + 3 * (size_t)tri[3 * i + 1], *v2 = V + 3 * (size_t)tri[3 * i + 2];
        for (int c = 0; c < 3; c++) {
            b.lo[3 * i + c] = nearest_minf(nearest_minf(v0[c], v1[c]), v2[c]);
            b.hi[3 * i + c] = nearest_maxf(nearest_maxf(v0[c], v1[c]), v2[c]);
            b.key[3 * i + c] = nearest_order_key(b.lo[3 * i + c] + b.hi[3 * i + c]);
        }
    }
    out.nodes.reserve(2 * (size_t)nt);
    out.nodes.resize(1);
    b.build(0, 0, nt, 1);
    out.tris.resize((size_t)nt);
    for (size_t k = 0; k < (size_t)nt; k++) {
        const size_t i = b.order[k];
        NearestTri t = {};
        for (int c = 0; c < 3; c++) {
            t.v0[c] = V[3 * (size_t)tri[3 * i] + c];
            t.v1[c] = V[3 * (size_t)tri[3 * i + 1] + c];
            t.v2[c] = V[3 * (size_t)tri[3 * i + 2] + c];
        }
        t.prim = (uint32_t)i;
        out.tris[k] = t;
    }
}

#endif
