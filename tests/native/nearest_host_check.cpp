// nearest_host_check.cpp -- the tree and the traversal of librls_nearest.so on the CPU: rls_nearest_bvh.hpp and the host + device
// functions of rls_nearest_device.hpp compiled for the host with -ffp-contract=off, no HIP.
//
//   nearest_host_check bvh                the tree's invariants for leaf_size 1, 2, 4, 8 and nt = 0, 1, 2, 3, 1025 (and the meshes
//                                         below): every triangle in exactly one leaf, every node's box contains its children's
//                                         and its triangles', the depth within ceil(log2(nt / leaf)) + 1, leaves within leaf_size
//   nearest_host_check traverse [rays]    the traversal against THIS program's brute force over the statement of
//                                         include/rlshaders_amd_nearest.h (restated below, independently of the library's
//                                         source), bit for bit in (hit, t, prim), on `rays` rays (default 1 000 000) over an
//                                         icosphere (320 triangles), a 33 x 33 quad grid and a 1025-triangle soup with degenerate
//                                         triangles, for every leaf_size: random rays, rays at vertices and edges, axis-parallel
//                                         rays with signed zeros, origins on box planes, NaN / inf components, hostile reaches,
//                                         skipped triangles
//   nearest_host_check file <mesh.bin> <rays.bin> <out.bin> [leaf]
//                                         the brute force over a mesh and a ray stream that tests/nearest_host_check_util.py
//                                         wrote (a reference that scales to 2^22 triangles), on min(hardware threads, 16)
//                                         threads.  mesh.bin: int64 nv, nt; float V[nv * 3]; uint32 T[nt * 3].  rays.bin: int64
//                                         rays; 8 words a ray: o.xyz, d.xyz, maxdist (float), skip (uint32).  out.bin, a ray:
//                                         the brute force's prim (0xFFFFFFFF: none), t (float).  With leaf the tree is built,
//                                         its invariants are checked (exit 1 where one fails) and the traversal runs too: out.bin
//                                         then holds 7 words a ray, the two above and the traversal's prim, t, nodes, triangles,
//                                         max_stack (the most stack entries held).  Prints one line: the tree's depth and nodes,
//                                         the hits and how many rays differ; the caller compares the words.
// Prints "ok ..." lines and exits 0, or the first differences and exits 1.  tests/test_nearest_bvh.py,
// tests/test_nearest_host_traversal.py and tests/test_nearest_deep.py drive it, the latter two once more under
// -fsanitize=address,undefined.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <thread>
#include <utility>
#include <vector>

#include "../../rlshaders_amd/csrc_nearest/rls_nearest_device.hpp"

namespace {

struct Mesh {
    std::vector<float> V;        // xyz
    std::vector<uint32_t> T;
    int64_t nt() const { return (int64_t)T.size() / 3; }
};

struct Rng {                     // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    double range(double a, double b) { return a + (b - a) * uni(); }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

Mesh icosphere(int level)
{
    const double g = (1 + sqrt(5.0)) / 2;
    std::vector<double> V = { -1, g, 0, 1, g, 0, -1, -g, 0, 1, -g, 0, 0, -1, g, 0, 1, g, 0, -1, -g, 0, 1, -g, g, 0, -1, g, 0, 1, -g, 0, -1, -g, 0, 1 };
    std::vector<uint32_t> T = { 0, 11, 5, 0, 5, 1, 0, 1, 7, 0, 7, 10, 0, 10, 11, 1, 5, 9, 5, 11, 4, 11, 10, 2, 10, 7, 6, 7, 1, 8,
                                3, 9, 4, 3, 4, 2, 3, 2, 6, 3, 6, 8, 3, 8, 9, 4, 9, 5, 2, 4, 11, 6, 2, 10, 8, 6, 7, 9, 8, 1 };
    auto norm = [&](size_t i) { const double l = sqrt(V[3 * i] * V[3 * i] + V[3 * i + 1] * V[3 * i + 1] + V[3 * i + 2] * V[3 * i + 2]); for (int c = 0; c < 3; c++) V[3 * i + c] /= l; };
    for (size_t i = 0; i < 12; i++) norm(i);
    for (int l = 0; l < level; l++) {
        std::map<std::pair<uint32_t, uint32_t>, uint32_t> mid;
        auto middle = [&](uint32_t a, uint32_t b) {
            const auto key = std::make_pair(a < b ? a : b, a < b ? b : a);
            auto it = mid.find(key);
            if (it != mid.end()) return it->second;
            const uint32_t i = (uint32_t)(V.size() / 3);
            for (int c = 0; c < 3; c++) V.push_back(V[3 * a + c] + V[3 * b + c]);
            norm(i);
            mid[key] = i;
            return i;
        };
        std::vector<uint32_t> T2;
        for (size_t t = 0; t < T.size(); t += 3) {
            const uint32_t a = T[t], b = T[t + 1], c = T[t + 2], ab = middle(a, b), bc = middle(b, c), ca = middle(c, a);
            const uint32_t add[12] = { a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca };
            T2.insert(T2.end(), add, add + 12);
        }
        T.swap(T2);
    }
    Mesh m;
    for (double v : V) m.V.push_back((float)v);
    m.T = T;
    return m;
}

Mesh quad_grid(int n)
{
    Mesh m;
    for (int j = 0; j <= n; j++)
        for (int i = 0; i <= n; i++) {
            const double x = -1 + 2.0 * i / n, y = -1 + 2.0 * j / n;
            m.V.push_back((float)x); m.V.push_back((float)y); m.V.push_back((float)(0.1 * sin(3 * x) * cos(2 * y)));
        }
    for (int j = 0; j < n; j++)
        for (int i = 0; i < n; i++) {
            const uint32_t a = (uint32_t)(j * (n + 1) + i), add[6] = { a, a + 1, a + (uint32_t)n + 2, a, a + (uint32_t)n + 2, a + (uint32_t)n + 1 };
            m.T.insert(m.T.end(), add, add + 6);
        }
    return m;
}

// random small triangles; every 16th degenerate (a repeated index, collinear vertices, a duplicated vertex), every 64th flat in an
// axis plane
Mesh soup(int nt, uint64_t seed)
{
    Rng r = { seed };
    Mesh m;
    for (int i = 0; i < nt; i++) {
        const double c[3] = { r.range(-1, 1), r.range(-1, 1), r.range(-1, 1) };
        for (int v = 0; v < 3; v++)
            for (int k = 0; k < 3; k++) m.V.push_back((float)(c[k] + r.range(-0.2, 0.2)));
        for (uint32_t v = 0; v < 3; v++) m.T.push_back(3 * (uint32_t)i + v);
        float *p = &m.V[9 * (size_t)i];
        if (i % 16 == 0) {
            const int kind = (i / 16) % 3;
            if (kind == 0) m.T[3 * (size_t)i + 2] = m.T[3 * (size_t)i + 1];
            else if (kind == 1) for (int k = 0; k < 3; k++) p[6 + k] = p[k] + (p[3 + k] - p[k]) * 2.0f;
            else for (int k = 0; k < 3; k++) p[6 + k] = p[3 + k];
        } else if (i % 64 == 5) {
            const int axis = (i / 64) % 3;
            p[3 + axis] = p[6 + axis] = p[axis];
        }
    }
    return m;
}

// ---- the tree's invariants -------------------------------------------------------------------------------------------------------
int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

void check_built(const Mesh &m, const NearestBvh &b, int leaf, const char *what)
{
    const int64_t nt = m.nt();
    CHECK(b.depth <= nearest_depth_bound(nt, leaf), "%s leaf %d: depth %d > bound %d", what, leaf, b.depth, nearest_depth_bound(nt, leaf));
    CHECK(b.depth - 1 <= kNearestStack, "%s: depth %d past the stack", what, b.depth);
    CHECK((int64_t)b.tris.size() == nt, "%s: %zu records for %lld triangles", what, b.tris.size(), (long long)nt);
    if (nt == 0) { CHECK(b.nodes.empty() && b.depth == 0, "%s: an empty mesh has nodes", what); return; }
    std::vector<int> seen((size_t)nt, 0), slot((size_t)nt, 0), reached(b.nodes.size(), 0);
    int deepest = 0;
    std::vector<std::pair<uint32_t, int>> todo = { { 0u, 1 } };
    while (!todo.empty()) {
        const uint32_t at = todo.back().first;
        const int level = todo.back().second;
        todo.pop_back();
        CHECK(at < b.nodes.size(), "%s: node %u past the array", what, at);
        if (at >= b.nodes.size()) continue;
        CHECK(reached[at]++ == 0, "%s: node %u reached twice", what, at);
        deepest = level > deepest ? level : deepest;
        const NearestNode &n = b.nodes[at];
        const uint32_t count = n.meta & kNearestCountMask;
        if (count == 0) {
            CHECK((n.meta >> kNearestAxisShift) < 3, "%s: node %u axis", what, at);
            for (uint32_t c = n.first; c < n.first + 2 && c < b.nodes.size(); c++) {
                for (int k = 0; k < 3; k++)
                    CHECK(n.lo[k] <= b.nodes[c].lo[k] && b.nodes[c].hi[k] <= n.hi[k], "%s: node %u does not contain child %u", what, at, c);
                todo.push_back({ c, level + 1 });
            }
            continue;
        }
        CHECK((int)count <= leaf, "%s: leaf %u holds %u > %d", what, at, count, leaf);
        for (uint32_t k = n.first; k < n.first + count; k++) {
            CHECK(k < (uint32_t)nt, "%s: leaf %u record %u past the array", what, at, k);
            if (k >= (uint32_t)nt) continue;
            const NearestTri &t = b.tris[k];
            CHECK(t.prim < (uint32_t)nt && seen[t.prim]++ == 0, "%s: triangle %u in two leaves", what, t.prim);
            CHECK(slot[k]++ == 0, "%s: record %u in two leaves", what, k);
            CHECK(k == n.first || b.tris[k - 1].prim < t.prim, "%s: leaf %u is not sorted by index", what, at);
            const float *vs[3] = { t.v0, t.v1, t.v2 };
            for (int v = 0; v < 3; v++)
                for (int c = 0; c < 3; c++) {
                    CHECK(vs[v][c] == m.V[3 * (size_t)m.T[3 * (size_t)t.prim + v] + c], "%s: record %u is not triangle %u", what, k, t.prim);
                    CHECK(n.lo[c] <= vs[v][c] && vs[v][c] <= n.hi[c], "%s: leaf %u does not contain triangle %u", what, at, t.prim);
                }
        }
    }
    for (int64_t i = 0; i < nt; i++) CHECK(seen[(size_t)i] == 1, "%s leaf %d: triangle %lld in %d leaves", what, leaf, (long long)i, seen[(size_t)i]);
    for (size_t i = 0; i < b.nodes.size(); i++) CHECK(reached[i] == 1, "%s: node %zu reached %d times", what, i, reached[i]);
    CHECK(deepest == b.depth, "%s: depth %d reported, %d found", what, b.depth, deepest);
}

void check_tree(const Mesh &m, int leaf, const char *what)
{
    NearestBvh b;
    const int64_t nt = m.nt();
    nearest_build(m.V.data(), m.T.data(), nt, leaf, b);
    check_built(m, b, leaf, what);
    if (nt == 0) return;
    // the same inputs give the same tree
    NearestBvh again;
    nearest_build(m.V.data(), m.T.data(), nt, leaf, again);
    CHECK(again.nodes.size() == b.nodes.size() && !memcmp(again.nodes.data(), b.nodes.data(), b.nodes.size() * sizeof(NearestNode)) &&
              !memcmp(again.tris.data(), b.tris.data(), b.tris.size() * sizeof(NearestTri)), "%s: a second build differs", what);
}

int run_bvh()
{
    const int leaves[4] = { 1, 2, 4, 8 }, sizes[5] = { 0, 1, 2, 3, 1025 };
    for (int leaf : leaves) {
        for (int nt : sizes) {
            char what[64];
            snprintf(what, sizeof what, "soup %d", nt);
            check_tree(soup(nt, 7 + (uint64_t)nt), leaf, what);
        }
        check_tree(icosphere(2), leaf, "icosphere");
        check_tree(quad_grid(33), leaf, "quad grid");
        Mesh same = soup(64, 3);                                     // 64 copies of one triangle: every centroid ties
        for (size_t i = 9; i < same.V.size(); i++) same.V[i] = same.V[i % 9];
        for (size_t i = 0; i < same.T.size(); i++) same.T[i] = (uint32_t)i;
        check_tree(same, leaf, "coincident");
    }
    // the depth bound at the limit's end of the range (such a tree is built by the file mode, tests/test_nearest_deep.py): 2^22
    // triangles at leaf 1 need 23 levels, 22 entries
    CHECK(nearest_depth_bound((int64_t)1 << 22, 1) - 1 <= kNearestStack, "the triangle limit does not fit the stack");
    if (fails) return 1;
    printf("ok bvh\n");
    return 0;
}

// ---- this program's brute force: the statement restated, not the library's functions --------------------------------------------
struct Result { uint32_t prim; float t; };

inline bool sign_bit(float f) { uint32_t b; memcpy(&b, &f, 4); return (b >> 31) != 0; }

Result brute(const Mesh &m, const float o[3], const float d[3], float reach, uint32_t skip)
{
    Result best = { 0xFFFFFFFFu, 0.0f };
    const float ix = 1.0f / d[0], iy = 1.0f / d[1], iz = 1.0f / d[2];
    const float inv[3] = { ix, iy, iz };
    for (int64_t i = 0; i < m.nt(); i++) {
        if ((uint32_t)i == skip) continue;
        const float *a = &m.V[3 * (size_t)m.T[3 * i]], *b = &m.V[3 * (size_t)m.T[3 * i + 1]], *c = &m.V[3 * (size_t)m.T[3 * i + 2]];
        float tn = 0.0f, tf = INFINITY;
        for (int k = 0; k < 3; k++) {
            float lo = a[k], hi = a[k];
            if (b[k] < lo) lo = b[k];
            if (c[k] < lo) lo = c[k];
            if (b[k] > hi) hi = b[k];
            if (c[k] > hi) hi = c[k];
            float t0 = (lo - o[k]) * inv[k], t1 = (hi - o[k]) * inv[k];
            if (sign_bit(inv[k])) { float s = t0; t0 = t1; t1 = s; }
            if (t0 > tn) tn = t0;
            if (t1 < tf) tf = t1;
        }
        if (tn > tf) continue;
        const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2], e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
        const float px = d[1] * e2z - d[2] * e2y, py = d[2] * e2x - d[0] * e2z, pz = d[0] * e2y - d[1] * e2x;
        const float det = (e1x * px + e1y * py) + e1z * pz;
        if (!(det < 0.0f || det > 0.0f)) continue;
        const float r = 1.0f / det, sx = o[0] - a[0], sy = o[1] - a[1], sz = o[2] - a[2];
        const float u = ((sx * px + sy * py) + sz * pz) * r;
        const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
        const float v = ((d[0] * qx + d[1] * qy) + d[2] * qz) * r;
        const float tm = ((e2x * qx + e2y * qy) + e2z * qz) * r;
        if (!(u >= 0.0f && v >= 0.0f && u + v <= 1.0f) || tm != tm) continue;
        float t = tm;
        if (tn > t) t = tn;
        if (tf < t) t = tf;
        if (!(t > 0.0f) || !(t <= reach)) continue;
        if (best.prim == 0xFFFFFFFFu || t < best.t) { best.prim = (uint32_t)i; best.t = t; }   // ascending i: a tie keeps the smaller
    }
    return best;
}

struct Ray { float o[3], d[3], m; uint32_t skip; };

// ray k of a mesh's stream: a function of (mesh, k, seed) alone, a mix of the kinds the header of this file lists
Ray make_ray(const Mesh &m, uint64_t k, uint64_t seed)
{
    Rng r = { seed * 0x100000001B3ull + k };
    Ray q;
    const float inf = INFINITY;
    q.m = inf; q.skip = 0xFFFFFFFFu;
    const int64_t nt = m.nt();
    const size_t nv = m.V.size() / 3;
    const int kind = (int)(k % 16);
    for (int c = 0; c < 3; c++) q.o[c] = (float)r.range(-1.6, 1.6);
    if (kind < 6) {                                                  // origin in a cube, towards a point of a smaller one
        for (int c = 0; c < 3; c++) q.d[c] = (float)r.range(-1, 1) - q.o[c];
    } else if (kind < 9) {                                           // exactly at a vertex, or at a point of an edge
        const uint32_t t = r.below((uint32_t)nt), e = r.below(3);
        const float *a = &m.V[3 * (size_t)m.T[3 * (size_t)t + e]], *b = &m.V[3 * (size_t)m.T[3 * (size_t)t + (e + 1) % 3]];
        const float w = kind == 6 ? 0.0f : kind == 7 ? 0.5f : (float)r.uni();
        for (int c = 0; c < 3; c++) q.d[c] = (a[c] + (b[c] - a[c]) * w) - q.o[c];
    } else if (kind < 12) {                                          // axis-parallel through a vertex's planes, signed zeros
        const float *p = &m.V[3 * (size_t)r.below((uint32_t)nv)];
        const int axis = kind - 9;
        const uint64_t bits = r.next();
        for (int c = 0; c < 3; c++) {
            q.o[c] = (bits >> c & 1) ? p[c] : p[c] + (float)r.range(-0.05, 0.05);   // on the vertex's plane: a box plane
            q.d[c] = (bits >> (3 + c) & 1) ? -0.0f : 0.0f;
        }
        q.d[axis] = (bits >> 8 & 1) ? 1.0f : -1.0f;
        q.o[axis] = p[axis] - q.d[axis] * (float)((bits >> 9 & 1) ? 2.0 : 0.0);      // also an origin ON the plane it aims along
    } else if (kind == 12) {                                         // a hostile reach
        const float reach[8] = { 0.0f, -0.0f, NAN, -1.0f, inf, 1e-30f, 0.5f, -inf };
        for (int c = 0; c < 3; c++) q.d[c] = (float)r.range(-1, 1) - q.o[c];
        q.m = reach[r.below(8)];
    } else if (kind == 13) {                                         // a non-finite or huge or subnormal component
        const float bad[8] = { NAN, inf, -inf, 3e38f, -3e38f, 1e-40f, -1e-40f, 0.0f };
        for (int c = 0; c < 3; c++) q.d[c] = (float)r.range(-1, 1) - q.o[c];
        const uint32_t n = 1 + r.below(2);
        for (uint32_t i = 0; i < n; i++) (r.below(2) ? q.o : q.d)[r.below(3)] = bad[r.below(8)];
        if (r.below(4) == 0) q.m = (float)r.range(0, 3);
    } else {                                                         // a finite reach about the hit, and a skipped triangle
        for (int c = 0; c < 3; c++) q.d[c] = (float)r.range(-1, 1) - q.o[c];
        q.m = (float)r.range(0.2, 1.5);
        if (kind == 15) {
            const Result first = brute(m, q.o, q.d, inf, 0xFFFFFFFFu);
            q.skip = first.prim != 0xFFFFFFFFu && r.below(4) ? first.prim : r.below((uint32_t)nt);
            if (first.prim != 0xFFFFFFFFu && r.below(2)) q.m = r.below(2) ? first.t : nextafterf(first.t, r.below(2) ? 0.0f : inf);
            else q.m = inf;
        }
    }
    return q;
}

unsigned pool_size(unsigned cap)
{
    const unsigned threads = std::thread::hardware_concurrency();
    return threads < 1 ? 1 : threads > cap ? cap : threads;
}

struct Tally { int64_t rays = 0, hits = 0, nodes = 0, tris = 0, bad = 0; };

void run_range(const Mesh &m, const NearestBvh &b, uint64_t seed, uint64_t begin, uint64_t end, Tally *out)
{
    Tally t;
    for (uint64_t k = begin; k < end; k++) {
        const Ray q = make_ray(m, k, seed);
        const Result want = brute(m, q.o, q.d, q.m, q.skip);
        const NearestRay r = nearest_ray(q.o, q.d, q.m, q.skip);
        uint32_t stack[kNearestStack];
        NearestStats st;
        const NearestBest got = nearest_traverse(b.nodes.data(), (int64_t)b.nodes.size(), b.tris.data(), r,
                                                 [&](int i) -> uint32_t & { return stack[i]; }, st);
        const bool same = got.prim == want.prim && (want.prim == 0xFFFFFFFFu || !memcmp(&got.t, &want.t, 4));
        if (!same && t.bad++ < 5)
            printf("FAIL ray %llu: o %a %a %a d %a %a %a m %a skip %u: traversal prim %u t %a, brute force prim %u t %a\n",
                   (unsigned long long)k, q.o[0], q.o[1], q.o[2], q.d[0], q.d[1], q.d[2], q.m, q.skip, got.prim, got.t, want.prim, want.t);
        t.rays++; t.hits += want.prim != 0xFFFFFFFFu; t.nodes += st.nodes; t.tris += st.tris;
    }
    *out = t;
}

int run_traverse(int64_t total)
{
    struct Case { const char *name; Mesh m; double share; } cases[3] = {
        { "icosphere", icosphere(2), 0.6 }, { "quad grid", quad_grid(33), 0.1 }, { "soup", soup(1025, 1032), 0.3 } };
    const int leaves[4] = { 1, 2, 4, 8 };
    const unsigned threads = pool_size(8);
    int64_t bad = 0, done = 0;
    for (int ci = 0; ci < 3; ci++) {
        const Case &c = cases[ci];
        const int64_t per_leaf = (int64_t)(total * c.share / 4) + 1;
        for (int leaf : leaves) {
            NearestBvh b;
            nearest_build(c.m.V.data(), c.m.T.data(), c.m.nt(), leaf, b);
            std::vector<Tally> t(threads);
            std::vector<std::thread> pool;
            for (unsigned w = 0; w < threads; w++)
                pool.emplace_back(run_range, std::cref(c.m), std::cref(b), 1000u * (unsigned)leaf + (unsigned)ci,
                                  (uint64_t)(per_leaf * w / threads), (uint64_t)(per_leaf * (w + 1) / threads), &t[w]);
            for (auto &th : pool) th.join();
            Tally sum;
            for (const Tally &x : t) { sum.rays += x.rays; sum.hits += x.hits; sum.nodes += x.nodes; sum.tris += x.tris; sum.bad += x.bad; }
            printf("%s %s leaf %d: %lld rays, %lld hits, %.1f nodes and %.1f triangles a ray, %lld differ\n", sum.bad ? "FAIL" : "ok",
                   c.name, leaf, (long long)sum.rays, (long long)sum.hits, (double)sum.nodes / (double)sum.rays,
                   (double)sum.tris / (double)sum.rays, (long long)sum.bad);
            bad += sum.bad; done += sum.rays;
            if (sum.hits * 5 < sum.rays) { printf("FAIL %s: too few rays hit for the check to mean much\n", c.name); bad++; }
        }
    }
    // an empty scene: no node, every ray misses
    NearestBvh none;
    nearest_build(nullptr, nullptr, 0, 4, none);
    const float o[3] = { 0, 0, 0 }, d[3] = { 0, 0, 1 };
    NearestNoStats ns;
    uint32_t stack[kNearestStack];
    bad += nearest_traverse(none.nodes.data(), 0, none.tris.data(), nearest_ray(o, d, INFINITY, 0xFFFFFFFFu),
                            [&](int i) -> uint32_t & { return stack[i]; }, ns).prim != 0xFFFFFFFFu;
    printf("%s traverse: %lld rays, %lld differ\n", bad ? "FAIL" : "ok", (long long)done, (long long)bad);
    return bad ? 1 : 0;
}

// ---- a mesh and a ray stream from files ------------------------------------------------------------------------------------------
template <class T>
bool read_all(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

constexpr int kBruteWords = 2, kFileWords = 7;

void file_range(const Mesh &m, const NearestBvh *b, const uint32_t *rays, uint32_t *out, int words, int64_t begin, int64_t end,
                Tally *tally)
{
    Tally t;
    for (int64_t k = begin; k < end; k++) {
        Ray q;
        memcpy(&q, rays + 8 * k, sizeof q);
        uint32_t *w = out + (size_t)words * (size_t)k;
        const Result want = brute(m, q.o, q.d, q.m, q.skip);
        w[0] = want.prim;
        memcpy(&w[1], &want.t, 4);
        t.rays++; t.hits += want.prim != 0xFFFFFFFFu;
        if (!b) continue;
        const NearestRay r = nearest_ray(q.o, q.d, q.m, q.skip);
        uint32_t stack[kNearestStack];
        NearestStats st;
        const NearestBest got = nearest_traverse(b->nodes.data(), (int64_t)b->nodes.size(), b->tris.data(), r,
                                                 [&](int i) -> uint32_t & { return stack[i]; }, st);
        w[2] = got.prim;
        memcpy(&w[3], &got.t, 4);
        w[4] = (uint32_t)st.nodes; w[5] = (uint32_t)st.tris; w[6] = (uint32_t)st.max_stack;
        t.nodes += st.nodes; t.tris += st.tris;
        t.bad += !(got.prim == want.prim && (want.prim == 0xFFFFFFFFu || !memcmp(&got.t, &want.t, 4)));
    }
    *tally = t;
}

int run_file(const char *mesh_path, const char *rays_path, const char *out_path, int leaf)
{
    static_assert(sizeof(Ray) == 32, "a ray record is 8 words");
    Mesh m;
    std::vector<uint32_t> rays;
    int64_t head[2] = { 0, 0 }, count = 0;
    FILE *f = fopen(mesh_path, "rb");
    bool ok = f && fread(head, sizeof(int64_t), 2, f) == 2 && head[0] >= 0 && head[1] >= 0 && head[1] <= ((int64_t)1 << 22) &&
              head[0] <= 3 * head[1] + 3;
    if (ok) {
        m.V.resize(3 * (size_t)head[0]); m.T.resize(3 * (size_t)head[1]);
        ok = read_all(f, m.V) && read_all(f, m.T);
        for (uint32_t i : m.T) ok = ok && (int64_t)i < head[0];
    }
    if (f) fclose(f);
    if (!ok) { fprintf(stderr, "nearest_host_check: %s is missing, short or malformed\n", mesh_path); return 2; }
    f = fopen(rays_path, "rb");
    ok = f && fread(&count, sizeof(int64_t), 1, f) == 1 && count >= 0 && count <= ((int64_t)1 << 24);
    if (ok) {
        rays.resize(8 * (size_t)count);
        ok = read_all(f, rays);
    }
    if (f) fclose(f);
    if (!ok) { fprintf(stderr, "nearest_host_check: %s is missing, short or malformed\n", rays_path); return 2; }
    if (leaf < 0 || leaf > 8) { fprintf(stderr, "nearest_host_check: leaf 1 .. 8\n"); return 2; }
    NearestBvh b;
    if (leaf) {
        nearest_build(m.V.data(), m.T.data(), m.nt(), leaf, b);
        check_built(m, b, leaf, "file");
    }
    const int words = leaf ? kFileWords : kBruteWords;
    std::vector<uint32_t> out((size_t)words * (size_t)count);
    const unsigned threads = pool_size(16);
    std::vector<Tally> t(threads);
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < threads; w++)
        pool.emplace_back(file_range, std::cref(m), leaf ? &b : nullptr, rays.data(), out.data(), words, count * w / threads,
                          count * (w + 1) / threads, &t[w]);
    for (auto &th : pool) th.join();
    Tally sum;
    for (const Tally &x : t) { sum.rays += x.rays; sum.hits += x.hits; sum.nodes += x.nodes; sum.tris += x.tris; sum.bad += x.bad; }
    f = fopen(out_path, "wb");
    ok = f && (out.empty() || fwrite(out.data(), 4, out.size(), f) == out.size());
    if (f) ok = fclose(f) == 0 && ok;
    if (!ok) { fprintf(stderr, "nearest_host_check: cannot write %s\n", out_path); return 2; }
    if (fails) return 1;
    printf("ok file: nt %lld leaf %d depth %d nodes %lld rays %lld hits %lld differ %lld\n", (long long)m.nt(), leaf, b.depth,
           (long long)b.nodes.size(), (long long)sum.rays, (long long)sum.hits, (long long)sum.bad);
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "bvh")) return run_bvh();
    if (argc >= 2 && !strcmp(argv[1], "traverse")) return run_traverse(argc >= 3 ? atoll(argv[2]) : 1000000);
    if (argc >= 5 && !strcmp(argv[1], "file")) return run_file(argv[2], argv[3], argv[4], argc >= 6 ? atoi(argv[5]) : 0);
    fprintf(stderr, "usage: nearest_host_check bvh | traverse [rays] | file <mesh.bin> <rays.bin> <out.bin> [leaf]\n");
    return 2;
}
