// nearest_refit_host_check.cpp -- the refit of librls_nearest_refit.so on the CPU: the product's builder (rls_nearest_bvh.hpp), the
// refit's own source (rls_nearest_refit.hpp) and the traversal (rls_nearest_device.hpp) compiled for the host with
// -ffp-contract=off, no HIP.
//
//   nearest_refit_host_check <pair.bin> <rays> <leaf>
//
// pair.bin: int64 nv, nt; float A[nv * 3]; float B[nv * 3]; uint32 T[nt * 3] (tests/nearest_refit_util.py writes it).  A is
// finite; B may hold NaN and infinities.  The tree is built on A, then refit to B, and
//   - every node box == the exact union of what is below it, recomputed here from B (not with the refit's functions);
//   - first, meta and the order of the triangle ids are those of the built tree; every record holds B's vertices, or three
//     vertices at the origin where the triangle has a non-finite coordinate, and the refit's parked count is this program's;
//   - the traversal over the refit tree == this program's brute force over the statement on B, parked triangles never
//     hitting, bit for bit in (hit, t, prim), on `rays` rays: aimed at triangles, random, axis-parallel with signed zeros,
//     non-finite components, hostile reaches, skipped triangles;
//   - a refit back to A restores every box and every record by value.
// It also counts the nodes and triangles a ray visits on the refit tree and, where B is finite, on a tree rebuilt from B.
// Prints one "ok pair: ..." line and exits 0, or the first differences and exits 1.  tests/test_nearest_refit_host.py drives
// it, once more under -fsanitize=address,undefined.
//
//   nearest_refit_host_check tree <pair.bin> <leaf> <out.bin>
//
// writes the tree the builder makes on A -- the tree a scene on A holds: int64 nodes, nt; uint32 (first, meta)[nodes];
// uint32 prim[nt] in leaf order; float (lo xyz, hi xyz)[nodes] -- what rls_nearest_refit_read_tree returns, without a device.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <thread>
#include <vector>

#include "../../rlshaders_amd/csrc_nearest/rls_nearest_device.hpp"
#include "../../rlshaders_amd/csrc_nearest/rls_nearest_refit.hpp"

namespace {

int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Rng {                     // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    double range(double a, double b) { return a + (b - a) * uni(); }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

struct Pair {
    int64_t nv = 0, nt = 0;
    std::vector<float> A, B;
    std::vector<uint32_t> T;
};

bool is_finite(float f) { uint32_t b; memcpy(&b, &f, 4); return (b & 0x7F800000u) != 0x7F800000u; }

bool parked(const Pair &p, const std::vector<float> &V, int64_t i)
{
    for (int v = 0; v < 3; v++)
        for (int c = 0; c < 3; c++)
            if (!is_finite(V[3 * (size_t)p.T[3 * i + v] + c])) return true;
    return false;
}

// ---- the exact union, by this program ----------------------------------------------------------------------------------------------
struct Box { float lo[3], hi[3]; };

Box want_box(const Pair &p, const std::vector<float> &V, const NearestBvh &b, uint32_t node)
{
    const NearestNode &n = b.nodes[node];
    const uint32_t count = n.meta & kNearestCountMask;
    Box w;
    if (count == 0) {
        const Box l = want_box(p, V, b, n.first), r = want_box(p, V, b, n.first + 1);
        for (int c = 0; c < 3; c++) { w.lo[c] = r.lo[c] < l.lo[c] ? r.lo[c] : l.lo[c]; w.hi[c] = r.hi[c] > l.hi[c] ? r.hi[c] : l.hi[c]; }
        return w;
    }
    bool first = true;
    for (uint32_t k = n.first; k < n.first + count; k++) {
        const int64_t i = b.tris[k].prim;
        const bool park = parked(p, V, i);
        for (int v = 0; v < 3; v++)
            for (int c = 0; c < 3; c++) {
                const float x = park ? 0.0f : V[3 * (size_t)p.T[3 * i + v] + c];
                if (first && v == 0) { w.lo[c] = w.hi[c] = x; continue; }
                if (x < w.lo[c]) w.lo[c] = x;
                if (x > w.hi[c]) w.hi[c] = x;
            }
        first = false;
    }
    return w;
}

int64_t check_refit(const Pair &p, const std::vector<float> &V, const NearestBvh &built, const NearestBvh &b, const char *what)
{
    int64_t park = 0;
    CHECK(b.nodes.size() == built.nodes.size() && b.tris.size() == built.tris.size(), "%s: sizes changed", what);
    for (size_t n = 0; n < b.nodes.size(); n++) {
        CHECK(b.nodes[n].first == built.nodes[n].first && b.nodes[n].meta == built.nodes[n].meta, "%s: node %zu's links changed", what, n);
        const Box w = want_box(p, V, b, (uint32_t)n);
        for (int c = 0; c < 3; c++)
            CHECK(b.nodes[n].lo[c] == w.lo[c] && b.nodes[n].hi[c] == w.hi[c], "%s: node %zu axis %d holds [%a, %a], the union is [%a, %a]", what,
                  n, c, b.nodes[n].lo[c], b.nodes[n].hi[c], w.lo[c], w.hi[c]);
    }
    for (size_t k = 0; k < b.tris.size(); k++) {
        const NearestTri &t = b.tris[k];
        CHECK(t.prim == built.tris[k].prim, "%s: record %zu holds triangle %u, was %u", what, k, t.prim, built.tris[k].prim);
        const bool pk = parked(p, V, t.prim);
        park += pk;
        const float *vs[3] = { t.v0, t.v1, t.v2 };
        for (int v = 0; v < 3; v++)
            for (int c = 0; c < 3; c++) {
                const float x = pk ? 0.0f : V[3 * (size_t)p.T[3 * (size_t)t.prim + v] + c];
                CHECK(!memcmp(&vs[v][c], &x, 4), "%s: record %zu vertex %d axis %d holds %a, not %a", what, k, v, c, vs[v][c], x);
            }
    }
    return park;
}

// ---- this program's brute force: the statement restated; a parked triangle never hits ----------------------------------------------
struct Result { uint32_t prim; float t; };
inline bool sign_bit(float f) { uint32_t b; memcpy(&b, &f, 4); return (b >> 31) != 0; }

Result brute(const Pair &p, const std::vector<float> &V, const std::vector<char> &park, const float o[3], const float d[3], float reach,
             uint32_t skip)
{
    Result best = { 0xFFFFFFFFu, 0.0f };
    const float inv[3] = { 1.0f / d[0], 1.0f / d[1], 1.0f / d[2] };
    for (int64_t i = 0; i < p.nt; i++) {
        if ((uint32_t)i == skip || park[(size_t)i]) continue;
        const float *a = &V[3 * (size_t)p.T[3 * i]], *b = &V[3 * (size_t)p.T[3 * i + 1]], *c = &V[3 * (size_t)p.T[3 * i + 2]];
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

// ray k: a function of (B, k) alone
Ray make_ray(const Pair &p, const std::vector<float> &V, const std::vector<char> &park, uint64_t k)
{
    Rng r = { 0x5EEDull * 0x100000001B3ull + k };
    Ray q;
    q.m = INFINITY; q.skip = 0xFFFFFFFFu;
    const int kind = (int)(k % 16);
    for (int c = 0; c < 3; c++) { q.o[c] = (float)r.range(-1.6, 1.6); q.d[c] = (float)r.range(-1, 1) - q.o[c]; }
    if (p.nt == 0) return q;
    uint32_t t = r.below((uint32_t)p.nt);
    for (int tries = 0; tries < 8 && park[t]; tries++) t = r.below((uint32_t)p.nt);
    const float *a = &V[3 * (size_t)p.T[3 * (size_t)t]], *b = &V[3 * (size_t)p.T[3 * (size_t)t + 1]], *c = &V[3 * (size_t)p.T[3 * (size_t)t + 2]];
    if (kind < 9) {                                                  // towards a point of a triangle, from about it
        if (park[t]) return q;                                       // (none found that is not parked: the random ray)
        double w0 = r.uni(), w1 = r.uni();
        if (w0 + w1 > 1) { w0 = 1 - w0; w1 = 1 - w1; }
        if (kind == 7) { w0 = 0; w1 = 0; }                           // exactly at a vertex
        if (kind == 8) w1 = 0;                                       // on an edge
        double dir[3], len = 0;
        for (int x = 0; x < 3; x++) { dir[x] = r.range(-1, 1); len += dir[x] * dir[x]; }
        len = sqrt(len) + 1e-30;
        const double spread = kind < 3 ? 3.0 : r.range(0.05, 2.0);
        for (int x = 0; x < 3; x++) {
            const double target = (double)a[x] + ((double)b[x] - a[x]) * w0 + ((double)c[x] - a[x]) * w1;
            const double scale = fabs(target) > 4.0 ? fabs(target) : 1.0;   // (coordinates up to 3e38: stay about the target)
            q.o[x] = (float)(target + spread * scale * dir[x] / len);
            q.d[x] = (float)(target - (double)q.o[x]);
        }
        if (kind == 6) { q.m = (float)r.range(0.2, 1.5); q.skip = r.below(4) ? t : r.below((uint32_t)p.nt); }
    } else if (kind < 12) {                                          // axis-parallel through a vertex's planes, signed zeros
        const int axis = kind - 9;
        const uint64_t bits = r.next();
        for (int x = 0; x < 3; x++) {
            q.o[x] = (bits >> x & 1) || !is_finite(a[x]) ? a[x] : a[x] + (float)r.range(-0.05, 0.05);
            q.d[x] = (bits >> (3 + x) & 1) ? -0.0f : 0.0f;
        }
        q.d[axis] = (bits >> 8 & 1) ? 1.0f : -1.0f;
        q.o[axis] = a[axis] - q.d[axis] * (float)((bits >> 9 & 1) ? 2.0 : 0.0);
    } else if (kind == 12) {                                         // a hostile reach
        const float reach[8] = { 0.0f, -0.0f, NAN, -1.0f, INFINITY, 1e-30f, 0.5f, -INFINITY };
        q.m = reach[r.below(8)];
    } else if (kind == 13) {                                         // a non-finite or huge or subnormal component
        const float bad[8] = { NAN, INFINITY, -INFINITY, 3e38f, -3e38f, 1e-40f, -1e-40f, 0.0f };
        const uint32_t n = 1 + r.below(2);
        for (uint32_t i = 0; i < n; i++) (r.below(2) ? q.o : q.d)[r.below(3)] = bad[r.below(8)];
    } else if (kind == 14) {                                         // through the origin, where the parked triangles stand
        for (int x = 0; x < 3; x++) q.d[x] = -q.o[x];
    }
    return q;
}

struct Tally { int64_t rays = 0, hits = 0, nodes = 0, tris = 0, nodes_rebuilt = 0, tris_rebuilt = 0, bad = 0; };

void run_range(const Pair &p, const std::vector<float> &V, const std::vector<char> &park, const NearestBvh &b, const NearestBvh *rebuilt,
               uint64_t begin, uint64_t end, Tally *out)
{
    Tally t;
    for (uint64_t k = begin; k < end; k++) {
        const Ray q = make_ray(p, V, park, k);
        const Result want = brute(p, V, park, q.o, q.d, q.m, q.skip);
        const NearestRay r = nearest_ray(q.o, q.d, q.m, q.skip);
        uint32_t stack[kNearestStack];
        NearestStats st;
        const NearestBest got = nearest_traverse(b.nodes.data(), (int64_t)b.nodes.size(), b.tris.data(), r,
                                                 [&](int i) -> uint32_t & { return stack[i]; }, st);
        bool same = got.prim == want.prim && (want.prim == 0xFFFFFFFFu || !memcmp(&got.t, &want.t, 4));
        if (rebuilt) {
            NearestStats s2;
            const NearestBest g2 = nearest_traverse(rebuilt->nodes.data(), (int64_t)rebuilt->nodes.size(), rebuilt->tris.data(), r,
                                                    [&](int i) -> uint32_t & { return stack[i]; }, s2);
            same = same && g2.prim == got.prim && (got.prim == 0xFFFFFFFFu || (!memcmp(&g2.t, &got.t, 4) && !memcmp(&g2.u, &got.u, 4) && !memcmp(&g2.v, &got.v, 4)));
            t.nodes_rebuilt += s2.nodes; t.tris_rebuilt += s2.tris;
        }
        if (!same && t.bad++ < 5)
            printf("FAIL ray %llu: o %a %a %a d %a %a %a m %a skip %u: refit tree prim %u t %a, brute force prim %u t %a\n",
                   (unsigned long long)k, q.o[0], q.o[1], q.o[2], q.d[0], q.d[1], q.d[2], q.m, q.skip, got.prim, got.t, want.prim, want.t);
        t.rays++; t.hits += want.prim != 0xFFFFFFFFu; t.nodes += st.nodes; t.tris += st.tris;
    }
    *out = t;
}

template <class T>
bool read_all(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

bool read_pair(const char *path, Pair &p)
{
    int64_t head[2] = { 0, 0 };
    FILE *f = fopen(path, "rb");
    bool ok = f && fread(head, sizeof(int64_t), 2, f) == 2 && head[0] >= 0 && head[1] >= 0 && head[1] <= ((int64_t)1 << 22) &&
              head[0] <= ((int64_t)1 << 24);
    if (ok) {
        p.nv = head[0]; p.nt = head[1];
        p.A.resize(3 * (size_t)p.nv); p.B.resize(3 * (size_t)p.nv); p.T.resize(3 * (size_t)p.nt);
        ok = read_all(f, p.A) && read_all(f, p.B) && read_all(f, p.T);
        for (uint32_t i : p.T) ok = ok && (int64_t)i < p.nv;
        for (float x : p.A) ok = ok && is_finite(x);
    }
    if (f) fclose(f);
    return ok;
}

int run_pair(const char *path, int64_t rays, int leaf)
{
    Pair p;
    if (!read_pair(path, p)) { fprintf(stderr, "nearest_refit_host_check: %s is missing, short or malformed (A must be finite)\n", path); return 2; }
    if (leaf < 1 || leaf > 8 || rays < 0) { fprintf(stderr, "nearest_refit_host_check: leaf 1 .. 8, rays >= 0\n"); return 2; }
    NearestBvh built;
    nearest_build(p.A.data(), p.T.data(), p.nt, leaf, built);
    std::vector<uint32_t> list;
    std::vector<int64_t> offset;
    const bool tree = refit_levels(built.nodes.data(), (int64_t)built.nodes.size(), p.nt, list, offset);
    CHECK(tree && (int)offset.size() - 1 == built.depth && list.size() == built.nodes.size(), "the levels are not the built tree's: %zu levels, depth %d",
          offset.size() - 1, built.depth);
    if (!tree) return 1;
    // a level's nodes stand after every node they read
    {
        std::vector<int> done(built.nodes.size(), 0);
        for (uint32_t n : list) {
            const NearestNode &nd = built.nodes[n];
            if (!(nd.meta & kNearestCountMask)) CHECK(done[nd.first] && done[nd.first + 1], "node %u is listed before its children", n);
            done[n]++;
        }
        for (size_t n = 0; n < done.size(); n++) CHECK(done[n] == 1, "node %zu is listed %d times", n, done[n]);
        if (!list.empty()) CHECK(list.back() == 0u && offset.back() - offset[offset.size() - 2] == 1, "the root is not the last level");
    }
    std::vector<char> park((size_t)p.nt, 0);
    int64_t want_parked = 0;
    for (int64_t i = 0; i < p.nt; i++) want_parked += (park[(size_t)i] = parked(p, p.B, i));

    NearestBvh b = built;
    const int64_t got_parked = refit_host(b.nodes.data(), b.tris.data(), p.nt, p.T.data(), p.B.data(), list);
    CHECK(got_parked == want_parked, "%lld triangles parked, %lld hold a non-finite coordinate", (long long)got_parked, (long long)want_parked);
    CHECK(check_refit(p, p.B, built, b, "A -> B") == want_parked, "the records' parked triangles are not B's");

    NearestBvh rebuilt;
    const bool finite = want_parked == 0;
    if (finite) nearest_build(p.B.data(), p.T.data(), p.nt, leaf, rebuilt);

    unsigned threads = std::thread::hardware_concurrency();
    threads = threads < 1 ? 1 : threads > 8 ? 8 : threads;
    std::vector<Tally> t(threads);
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < threads; w++)
        pool.emplace_back(run_range, std::cref(p), std::cref(p.B), std::cref(park), std::cref(b), finite ? &rebuilt : nullptr,
                          (uint64_t)(rays * w / threads), (uint64_t)(rays * (w + 1) / threads), &t[w]);
    for (auto &th : pool) th.join();
    Tally sum;
    for (const Tally &x : t) {
        sum.rays += x.rays; sum.hits += x.hits; sum.nodes += x.nodes; sum.tris += x.tris; sum.bad += x.bad;
        sum.nodes_rebuilt += x.nodes_rebuilt; sum.tris_rebuilt += x.tris_rebuilt;
    }
    fails += (int)(sum.bad > 1000 ? 1000 : sum.bad);

    // and back: every box and record by value
    const int64_t none = refit_host(b.nodes.data(), b.tris.data(), p.nt, p.T.data(), p.A.data(), list);
    CHECK(none == 0, "%lld triangles parked on the way back to a finite mesh", (long long)none);
    check_refit(p, p.A, built, b, "B -> A");
    for (size_t n = 0; n < b.nodes.size(); n++)
        for (int c = 0; c < 3; c++)
            CHECK(b.nodes[n].lo[c] == built.nodes[n].lo[c] && b.nodes[n].hi[c] == built.nodes[n].hi[c], "B -> A: node %zu axis %d is not the builder's box", n, c);
    CHECK(b.tris.empty() || !memcmp(b.tris.data(), built.tris.data(), b.tris.size() * sizeof(NearestTri)), "B -> A: the records are not the builder's");

    if (fails) return 1;
    const double n = sum.rays ? (double)sum.rays : 1.0;
    printf("ok pair: nt %lld leaf %d depth %d nodes %lld parked %lld rays %lld hits %lld differ %lld refit %.2f nodes %.2f triangles a ray rebuilt %.2f nodes %.2f triangles a ray\n",
           (long long)p.nt, leaf, built.depth, (long long)built.nodes.size(), (long long)got_parked, (long long)sum.rays, (long long)sum.hits,
           (long long)sum.bad, (double)sum.nodes / n, (double)sum.tris / n, (double)sum.nodes_rebuilt / n, (double)sum.tris_rebuilt / n);
    return 0;
}

// the tree the product's builder makes on A -- the tree a scene on A holds -- for the tests that need its links without a device
int write_tree(const char *path, int leaf, const char *out)
{
    Pair p;
    if (!read_pair(path, p)) { fprintf(stderr, "nearest_refit_host_check: %s is missing, short or malformed (A must be finite)\n", path); return 2; }
    if (leaf < 1 || leaf > 8) { fprintf(stderr, "nearest_refit_host_check: leaf 1 .. 8\n"); return 2; }
    NearestBvh built;
    nearest_build(p.A.data(), p.T.data(), p.nt, leaf, built);
    const int64_t head[2] = { (int64_t)built.nodes.size(), (int64_t)built.tris.size() };
    std::vector<uint32_t> links, prims;
    std::vector<float> boxes;
    for (const NearestNode &n : built.nodes) {
        links.push_back(n.first); links.push_back(n.meta);
        for (int c = 0; c < 3; c++) boxes.push_back(n.lo[c]);
        for (int c = 0; c < 3; c++) boxes.push_back(n.hi[c]);
    }
    for (const NearestTri &t : built.tris) prims.push_back(t.prim);
    FILE *f = fopen(out, "wb");
    bool ok = f && fwrite(head, sizeof(int64_t), 2, f) == 2;
    ok = ok && fwrite(links.data(), sizeof(uint32_t), links.size(), f) == links.size();
    ok = ok && fwrite(prims.data(), sizeof(uint32_t), prims.size(), f) == prims.size();
    ok = ok && fwrite(boxes.data(), sizeof(float), boxes.size(), f) == boxes.size();
    if (f) ok = fclose(f) == 0 && ok;
    if (!ok) { fprintf(stderr, "nearest_refit_host_check: cannot write %s\n", out); return 2; }
    printf("ok tree: nt %lld leaf %d depth %d nodes %lld\n", (long long)p.nt, leaf, built.depth, (long long)built.nodes.size());
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "tree")) return write_tree(argv[2], atoi(argv[3]), argv[4]);
    if (argc == 4) return run_pair(argv[1], atoll(argv[2]), atoi(argv[3]));
    fprintf(stderr, "usage: nearest_refit_host_check <pair.bin> <rays> <leaf>\n       nearest_refit_host_check tree <pair.bin> <leaf> <out.bin>\n");
    return 2;
}
