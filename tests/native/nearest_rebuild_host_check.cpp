// nearest_rebuild_host_check.cpp -- the rebuild of librls_nearest_rebuild.so on the CPU: the product's builder
// (rls_nearest_bvh.hpp) and the rebuild's own source (rls_nearest_rebuild.hpp, over rls_nearest_refit.hpp) compiled for the host
// with -ffp-contract=off, no HIP.
//
//   nearest_rebuild_host_check <pair.bin> <leaf> [<out.bin>]
//
// pair.bin: int64 nv, nt; float A[nv * 3]; float B[nv * 3]; uint32 T[nt * 3] (tests/nearest_refit_util.py writes it).  A is
// finite; B may hold NaN and infinities.  The tree is built on A -- the tree a scene on A holds --, its shape and levels are
// read from its links as rls_nearest_rebuild_create reads them, and rebuild_host moves it to B.  Then
//   - the REFERENCE is nearest_build on B with every parked triangle (a non-finite coordinate, judged by this program) taken
//     as three vertices at the origin: a mesh of 3 nt vertices of its own, so that a vertex shared with a finite triangle
//     keeps its place there;
//   - every node's first and meta (the axis bits included) and the order of the triangle ids equal the reference's exactly,
//     every box equals it by value, every record holds the reference's vertices bit for bit, and the parked count is this
//     program's;
//   - the sizes and the depth did not change;
//   - the rebuild's order key is the builder's on every coordinate sum met, and its inverse gives the bits back;
//   - a rebuild back to A gives the tree built on A.
// With <out.bin> the rebuilt tree is written as nearest_refit_host_check's tree mode writes one.  Prints one "ok rebuild: ..."
// line and exits 0, or the first differences and exits 1.  tests/test_nearest_rebuild_host.py drives it, once more under
// -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../rlshaders_amd/csrc_nearest/rls_nearest_rebuild.hpp"

namespace {

int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

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

bool read_pair(const char *path, Pair &p)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    int64_t head[2];
    bool ok = fread(head, 8, 2, f) == 2 && head[0] >= 0 && head[1] >= 0;
    if (ok) {
        p.nv = head[0]; p.nt = head[1];
        p.A.resize(3 * (size_t)p.nv); p.B.resize(3 * (size_t)p.nv); p.T.resize(3 * (size_t)p.nt);
        ok = fread(p.A.data(), 4, p.A.size(), f) == p.A.size() && fread(p.B.data(), 4, p.B.size(), f) == p.B.size() &&
             fread(p.T.data(), 4, p.T.size(), f) == p.T.size();
    }
    fclose(f);
    for (uint32_t i : p.T) ok = ok && (int64_t)i < p.nv;
    return ok;
}

// the reference: the builder on the mesh whose parked triangles stand at the origin -> its parked count
int64_t reference(const Pair &p, const std::vector<float> &V, int leaf, NearestBvh &out)
{
    std::vector<float> own(9 * (size_t)p.nt, 0.0f);
    std::vector<uint32_t> tri(3 * (size_t)p.nt);
    int64_t park = 0;
    for (int64_t i = 0; i < p.nt; i++) {
        const bool pk = parked(p, V, i);
        park += pk;
        for (int v = 0; v < 3; v++) {
            tri[3 * (size_t)i + v] = (uint32_t)(3 * i + v);
            for (int c = 0; c < 3; c++)
                if (!pk) own[9 * (size_t)i + 3 * v + c] = V[3 * (size_t)p.T[3 * i + v] + c];
        }
    }
    nearest_build(own.data(), tri.data(), p.nt, leaf, out);
    return park;
}

// the keys: the rebuild's is the builder's, and the inverse gives the bits back
void check_keys(const std::vector<float> &V)
{
    for (size_t k = 0; k + 1 < V.size(); k++) {
        const float probe[4] = { V[k], V[k] + V[k + 1], -V[k], V[k] + V[k] };
        for (float f : probe) {
            if (f != f) continue;
            const uint32_t key = rebuild_order_key(f);
            const float back = rebuild_key_value(key);
            CHECK(key == nearest_order_key(f), "the order key of %a is %08x, the builder's %08x", f, key, nearest_order_key(f));
            CHECK(!memcmp(&back, &f, 4), "the value of key %08x is %a, not %a", key, back, f);
        }
    }
    const float zeros[2] = { 0.0f, -0.0f };
    CHECK(rebuild_order_key(zeros[1]) < rebuild_order_key(zeros[0]), "-0 orders below +0");
}

void compare(const NearestBvh &got, const NearestBvh &want, const char *what)
{
    CHECK(got.nodes.size() == want.nodes.size() && got.tris.size() == want.tris.size(), "%s: %zu nodes and %zu records, the builder has %zu and %zu",
          what, got.nodes.size(), got.tris.size(), want.nodes.size(), want.tris.size());
    if (got.nodes.size() != want.nodes.size() || got.tris.size() != want.tris.size()) return;
    for (size_t n = 0; n < got.nodes.size(); n++) {
        const NearestNode &g = got.nodes[n], &w = want.nodes[n];
        CHECK(g.first == w.first && g.meta == w.meta, "%s: node %zu links (%u, %08x), the builder's (%u, %08x)", what, n, g.first, g.meta, w.first, w.meta);
        for (int c = 0; c < 3; c++)
            CHECK(g.lo[c] == w.lo[c] && g.hi[c] == w.hi[c], "%s: node %zu axis %d holds [%a, %a], the builder's [%a, %a]", what, n, c, g.lo[c], g.hi[c],
                  w.lo[c], w.hi[c]);
    }
    for (size_t k = 0; k < got.tris.size(); k++) {
        const NearestTri &g = got.tris[k], &w = want.tris[k];
        CHECK(g.prim == w.prim, "%s: record %zu holds triangle %u, the builder's %u", what, k, g.prim, w.prim);
        CHECK(!memcmp(g.v0, w.v0, 12) && !memcmp(g.v1, w.v1, 12) && !memcmp(g.v2, w.v2, 12), "%s: record %zu's vertices differ", what, k);
    }
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: nearest_rebuild_host_check <pair.bin> <leaf> [<out.bin>]\n"); return 2; }
    Pair p;
    const int leaf = atoi(argv[2]);
    if (!read_pair(argv[1], p) || leaf < 1 || leaf > kRebuildMaxLeaf) { fprintf(stderr, "bad arguments\n"); return 2; }
    for (float f : p.A)
        if (!is_finite(f)) { fprintf(stderr, "A is not finite\n"); return 2; }

    NearestBvh built, tree;
    nearest_build(p.A.data(), p.T.data(), p.nt, leaf, built);
    tree = built;
    std::vector<RebuildRange> range;
    std::vector<uint32_t> list;
    std::vector<int64_t> offset;
    const int64_t nodes = (int64_t)tree.nodes.size();
    const bool levels_ok = refit_levels(tree.nodes.data(), nodes, p.nt, list, offset);
    const bool shape_ok = rebuild_shape(tree.nodes.data(), nodes, p.nt, leaf, range);
    CHECK(levels_ok && shape_ok, "the built tree is refused: levels %d shape %d", (int)levels_ok, (int)shape_ok);
    const int levels = (int)offset.size() - 1;
    CHECK(levels == built.depth, "%d levels, the builder's depth %d", levels, built.depth);
    if (fails) return 1;
    // a tree of another shape is refused: a leaf one record short, an inner node's children swapped
    if (nodes > 1) {
        std::vector<NearestNode> bad(tree.nodes);
        std::vector<RebuildRange> r2;
        std::swap(bad[bad[0].first], bad[bad[0].first + 1]);
        if (p.nt % 2) CHECK(!rebuild_shape(bad.data(), nodes, p.nt, leaf, r2), "a tree with the root's children swapped is accepted");
        bad = tree.nodes;
        for (NearestNode &n : bad)
            if (n.meta & kNearestCountMask) { n.first += 1; break; }
        CHECK(!rebuild_shape(bad.data(), nodes, p.nt, leaf, r2), "a tree with a moved leaf is accepted");
    }

    const int64_t park = rebuild_host(tree.nodes.data(), tree.tris.data(), p.nt, leaf, p.T.data(), p.B.data(), range, list, levels);
    NearestBvh want;
    const int64_t want_park = reference(p, p.B, leaf, want);
    CHECK(park == want_park, "%lld triangles parked, %lld are", (long long)park, (long long)want_park);
    CHECK(want.depth == built.depth, "the reference's depth %d, the scene's %d", want.depth, built.depth);
    compare(tree, want, "rebuilt to B");
    check_keys(p.B);
    check_keys(p.A);
    int axes[3] = { 0, 0, 0 };
    for (const NearestNode &n : tree.nodes)
        if (!(n.meta & kNearestCountMask)) axes[(n.meta >> kNearestAxisShift) & 3u]++;

    if (argc == 4) {
        FILE *f = fopen(argv[3], "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
        const int64_t head[2] = { nodes, p.nt };
        fwrite(head, 8, 2, f);
        for (const NearestNode &n : tree.nodes) { fwrite(&n.first, 4, 1, f); fwrite(&n.meta, 4, 1, f); }
        for (const NearestTri &t : tree.tris) fwrite(&t.prim, 4, 1, f);
        for (const NearestNode &n : tree.nodes) { fwrite(n.lo, 4, 3, f); fwrite(n.hi, 4, 3, f); }
        fclose(f);
    }

    // and back: the tree built on A
    const int64_t back = rebuild_host(tree.nodes.data(), tree.tris.data(), p.nt, leaf, p.T.data(), p.A.data(), range, list, levels);
    CHECK(back == 0, "%lld triangles of A parked", (long long)back);
    compare(tree, built, "rebuilt back to A");

    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("ok rebuild: nt %lld leaf %d depth %d nodes %lld parked %lld axes %d %d %d\n", (long long)p.nt, leaf, built.depth, (long long)nodes,
           (long long)park, axes[0], axes[1], axes[2]);
    return 0;
}
