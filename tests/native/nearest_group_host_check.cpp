// nearest_group_host_check.cpp -- the two-level traversal of librls_nearest_group.so on the CPU: the product's builder
// (rls_nearest_bvh.hpp) and the group's own source (rls_nearest_group.hpp, over rls_nearest_device.hpp and rls_nearest_refit.hpp)
// compiled for the host with -ffp-contract=off, no HIP.
//
//   nearest_group_host_check <group.bin> <rays.bin> <out.bin> <top leaf> <scene leaf>
//
// group.bin: int64 meshes, instances; a mesh: int64 nv, nt; float V[nv * 3]; uint32 T[nt * 3]; an instance: uint32 mesh, float
// A[12], float B[12].  rays.bin: int64 rays; 9 words a ray: o.xyz, d.xyz, maxdist (float32), skip_instance, skip_prim (uint32).
// (tests/nearest_group_host_util.py writes both.)  Every mesh's tree is built with <scene leaf>, every instance's record by
// group_record from its tree's root box, the top tree by group_build with <top leaf> -- what rls_nearest_group_create does.  Then
//   - the top tree's depth is within its bound and within the top stack, its leaves hold every instance once, its levels are read
//     from its links, and the update's union (group_node over the levels, deepest first) leaves every box what it was, by value;
//   - a second group_build over the same boxes gives the same tree (the builder is deterministic);
//   - for every ray the traversal (group_traverse, both stacks in one array of 16 + 24 words) equals the brute force
//     (group_brute: every instance that takes part, every triangle) bit for bit in (instance, prim, t).
// The rays are shared out over min(hardware threads, 16) threads where the brute force is large (a ray's result depends on
// nothing but the ray).  out.bin: 10 words a ray: the brute force's instance, prim, t; the traversal's instance, prim, t; top
// nodes visited, instances entered, the most top-stack entries held, the most object-stack entries held.  Prints "levels: ..." (the top tree's node count
// level by level, the root's first: what rls_nearest_group_update's launch plan is made from) and one "ok group: ..." line and
// exits 0, or the first differences and exits 1.  tests/test_nearest_group_host.py drives it, once more under -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../rlshaders_amd/csrc_nearest/rls_nearest_group.hpp"

namespace {

std::atomic<int> fails(0);
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Mesh {
    std::vector<float> V;
    std::vector<uint32_t> T;
    NearestBvh bvh;
};

uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

template <class T> bool read_n(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

} // namespace

int main(int argc, char **argv)
{
    if (argc != 6) { fprintf(stderr, "usage: %s group.bin rays.bin out.bin top_leaf scene_leaf\n", argv[0]); return 2; }
    const int top_leaf = atoi(argv[4]), scene_leaf = atoi(argv[5]);
    if (top_leaf < 1 || top_leaf > 4 || scene_leaf < 1 || scene_leaf > 8) { fprintf(stderr, "leaf sizes out of range\n"); return 2; }

    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int64_t head[2];
    bool ok = fread(head, 8, 2, f) == 2 && head[0] >= 0 && head[1] >= 0 && head[1] <= ((int64_t)1 << 16);
    std::vector<Mesh> meshes(ok ? (size_t)head[0] : 0);
    for (Mesh &m : meshes) {
        int64_t h[2];
        ok = ok && fread(h, 8, 2, f) == 2 && h[0] >= 0 && h[1] >= 0 && read_n(f, m.V, 3 * (size_t)h[0]) && read_n(f, m.T, 3 * (size_t)h[1]);
        if (!ok) break;
        for (uint32_t i : m.T) ok = ok && (int64_t)i < h[0];
        if (ok) nearest_build(m.V.data(), m.T.data(), h[1], scene_leaf, m.bvh);
    }
    const int64_t count = ok ? head[1] : 0;
    std::vector<GroupPlacement> place((size_t)count);
    int64_t placed_tris = 0;                                             // the triangles a ray meets in the brute force, at most
    for (int64_t j = 0; ok && j < count; j++) {
        uint32_t w[25];
        ok = fread(w, 4, 25, f) == 25 && w[0] < meshes.size();
        if (!ok) break;
        GroupPlacement &p = place[(size_t)j];
        p = GroupPlacement();
        memcpy(p.A, w + 1, 48);
        memcpy(p.B, w + 13, 48);
        const Mesh &m = meshes[w[0]];
        p.nodes = m.bvh.nodes.data(); p.tris = m.bvh.tris.data(); p.index = m.T.data();
        p.node_count = (uint32_t)m.bvh.nodes.size();
        placed_tris += (int64_t)(m.T.size() / 3);
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "bad group file\n"); return 2; }

    // the records by instance, the world boxes, the top tree
    std::vector<GroupInstance> by_instance((size_t)count), recs((size_t)count);
    std::vector<float> world(6 * (size_t)count);
    int64_t parked = 0;
    for (int64_t j = 0; j < count; j++) {
        const GroupPlacement &p = place[(size_t)j];
        float lo[3] = { 0, 0, 0 }, hi[3] = { 0, 0, 0 };
        if (p.node_count)
            for (int c = 0; c < 3; c++) { lo[c] = p.nodes[0].lo[c]; hi[c] = p.nodes[0].hi[c]; }
        parked += group_record(p, lo, hi, (uint32_t)j, by_instance[(size_t)j]) ? 1 : 0;
        for (int c = 0; c < 3; c++) { world[6 * j + c] = by_instance[(size_t)j].lo[c]; world[6 * j + 3 + c] = by_instance[(size_t)j].hi[c]; }
    }
    NearestBvh top, again;
    std::vector<uint32_t> order, order2, list;
    std::vector<int64_t> offset;
    group_build(world.data(), count, top_leaf, top, order);
    group_build(world.data(), count, top_leaf, again, order2);
    CHECK(order == order2 && top.nodes.size() == again.nodes.size() &&
              (top.nodes.empty() || memcmp(top.nodes.data(), again.nodes.data(), top.nodes.size() * sizeof(NearestNode)) == 0),
          "the top builder is not deterministic");
    CHECK(top.depth <= nearest_depth_bound(count, top_leaf) && top.depth - 1 <= kGroupStack, "top depth %d past its bound", top.depth);
    std::vector<char> seen((size_t)count, 0);
    for (size_t k = 0; k < (size_t)count; k++) {
        CHECK(order[k] < (uint32_t)count && !seen[order[k]], "slot %zu: instance %u twice or out of range", k, order[k]);
        if (order[k] < (uint32_t)count) seen[order[k]] = 1;
        recs[k] = by_instance[order[k]];
    }
    CHECK(refit_levels(top.nodes.data(), (int64_t)top.nodes.size(), count, list, offset), "the top tree's links are not a tree");
    CHECK((int64_t)offset.size() - 1 == top.depth, "levels %zu, depth %d", offset.size() - 1, top.depth);
    {   // the update's union restated on the host: boxes scrambled, then every node from what is below it
        std::vector<NearestNode> moved = top.nodes;
        for (NearestNode &n : moved)
            for (int c = 0; c < 3; c++) { n.lo[c] = 1e30f; n.hi[c] = -1e30f; }
        for (uint32_t n : list) group_node(moved.data(), recs.data(), n);
        for (size_t n = 0; n < moved.size(); n++) {
            CHECK(moved[n].first == top.nodes[n].first && moved[n].meta == top.nodes[n].meta, "node %zu: links changed", n);
            for (int c = 0; c < 3; c++)
                CHECK(moved[n].lo[c] == top.nodes[n].lo[c] && moved[n].hi[c] == top.nodes[n].hi[c], "node %zu: the union is not the builder's box", n);
        }
    }

    f = fopen(argv[2], "rb");
    int64_t M = 0;
    std::vector<uint32_t> rays;
    ok = f && fread(&M, 8, 1, f) == 1 && M >= 0 && read_n(f, rays, 9 * (size_t)M);
    if (f) fclose(f);
    if (!ok) { fprintf(stderr, "bad rays file\n"); return 2; }
    std::vector<uint32_t> out(10 * (size_t)M);
    struct Tally { int64_t hits = 0, differ = 0; int max_top = 0, max_stack = 0; };
    auto work = [&](int64_t k0, int64_t k1, Tally *tally) {
        int64_t hits = 0, differ = 0;
        int max_top = 0, max_stack = 0;
        for (int64_t k = k0; k < k1; k++) {
            float w[7];
            memcpy(w, &rays[9 * (size_t)k], 28);
            const float o[3] = { w[0], w[1], w[2] }, d[3] = { w[3], w[4], w[5] };
            GroupRay g;
            g.w = nearest_ray(o, d, w[6], rays[9 * (size_t)k + 8]);
            g.skip_instance = rays[9 * (size_t)k + 7];
            const GroupBest want = group_brute(by_instance.data(), count, g);
            uint32_t stack[kGroupStack + kNearestStack];
            GroupStats st;
            const GroupBest got = group_traverse(top.nodes.data(), (int64_t)top.nodes.size(), recs.data(), g,
                                                 [&](int i) -> uint32_t & { return stack[i]; }, st);
            const bool hit = want.instance != kGroupNoInstance;
            hits += hit;
            const bool same = want.instance == got.instance && (!hit || (want.prim == got.prim && bits(want.t) == bits(got.t) &&
                                                                          bits(want.u) == bits(got.u) && bits(want.v) == bits(got.v)));
            if (!same) {
                differ++;
                CHECK(false, "ray %lld: brute (%u, %u, %a) traversal (%u, %u, %a)", (long long)k, want.instance, want.prim, want.t, got.instance, got.prim, got.t);
            }
            CHECK(st.max_top <= kGroupStack && st.max_top <= (top.depth > 0 ? top.depth - 1 : 0), "ray %lld: %d top entries", (long long)k, st.max_top);
            CHECK(st.max_stack <= kNearestStack, "ray %lld: %d object entries", (long long)k, st.max_stack);
            if (st.max_top > max_top) max_top = st.max_top;
            if (st.max_stack > max_stack) max_stack = st.max_stack;
            uint32_t *r = &out[10 * (size_t)k];
            r[0] = want.instance; r[1] = hit ? want.prim : kNearestNoPrim; r[2] = bits(hit ? want.t : 0.0f);
            r[3] = got.instance; r[4] = got.instance != kGroupNoInstance ? got.prim : kNearestNoPrim; r[5] = bits(got.instance != kGroupNoInstance ? got.t : 0.0f);
            r[6] = (uint32_t)st.top_nodes; r[7] = (uint32_t)st.instances; r[8] = (uint32_t)st.max_top; r[9] = (uint32_t)st.max_stack;
        }
        tally->hits = hits; tally->differ = differ; tally->max_top = max_top; tally->max_stack = max_stack;
    };
    int threads = (int)std::thread::hardware_concurrency();
    threads = threads < 1 ? 1 : threads > 16 ? 16 : threads;
    if (M * (placed_tris + count + 1) < 4000000) threads = 1;
    std::vector<Tally> tallies((size_t)threads);
    if (threads == 1) {
        work(0, M, &tallies[0]);
    } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; t++) pool.emplace_back(work, M * t / threads, M * (t + 1) / threads, &tallies[(size_t)t]);
        for (std::thread &t : pool) t.join();
    }
    int64_t hits = 0, differ = 0;
    int max_top = 0, max_stack = 0;
    for (const Tally &t : tallies) {
        hits += t.hits; differ += t.differ;
        if (t.max_top > max_top) max_top = t.max_top;
        if (t.max_stack > max_stack) max_stack = t.max_stack;
    }
    f = fopen(argv[3], "wb");
    ok = f && (out.empty() || fwrite(out.data(), 4, out.size(), f) == out.size());
    if (f) fclose(f);
    if (!ok) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    if (fails) { printf("%d checks failed\n", (int)fails); return 1; }
    printf("levels:");                                                   // the root's level first: what the update's plan is made from
    for (size_t l = offset.size() - 1; l >= 1; l--) printf(" %lld", (long long)(offset[l] - offset[l - 1]));
    printf("\n");
    printf("ok group: instances %lld parked %lld top_leaf %d scene_leaf %d depth %d top_nodes %zu rays %lld hits %lld differ %lld max_top %d max_stack %d\n",
           (long long)count, (long long)parked, top_leaf, scene_leaf, top.depth, top.nodes.size(), (long long)M, (long long)hits,
           (long long)differ, max_top, max_stack);
    return 0;
}
