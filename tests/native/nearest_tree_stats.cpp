// nearest_tree_stats.cpp -- the nodes and triangles rays visit on a GIVEN tree: what rls_nearest_refit_read_tree or
// rls_nearest_rebuild_read_tree returned for a scene (boxes, links, the triangle ids in leaf order), the records made again from
// the mesh as the refit makes them (rls_nearest_refit.hpp, refit_record: a triangle with a non-finite coordinate stands at the
// origin), traversed by the source the kernel compiles (rls_nearest_device.hpp through NearestStats).  The product's
// nearest_stats counts on the tree the builder makes; this one counts on the tree a device holds, whoever made it.  A stand-alone
// host program, no HIP; -ffp-contract=off.
//
// usage: nearest_tree_stats <file>
// file: int64 nv, nt, nodes, rays; float V[nv * 3]; uint32 T[nt * 3]; uint32 links[nodes * 2]; uint32 prims[nt];
// float boxes[nodes * 6]; per ray 8 words: o.xyz, d.xyz, maxdist (float), skip (uint32).  Prints one JSON line: rays, hits, the
// nodes and triangles visited in all, max_stack, and an FNV-1a checksum over every ray's (hit, prim, t).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../rlshaders_amd/csrc_nearest/rls_nearest_device.hpp"
#include "../../rlshaders_amd/csrc_nearest/rls_nearest_refit.hpp"

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: nearest_tree_stats <file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "nearest_tree_stats: cannot open %s\n", argv[1]); return 2; }
    int64_t head[4] = { 0, 0, 0, 0 };
    bool ok = fread(head, sizeof(int64_t), 4, f) == 4 && head[0] >= 0 && head[1] >= 0 && head[2] >= 0 && head[3] >= 0;
    const int64_t nv = head[0], nt = head[1], nodes = head[2], rays = head[3];
    std::vector<float> V, boxes;
    std::vector<uint32_t> T, links, prims, R;
    if (ok) {
        V.resize((size_t)nv * 3); T.resize((size_t)nt * 3); links.resize((size_t)nodes * 2); prims.resize((size_t)nt);
        boxes.resize((size_t)nodes * 6); R.resize((size_t)rays * 8);
        ok = fread(V.data(), 4, V.size(), f) == V.size() && fread(T.data(), 4, T.size(), f) == T.size() &&
             fread(links.data(), 4, links.size(), f) == links.size() && fread(prims.data(), 4, prims.size(), f) == prims.size() &&
             fread(boxes.data(), 4, boxes.size(), f) == boxes.size() && fread(R.data(), 4, R.size(), f) == R.size();
        for (uint32_t i : T) ok = ok && (int64_t)i < nv;
        for (uint32_t p : prims) ok = ok && (int64_t)p < nt;
    }
    fclose(f);
    std::vector<NearestNode> tree((size_t)nodes);
    std::vector<NearestTri> tris((size_t)nt);
    for (size_t n = 0; ok && n < tree.size(); n++) {
        for (int c = 0; c < 3; c++) { tree[n].lo[c] = boxes[6 * n + c]; tree[n].hi[c] = boxes[6 * n + 3 + c]; }
        tree[n].first = links[2 * n]; tree[n].meta = links[2 * n + 1];
    }
    std::vector<uint32_t> list;
    std::vector<int64_t> offset;
    ok = ok && refit_levels(tree.data(), nodes, nt, list, offset) && (int64_t)offset.size() - 1 <= kNearestStack + 1;
    if (!ok) { fprintf(stderr, "nearest_tree_stats: %s is short, malformed or holds no tree\n", argv[1]); return 2; }
    for (size_t k = 0; k < tris.size(); k++) {
        const uint32_t p = prims[k];
        (void)refit_record(V.data(), T[3 * (size_t)p], T[3 * (size_t)p + 1], T[3 * (size_t)p + 2], p, tris[k]);
    }
    NearestStats all;
    int64_t hits = 0;
    uint64_t sum = 1469598103934665603ull;
    for (int64_t k = 0; k < rays; k++) {
        float w[7];
        memcpy(w, &R[(size_t)k * 8], sizeof w);
        const float o[3] = { w[0], w[1], w[2] }, d[3] = { w[3], w[4], w[5] };
        const NearestRay r = nearest_ray(o, d, w[6], R[(size_t)k * 8 + 7]);
        uint32_t stack[kNearestStack];
        NearestStats st;
        const NearestBest best = nearest_traverse(tree.data(), nodes, tris.data(), r, [&](int i) -> uint32_t & { return stack[i]; }, st);
        const bool hit = best.prim != kNearestNoPrim;
        hits += hit;
        all.nodes += st.nodes; all.tris += st.tris;
        nearest_count_push(all, st.max_stack);
        uint32_t word[2] = { hit ? best.prim : kNearestNoPrim, 0u };
        if (hit) memcpy(&word[1], &best.t, 4);
        const uint8_t *b = (const uint8_t *)word;
        for (int i = 0; i < 8; i++) { sum ^= b[i]; sum *= 1099511628211ull; }
    }
    printf("{\"rays\": %lld, \"hits\": %lld, \"nodes\": %lld, \"triangles\": %lld, \"max_stack\": %d, \"results\": \"%016llx\"}\n",
           (long long)rays, (long long)hits, (long long)all.nodes, (long long)all.tris, all.max_stack, (unsigned long long)sum);
    return 0;
}
