// nearest_stats.cpp -- the nodes and triangles a ray visits and the most stack entries it holds, counted on the CPU by the traversal source the kernel compiles
// (rls_nearest_device.hpp through NearestStats) over the tree the library builds (rls_nearest_bvh.hpp).  A stand-alone host
// program, no HIP (rlshaders_amd/build.py, build_nearest_stats; -ffp-contract=off): rlshaders_amd.nearest.host_stats writes its
// input and reads its output; tools/trace_bench.py --closure nearest runs it on a sample of the rays it times.
//
// usage: nearest_stats <file> [--per-ray]
// file: int64 nv, nt, leaf_size, rays; float V[nv * 3]; uint32 T[nt * 3]; per ray 8 words: o.xyz, d.xyz, maxdist (float), skip
// (uint32).  Prints one JSON line: rays, hits, nodes and triangles visited in all, max_stack (the most stack entries any ray
// held), the tree's nodes and depth; with --per-ray also "per_ray": [[hit, prim, nodes, triangles, max_stack], ...].
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rls_nearest_device.hpp"

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: nearest_stats <file> [--per-ray]\n"); return 2; }
    const bool per_ray = argc > 2 && !strcmp(argv[2], "--per-ray");
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "nearest_stats: cannot open %s\n", argv[1]); return 2; }
    int64_t head[4] = { 0, 0, 0, 0 };
    bool ok = fread(head, sizeof(int64_t), 4, f) == 4 && head[0] >= 0 && head[1] >= 0 && head[2] >= 1 && head[2] <= 8 && head[3] >= 0;
    const int64_t nv = head[0], nt = head[1], rays = head[3];
    std::vector<float> V;
    std::vector<uint32_t> T, R;
    if (ok) {
        V.resize((size_t)nv * 3); T.resize((size_t)nt * 3); R.resize((size_t)rays * 8);
        ok = fread(V.data(), 4, V.size(), f) == V.size() && fread(T.data(), 4, T.size(), f) == T.size() &&
             fread(R.data(), 4, R.size(), f) == R.size();
        for (uint32_t i : T) ok = ok && (int64_t)i < nv;
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "nearest_stats: %s is short or malformed\n", argv[1]); return 2; }
    NearestBvh b;
    nearest_build(V.data(), T.data(), nt, (int)head[2], b);
    NearestStats all;
    int64_t hits = 0;
    printf("{\"rays\": %lld, \"tree_nodes\": %lld, \"depth\": %d, ", (long long)rays, (long long)b.nodes.size(), b.depth);
    if (per_ray) printf("\"per_ray\": [");
    for (int64_t k = 0; k < rays; k++) {
        float w[7];
        memcpy(w, &R[(size_t)k * 8], sizeof w);
        const float o[3] = { w[0], w[1], w[2] }, d[3] = { w[3], w[4], w[5] };
        const NearestRay r = nearest_ray(o, d, w[6], R[(size_t)k * 8 + 7]);
        uint32_t stack[kNearestStack];
        NearestStats st;
        const NearestBest best = nearest_traverse(b.nodes.data(), (int64_t)b.nodes.size(), b.tris.data(), r,
                                                  [&](int i) -> uint32_t & { return stack[i]; }, st);
        const bool hit = best.prim != kNearestNoPrim;
        hits += hit;
        all.nodes += st.nodes; all.tris += st.tris;
        nearest_count_push(all, st.max_stack);
        if (per_ray)
            printf("%s[%d, %u, %lld, %lld, %d]", k ? ", " : "", hit ? 1 : 0, hit ? best.prim : 0u, (long long)st.nodes, (long long)st.tris,
                   st.max_stack);
    }
    if (per_ray) printf("], ");
    printf("\"hits\": %lld, \"nodes\": %lld, \"triangles\": %lld, \"max_stack\": %d}\n", (long long)hits, (long long)all.nodes,
           (long long)all.tris, all.max_stack);
    return 0;
}
