// nearest_any_host_check.cpp -- the any-hit traversal of librls_nearest_any.so on the CPU: the product's builder
// (rls_nearest_bvh.hpp) and the library's own source (rls_nearest_any.hpp over rls_nearest_device.hpp) compiled for the host with
// -ffp-contract=off, no HIP.
//
//   nearest_any_host_check <mesh.bin> <rays.bin> <out.bin> <leaf>
//
// mesh.bin: int64 nv, nt, surfaces (0 / 1), flags (0: no table); float V[nv * 3]; uint32 T[nt * 3]; uint32 surface[nt] where
// surfaces; uint8 flag[flags].  rays.bin: int64 rays; 8 words a ray: o.xyz, d.xyz, maxdist (float32), skip (uint32).
// (tests/nearest_any_host_util.py writes both.)  The tree is built with <leaf>, its depth held to its bound and to the stack.
// For every ray any_traverse equals any_brute (the statement: every triangle, no tree, no early end) in state, and the stack
// entries it held stay within depth - 1; nearest_traverse runs on the same ray for the record.
// out.bin: 7 words a ray: the brute force's state, the traversal's state, nodes and triangles any_traverse visited, nodes and
// triangles nearest_traverse visited, the most stack entries any_traverse held.  Prints one "ok any: ..." line and exits 0, or
// the first differences and exits 1.  tests/test_nearest_any_host.py drives it, once more under -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <thread>
#include <vector>

#include "../../rlshaders_amd/csrc_nearest/rls_nearest_any.hpp"

namespace {

template <class T> bool read_n(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

} // namespace

int main(int argc, char **argv)
{
    if (argc != 5) { fprintf(stderr, "usage: %s mesh.bin rays.bin out.bin leaf\n", argv[0]); return 2; }
    const int leaf = atoi(argv[4]);
    if (leaf < 1 || leaf > 8) { fprintf(stderr, "leaf out of range\n"); return 2; }

    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int64_t head[4];
    std::vector<float> V;
    std::vector<uint32_t> T, surface;
    std::vector<uint8_t> flags;
    bool ok = fread(head, 8, 4, f) == 4 && head[0] >= 0 && head[1] >= 0 && head[3] >= 0;
    ok = ok && read_n(f, V, 3 * (size_t)head[0]) && read_n(f, T, 3 * (size_t)head[1]);
    ok = ok && read_n(f, surface, head[2] ? (size_t)head[1] : 0) && read_n(f, flags, (size_t)head[3]);
    fclose(f);
    for (uint32_t i : T) ok = ok && (int64_t)i < head[0];
    if (!ok) { fprintf(stderr, "bad mesh file\n"); return 2; }
    const int64_t nt = head[1];

    f = fopen(argv[2], "rb");
    int64_t M = 0;
    std::vector<uint32_t> rays;
    ok = f && fread(&M, 8, 1, f) == 1 && M >= 0 && read_n(f, rays, 8 * (size_t)M);
    if (f) fclose(f);
    if (!ok) { fprintf(stderr, "bad rays file\n"); return 2; }

    NearestBvh bvh;
    nearest_build(V.data(), T.data(), nt, leaf, bvh);
    if (bvh.depth > nearest_depth_bound(nt, leaf) || bvh.depth - 1 > kNearestStack) {
        printf("FAIL: depth %d past its bound\n", bvh.depth);
        return 1;
    }
    AnyClasses cls;
    cls.surface = surface.empty() ? nullptr : surface.data();
    cls.flags = flags.empty() ? nullptr : flags.data();
    cls.count = (uint32_t)flags.size();

    std::vector<uint32_t> out(7 * (size_t)M);
    const int64_t node_count = (int64_t)bvh.nodes.size();
    auto work = [&](int64_t begin, int64_t end) {
        for (int64_t k = begin; k < end; k++) {
            float w[7];
            memcpy(w, &rays[8 * (size_t)k], 28);
            const float o[3] = { w[0], w[1], w[2] }, d[3] = { w[3], w[4], w[5] };
            const NearestRay r = nearest_ray(o, d, w[6], rays[8 * (size_t)k + 7]);
            uint32_t stack[kNearestStack], stack2[kNearestStack];
            NearestStats sa, sn;
            uint32_t *q = &out[7 * (size_t)k];
            q[0] = any_brute(bvh.tris.data(), nt, cls, r);
            q[1] = any_traverse(bvh.nodes.data(), node_count, bvh.tris.data(), cls, r, [&](int i) -> uint32_t & { return stack[i]; }, sa);
            (void)nearest_traverse(bvh.nodes.data(), node_count, bvh.tris.data(), r, [&](int i) -> uint32_t & { return stack2[i]; }, sn);
            q[2] = (uint32_t)sa.nodes; q[3] = (uint32_t)sa.tris; q[4] = (uint32_t)sn.nodes; q[5] = (uint32_t)sn.tris;
            q[6] = (uint32_t)sa.max_stack;
        }
    };
    int threads = (int)std::thread::hardware_concurrency();
    threads = threads < 1 ? 1 : threads > 16 ? 16 : threads;
    if (M * (nt + 1) < 4000000) threads = 1;
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++) pool.emplace_back(work, M * t / threads, M * (t + 1) / threads);
    for (std::thread &t : pool) t.join();

    int64_t count[3] = { 0, 0, 0 }, differ = 0, an = 0, at = 0, nn = 0, ntr = 0;
    int max_stack = 0, fails = 0;
    for (int64_t k = 0; k < M; k++) {
        const uint32_t *q = &out[7 * (size_t)k];
        if (q[0] > 2 || q[0] != q[1]) {
            differ++;
            if (fails++ < 20) printf("FAIL ray %lld: brute %u traversal %u\n", (long long)k, q[0], q[1]);
            continue;
        }
        count[q[0]]++;
        an += q[2]; at += q[3]; nn += q[4]; ntr += q[5];
        if ((int)q[6] > max_stack) max_stack = (int)q[6];
    }
    if (max_stack > (bvh.depth > 0 ? bvh.depth - 1 : 0)) { printf("FAIL: %d stack entries in a tree of %d levels\n", max_stack, bvh.depth); fails++; }
    f = fopen(argv[3], "wb");
    ok = f && (out.empty() || fwrite(out.data(), 4, out.size(), f) == out.size());
    if (f) fclose(f);
    if (!ok) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("ok any: nt %lld leaf %d depth %d nodes %lld rays %lld clear %lld blocked %lld veiled %lld differ %lld any_nodes %lld any_tris %lld "
           "nearest_nodes %lld nearest_tris %lld max_stack %d\n", (long long)nt, leaf, bvh.depth, (long long)node_count, (long long)M,
           (long long)count[0], (long long)count[1], (long long)count[2], (long long)differ, (long long)an, (long long)at, (long long)nn,
           (long long)ntr, max_stack);
    return 0;
}
