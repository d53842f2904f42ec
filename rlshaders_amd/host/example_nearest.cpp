// example_nearest.cpp -- a light loop's shadow rays walked through a triangle mesh with no host tracer (rls_nearest.hpp over
// rls_shadow_walk.hpp): rlGgx points under two lights emit their shadow queue (rlsb::emitDirect); above them lies a tinted,
// semi-transparent quad and, on the way to the first light, an opaque tessellated sphere (a subdivided octahedron, 512
// triangles).  Every round rlsb::NearestScene::hits answers the nearest hit of the listed rays on the device -- `last` keeps a ray
// from meeting the triangle it stands on again -- and its planes go to rlsb::ShadowWalk::step as they are: the hit's surface
// indexes a two-entry table of sg->out_opacity (rlsb::ggxOpacity).  rlsb::resolveDirect then lights the points under the walk's
// visibility.  Then rlSss's probe rays of points on the sphere (rlsb::emitProbes) are walked through the same scene by
// rlsb::ProbeWalk over the same query, its planes handed over as rls_walk_found (hit, t, P, N, Ns: the sphere carries per-vertex
// normals, so Ns is not N).  The host reads one number a round, the active count.
//
// usage: example_nearest [points] [spp_n] [max_steps]; prints one JSON line: the scene's size, the active rays before every step,
// the rays left black, checksums (FNV-1a over the bits) of the visibility of the queue's rays and of the two AOVs, and under
// "probes" the steps, the hits stored and checksums of the hit counts and of the stored hits' P and N, which
// tests/test_gpu_nearest_host_cpp.py compares with the Python path (rlshaders_amd.nearest).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "rls_nearest.hpp"
#include "rls_shadow_walk.hpp"
#include "rls_walk.hpp"

namespace {
constexpr uint32_t kSeed = 1234;
constexpr float kQuadZ = 0.8f, kQuadHalf = 10.0f;                      // the quad: surface 0
const float kQuadKt[3] = {0.2f, 0.9f, 0.7f};
const double kCenter[3] = {-1.63, 0.82, 1.23};                         // the sphere: surface 1
constexpr double kRadius = 0.25;
constexpr int kLevel = 3;

uint64_t fnv(const void *data, size_t bytes)
{
    const uint8_t *p = static_cast<const uint8_t *>(data);
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < bytes; k++) { h ^= p[k]; h *= 1099511628211ull; }
    return h;
}
uint64_t fnv(const std::vector<float> &v) { return fnv(v.data(), 4 * v.size()); }

template <class T>
std::vector<T> download(const rlsb::Device &dev, const T *p, int64_t count)
{
    std::vector<T> v((size_t)count);
    if (count > 0) rlsb::check(rls_copy_to_host(dev.ctx(), v.data(), p, sizeof(T) * v.size()));
    return v;
}

// An octahedron subdivided kLevel times, every new vertex the normalised sum of its edge's ends (+, *, /, sqrt in double, in
// this order: the Python test builds the same floats), then the quad's four vertices and two triangles.  Nn: the per-vertex
// shading normals, the sphere's unit positions and the quad's +z.
void buildMesh(std::vector<float> &V, std::vector<uint32_t> &T, std::vector<uint32_t> &S, std::vector<float> &Nn)
{
    std::vector<double> U = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
    std::vector<uint32_t> F = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
    for (int l = 0; l < kLevel; l++) {
        std::map<std::pair<uint32_t, uint32_t>, uint32_t> mid;
        auto middle = [&](uint32_t a, uint32_t b) {
            const auto key = std::make_pair(a < b ? a : b, a < b ? b : a);
            const auto it = mid.find(key);
            if (it != mid.end()) return it->second;
            const double x = U[3 * a] + U[3 * b], y = U[3 * a + 1] + U[3 * b + 1], z = U[3 * a + 2] + U[3 * b + 2];
            const double len = std::sqrt((x * x + y * y) + z * z);
            const uint32_t i = (uint32_t)(U.size() / 3);
            U.push_back(x / len); U.push_back(y / len); U.push_back(z / len);
            mid[key] = i;
            return i;
        };
        std::vector<uint32_t> F2;
        for (size_t t = 0; t < F.size(); t += 3) {
            const uint32_t a = F[t], b = F[t + 1], c = F[t + 2], ab = middle(a, b), bc = middle(b, c), ca = middle(c, a);
            const uint32_t add[12] = {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca};
            F2.insert(F2.end(), add, add + 12);
        }
        F.swap(F2);
    }
    for (size_t i = 0; i < U.size(); i++) { V.push_back((float)(kCenter[i % 3] + kRadius * U[i])); Nn.push_back((float)U[i]); }
    T = F;
    S.assign(T.size() / 3, 1u);
    const uint32_t q = (uint32_t)(V.size() / 3);
    const float corners[4][2] = {{-kQuadHalf, -kQuadHalf}, {kQuadHalf, -kQuadHalf}, {kQuadHalf, kQuadHalf}, {-kQuadHalf, kQuadHalf}};
    for (const auto &c : corners) {
        V.push_back(c[0]); V.push_back(c[1]); V.push_back(kQuadZ);
        Nn.push_back(0.0f); Nn.push_back(0.0f); Nn.push_back(1.0f);
    }
    const uint32_t quad[6] = {q, q + 1, q + 2, q, q + 2, q + 3};
    T.insert(T.end(), quad, quad + 6);
    S.push_back(0u); S.push_back(0u);
}
} // namespace

int main(int argc, char **argv)
{
    const int64_t n = argc > 1 ? std::atoll(argv[1]) : 4096;
    const int spp_n = argc > 2 ? std::atoi(argv[2]) : 4;
    const int max_steps = argc > 3 ? std::atoi(argv[3]) : 8;
    try {
        rlsb::Device dev(0);
        rlsb::Planes frame(dev, n, 9);
        rlsb::check(rls_gen_frame(dev.ctx(), kSeed, 0, n, frame.vec3(0), frame.vec3(3), frame.vec3(6)));
        rls_ggx_closure c = {};
        c.wo = frame.cvec3(0); c.N = frame.cvec3(3); c.T = frame.cvec3(6);
        c.KsColor = rlsb::ParamRGB(0.9f, 0.6f, 0.3f).c();
        c.specularRoughness = rls_param{nullptr, 0.4f};
        c.ior = rls_param{nullptr, 1.6f};
        c.anisotropic = rls_param{nullptr, 0.5f};
        rls_ggx_shader sh = {};
        sh.KdColor = rlsb::ParamRGB(0.7f, 0.5f, 0.2f).c();
        sh.Kd = rls_param{nullptr, 0.8f};
        sh.diffuseRoughness = rls_param{nullptr, 0.3f};
        sh.Ks = rls_param{nullptr, 0.6f};
        rls_sphere_light lights[2] = {};
        const float centers[2][3] = {{-4.0f, 2.0f, 3.0f}, {6.0f, 1.0f, 2.0f}};
        const float radiances[2][3] = {{3.0f, 2.0f, 1.0f}, {1.0f, 4.0f, 2.0f}};
        for (int l = 0; l < 2; l++) {
            for (int k = 0; k < 3; k++) { lights[l].center[k] = centers[l][k]; lights[l].radiance[k] = radiances[l][k]; }
            lights[l].radius = 1.0f;
            lights[l].mis_mode = RLS_MIS_BOTH;
        }
        rlsb::Planes P(dev, std::vector<float>((size_t)(3 * n), 0.0f), 3);

        // 1. the scene: the tree is built on the host and uploaded once
        std::vector<float> V, Nn;
        std::vector<uint32_t> T, S;
        buildMesh(V, T, S, Nn);
        rls_nearest_mesh mesh = {};
        mesh.nv = (int64_t)(V.size() / 3); mesh.nt = (int64_t)(T.size() / 3);
        mesh.vertices = V.data(); mesh.triangles = T.data(); mesh.surface = S.data(); mesh.normals = Nn.data();
        rlsb::NearestScene scene(dev, mesh);
        const rls_nearest_scene_info info = scene.info();

        // 2. the light loop's shadow rays
        rlsb::ShadowQueue sq(dev, n, 2, spp_n, rlsb::ShadowQueue::Ggx);
        rlsb::emitDirect(dev, c, sh, P, lights, 2, n, spp_n, kSeed, sq);

        // 3. the two surfaces, shaded as shadow rays' points: the quad 1 - KtColor * Kt at Kt = 0.5, the sphere (Kt = 0) opaque
        const int surfaces = 2;
        std::vector<uint8_t> type((size_t)(5 * surfaces), 0);
        for (int k = 0; k < surfaces; k++) type[(size_t)k] = RLS_RT_SHADOW;
        rlsb::RayState shadowPoints(dev, type);
        rlsb::Planes table(dev, surfaces, 3);
        for (int k = 0; k < surfaces; k++) {
            rls_ggx_opacity o = {};
            o.opacity = rls_param{nullptr, 1.0f};
            o.opacity_color = rlsb::ParamRGB(1.0f, 1.0f, 1.0f).c();
            o.KtColor = k == 0 ? rlsb::ParamRGB(kQuadKt[0], kQuadKt[1], kQuadKt[2]).c() : rlsb::ParamRGB(1.0f, 1.0f, 1.0f).c();
            o.Kt = rls_param{nullptr, k == 0 ? 0.5f : 0.0f};
            rlsb::ggxOpacity(dev, o, 1, shadowPoints.c(k).ray_type, rls_rgb{table.plane(0) + k, table.plane(1) + k, table.plane(2) + k});
        }

        // 4. the walk: every round the device answers the listed rays' nearest hits; the host reads the active count alone
        const int64_t cap = sq.c().capacity;
        rlsb::ShadowWalk walk(dev, cap);
        walk.begin(sq, P, max_steps);
        rlsb::NearestFound found(dev, cap, rlsb::NearestFound::ForShadowWalk);
        found.resetLast(dev);
        std::printf("{\"points\": %lld, \"spp_n\": %d, \"triangles\": %lld, \"nodes\": %lld, \"depth\": %d, \"steps\": [", (long long)n, spp_n,
                    (long long)info.nt, (long long)info.nodes, info.depth);
        int steps = 0;
        for (int64_t m; (m = walk.active()) > 0; steps++) {
            std::printf("%s%lld", steps ? ", " : "", (long long)m);
            scene.hits(walk.rays(), m, found);
            walk.step(found.shadowFound(rls_crgb{table.plane(0), table.plane(1), table.plane(2)}, (uint32_t)surfaces), m);
        }

        // 5. the light loop under the walked visibility
        rlsb::Planes dd(dev, n, 3), ds(dev, n, 3);
        rlsb::resolveDirect(dev, c, sh, lights, 2, sq, walk.visibility(), dd, ds);

        const int64_t rays = sq.count(), slots = cap > 0 ? cap : 1;
        const std::vector<float> all = walk.visibility().download();
        std::vector<float> vis;
        for (int k = 0; k < 3; k++) vis.insert(vis.end(), all.begin() + (size_t)(k * slots), all.begin() + (size_t)(k * slots + rays));
        long long black = 0;
        double mean = 0.0;
        for (int64_t j = 0; j < rays; j++)
            if (vis[(size_t)j] == 0.0f && vis[(size_t)(rays + j)] == 0.0f && vis[(size_t)(2 * rays + j)] == 0.0f) black++;
        for (float v : vis) mean += v;
        std::printf("], \"rays\": %lld, \"black\": %lld, \"visibility\": \"%016llx\", \"direct_diffuse\": \"%016llx\", "
                    "\"direct_specular\": \"%016llx\", \"mean_visibility\": %.9g, ", (long long)rays, black,
                    (unsigned long long)fnv(vis), (unsigned long long)fnv(dd.download()), (unsigned long long)fnv(ds.download()),
                    vis.empty() ? 0.0 : mean / (double)vis.size());

        // 6. rlSss's probe rays of n points on the sphere, walked through the same scene: the same query, its planes as rls_walk_found
        rls_sss_closure sc = {};
        sc.sss_color = rlsb::ParamRGB(0.8f, 0.5f, 0.3f).c();
        sc.sss_dist_multiplier = rls_param{nullptr, 1.0f};
        sc.sss_scatter_dist[0] = rls_param{nullptr, 0.05f};
        sc.sss_scatter_dist[1] = rls_param{nullptr, 0.1f};
        sc.sss_scatter_dist[2] = rls_param{nullptr, 0.2f};
        sc.N = frame.cvec3(3); sc.T = frame.cvec3(6); sc.has_dPdu = 1;
        const std::vector<float> pts = frame.download();
        std::vector<float> Ph((size_t)(3 * n));
        for (int a = 0; a < 3; a++)
            for (int64_t i = 0; i < n; i++) Ph[(size_t)(a * n + i)] = (float)kCenter[a] + (float)kRadius * pts[(size_t)((3 + a) * n + i)];
        rlsb::Planes Pp(dev, Ph, 3);
        const int64_t prays = n * spp_n * spp_n, pslots = prays > 0 ? prays : 1;
        rlsb::ProbeQueue pq(dev, n, spp_n);
        rlsb::emitProbes(dev, sc, Pp, n, spp_n, kSeed, pq);
        rlsb::ProbeWalk pwalk(dev, prays);
        pwalk.begin(pq, Pp);
        rlsb::NearestFound pfound(dev, prays, rlsb::NearestFound::ForWalk);
        pfound.resetLast(dev);
        std::printf("\"probes\": {\"rays\": %lld, \"steps\": [", (long long)prays);
        int psteps = 0;
        for (int64_t m; (m = pwalk.active()) > 0; psteps++) {
            std::printf("%s%lld", psteps ? ", " : "", (long long)m);
            scene.hits(pwalk.rays(), m, pfound);
            pwalk.step(pfound.walkFound(false), m);                  // one object everywhere: no ids
        }
        const rls_walk_hits &wh = pwalk.c().hits;
        const std::vector<uint8_t> cnt = download(dev, wh.count, prays);
        std::vector<float> hitP, hitN;                               // the stored hits alone, plane by plane, slot-major
        for (int a = 0; a < 3; a++) {
            const std::vector<float> pa = download(dev, (&wh.P.x)[a], pslots * wh.max_hits), na = download(dev, (&wh.N.x)[a], pslots * wh.max_hits);
            for (int k = 0; k < wh.max_hits; k++)
                for (int64_t j = 0; j < prays; j++)
                    if (k < cnt[(size_t)j]) { hitP.push_back(pa[(size_t)(k * wh.stride + j)]); hitN.push_back(na[(size_t)(k * wh.stride + j)]); }
        }
        long long stored = 0;
        for (uint8_t c8 : cnt) stored += c8;
        std::printf("], \"hits\": %lld, \"count\": \"%016llx\", \"P\": \"%016llx\", \"N\": \"%016llx\"}}\n", stored,
                    (unsigned long long)fnv(cnt.data(), cnt.size()), (unsigned long long)fnv(hitP), (unsigned long long)fnv(hitN));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "example_nearest: %s\n", e.what());
        return 1;
    }
    return 0;
}
