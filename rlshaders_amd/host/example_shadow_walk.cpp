// example_shadow_walk.cpp -- shadow rays walked on the device (rls_shadow_walk.hpp): rlGgx points under two lights emit their light
// loop's shadow queue (rlsb::emitDirect); above them lies a stack of three tinted, semi-transparent rlGgx slabs and, on the way to
// the first light, one opaque sphere.  Every round the nearest hit of the active rays comes from a twenty-line closest-hit function
// on the host -- all a wavefront renderer has -- and names its surface by index into a four-entry table of sg->out_opacity the
// library formed (rlsb::ggxOpacity at a shadow ray's point); rlsb::ShadowWalk::step multiplies it in, ends the rays the sphere
// blocks and lists the rest.  rlsb::resolveDirect then lights the points under the walk's visibility.
//
// usage: example_shadow_walk [points] [spp_n] [max_steps]; prints one JSON line: the active rays before every step, the rays left
// black, and checksums (FNV-1a over the bits) of the visibility of the queue's rays and of the two AOVs, which
// tests/test_gpu_shadow_walk_host_cpp.py compares with the Python path (rlshaders_amd.shadow_walk).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rls_shadow_walk.hpp"

namespace {
constexpr uint32_t kSeed = 1234;
constexpr int kSlabs = 3;
const float kSlabZ[kSlabs] = {0.5f, 0.8f, 1.1f};                       // the slabs: the planes z = kSlabZ[k], surfaces 0 .. 2
const float kSlabKt[kSlabs][3] = {{0.2f, 0.9f, 0.7f}, {0.8f, 0.4f, 0.6f}, {0.5f, 0.5f, 1.0f}};
const float kCenter[3] = {-1.63f, 0.82f, 1.23f};                       // the sphere, surface 3
constexpr float kRadius = 0.25f;
constexpr float kTMin = 1e-3f;                                         // a root at or below it is the surface the ray stands on

uint64_t fnv(const std::vector<float> &v)
{
    const uint8_t *p = reinterpret_cast<const uint8_t *>(v.data());
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < 4 * v.size(); k++) { h ^= p[k]; h *= 1099511628211ull; }
    return h;
}

// the renderer's tracer: the closest surface in (kTMin, maxdist] from o along the unit direction d -> its index and t, or -1
int closestHit(const float o[3], const float d[3], float maxdist, float &t)
{
    int surface = -1;
    t = 0.0f;
    for (int k = 0; k < kSlabs; k++) {
        if (d[2] == 0.0f) continue;
        const float tk = (kSlabZ[k] - o[2]) / d[2];
        if (tk > kTMin && tk <= maxdist && (surface < 0 || tk < t)) { surface = k; t = tk; }
    }
    const float oc[3] = {o[0] - kCenter[0], o[1] - kCenter[1], o[2] - kCenter[2]};
    const float b = (oc[0] * d[0] + oc[1] * d[1]) + oc[2] * d[2];
    const float c = ((oc[0] * oc[0] + oc[1] * oc[1]) + oc[2] * oc[2]) - kRadius * kRadius;
    const float disc = b * b - c;
    if (disc >= 0.0f) {
        const float sq = std::sqrt(disc), t0 = -b - sq, t1 = -b + sq;
        const float ts = t0 > kTMin ? t0 : t1;
        if (ts > kTMin && ts <= maxdist && (surface < 0 || ts < t)) { surface = kSlabs; t = ts; }
    }
    return surface;
}

template <class T>
std::vector<T> download(const rlsb::Device &dev, const T *p, int64_t count)
{
    std::vector<T> v((size_t)count);
    if (count > 0) rlsb::check(rls_copy_to_host(dev.ctx(), v.data(), p, sizeof(T) * v.size()));
    return v;
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

        // 1. the light loop's shadow rays
        rlsb::ShadowQueue sq(dev, n, 2, spp_n, rlsb::ShadowQueue::Ggx);
        rlsb::emitDirect(dev, c, sh, P, lights, 2, n, spp_n, kSeed, sq);

        // 2. the four surfaces, shaded as shadow rays' points: the slabs 1 - KtColor * Kt at Kt = 0.5, the sphere (Kt = 0) opaque
        const int surfaces = kSlabs + 1;
        std::vector<uint8_t> type((size_t)(5 * surfaces), 0);
        for (int k = 0; k < surfaces; k++) type[(size_t)k] = RLS_RT_SHADOW;
        rlsb::RayState shadowPoints(dev, type);
        rlsb::Planes table(dev, surfaces, 3);
        for (int k = 0; k < surfaces; k++) {
            rls_ggx_opacity o = {};
            o.opacity = rls_param{nullptr, 1.0f};
            o.opacity_color = rlsb::ParamRGB(1.0f, 1.0f, 1.0f).c();
            o.KtColor = k < kSlabs ? rlsb::ParamRGB(kSlabKt[k][0], kSlabKt[k][1], kSlabKt[k][2]).c() : rlsb::ParamRGB(1.0f, 1.0f, 1.0f).c();
            o.Kt = rls_param{nullptr, k < kSlabs ? 0.5f : 0.0f};
            rlsb::ggxOpacity(dev, o, 1, shadowPoints.c(k).ray_type, rls_rgb{table.plane(0) + k, table.plane(1) + k, table.plane(2) + k});
        }

        // 3. the walk: begin reads the ray count on the device; every round the host traces the listed rays
        const int64_t cap = sq.c().capacity;
        rlsb::ShadowWalk walk(dev, cap);
        walk.begin(sq, P, max_steps);
        const int64_t slots = cap > 0 ? cap : 1;
        rlsb::Planes found(dev, slots, 4);                           // t, P of the listed rays
        void *dhit = nullptr, *dindex = nullptr;
        rlsb::check(rls_device_alloc(dev.ctx(), (size_t)slots, &dhit));
        rlsb::check(rls_device_alloc(dev.ctx(), (size_t)slots * sizeof(uint32_t), &dindex));
        std::printf("{\"points\": %lld, \"spp_n\": %d, \"steps\": [", (long long)n, spp_n);
        int steps = 0;
        for (int64_t m; (m = walk.active()) > 0; steps++) {
            std::printf("%s%lld", steps ? ", " : "", (long long)m);
            const rls_walk_rays &r = walk.rays();
            std::vector<float> o[3], d[3], md = download(dev, r.maxdist, m);
            for (int k = 0; k < 3; k++) { o[k] = download(dev, (&r.origin.x)[k], m); d[k] = download(dev, (&r.dir.x)[k], m); }
            std::vector<uint8_t> hit((size_t)slots, 0);
            std::vector<uint32_t> index((size_t)slots, 0u);
            std::vector<float> f((size_t)(4 * slots), 0.0f);
            for (int64_t k = 0; k < m; k++) {
                const float ok[3] = {o[0][(size_t)k], o[1][(size_t)k], o[2][(size_t)k]};
                const float dk[3] = {d[0][(size_t)k], d[1][(size_t)k], d[2][(size_t)k]};
                float t;
                const int surface = closestHit(ok, dk, md[(size_t)k], t);
                if (surface < 0) continue;
                hit[(size_t)k] = 1;
                index[(size_t)k] = (uint32_t)surface;
                f[(size_t)k] = t;
                for (int a = 0; a < 3; a++) f[(size_t)((1 + a) * slots + k)] = ok[a] + dk[a] * t;
            }
            found.upload(f);
            rlsb::check(rls_copy_to_device(dev.ctx(), dhit, hit.data(), hit.size()));
            rlsb::check(rls_copy_to_device(dev.ctx(), dindex, index.data(), index.size() * sizeof(uint32_t)));
            rls_shadow_walk_found wf = {};
            wf.hit = static_cast<const uint8_t *>(dhit); wf.t = found.plane(0); wf.P = found.cvec3(1);
            wf.opacity = rls_crgb{table.plane(0), table.plane(1), table.plane(2)};
            wf.index = static_cast<const uint32_t *>(dindex); wf.table_count = (uint32_t)surfaces;
            walk.step(wf, m);
        }
        rlsb::check(rls_device_free(dev.ctx(), dhit));
        rlsb::check(rls_device_free(dev.ctx(), dindex));

        // 4. the light loop under the walked visibility
        rlsb::Planes dd(dev, n, 3), ds(dev, n, 3);
        rlsb::resolveDirect(dev, c, sh, lights, 2, sq, walk.visibility(), dd, ds);

        const int64_t rays = sq.count();
        const std::vector<float> all = walk.visibility().download();
        std::vector<float> vis;
        for (int k = 0; k < 3; k++) vis.insert(vis.end(), all.begin() + (size_t)(k * slots), all.begin() + (size_t)(k * slots + rays));
        long long black = 0;
        double mean = 0.0;
        for (int64_t j = 0; j < rays; j++)
            if (vis[(size_t)j] == 0.0f && vis[(size_t)(rays + j)] == 0.0f && vis[(size_t)(2 * rays + j)] == 0.0f) black++;
        for (float v : vis) mean += v;
        std::printf("], \"rays\": %lld, \"black\": %lld, \"visibility\": \"%016llx\", \"direct_diffuse\": \"%016llx\", "
                    "\"direct_specular\": \"%016llx\", \"mean_visibility\": %.9g}\n", (long long)rays, black,
                    (unsigned long long)fnv(vis), (unsigned long long)fnv(dd.download()), (unsigned long long)fnv(ds.download()),
                    vis.empty() ? 0.0 : mean / (double)vis.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "example_shadow_walk: %s\n", e.what());
        return 1;
    }
    return 0;
}
