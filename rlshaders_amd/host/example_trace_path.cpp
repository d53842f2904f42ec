// example_trace_path.cpp -- a two-bounce loop over a mixed scene from C++ (rls_trace.hpp: HitRoutes, routeHits, gatherHits,
// scatterToRays, fillMisses beside emitBounce / resolveBounce / advanceState).  The camera hits of an rlGgx surface are shaded
// under an all-camera state and their glossy queue is taken: its rays' state is advanced, a stand-in tracer gives every ray a
// hit -- the node bin (rlGgx, rlDisney or a miss) and the hit's frame, both fixed functions of the ray index -- and the hits are
// routed: split by bin, each bin's frame and state gathered into a dense batch, the batch shaded by its node under unit
// visibility and a uniform radiance, its out scattered back to the rays' places in the glossy queue's radiance planes.  The
// misses get the environment there; the camera batch is then resolved with those planes.
//
//   example_trace_path [points] [spp_n]
// prints one JSON line: the bin sizes and checksums (FNV-1a over the bits of the planes), which
// tests/test_gpu_trace_route_host_cpp.py compares with the Python path (rlshaders_amd/trace.py) on the same inputs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rls_trace.hpp"

namespace {
constexpr uint32_t kSeed = 1234, kHitSeed = 4321;
const float kEnv[3] = {0.25f, 0.3f, 0.4f};          // what a miss sees
const float kDeep[3] = {0.5f, 0.4f, 0.3f};          // the uniform radiance of every ray that is not routed

uint64_t fnv(const std::vector<float> &v)
{
    const uint8_t *p = reinterpret_cast<const uint8_t *>(v.data());
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < 4 * v.size(); k++) { h ^= p[k]; h *= 1099511628211ull; }
    return h;
}

// the stand-in tracer's bin of ray k: 3 in 8 hit the rlGgx surface, 3 in 8 the rlDisney surface, 2 in 8 nothing
uint8_t hit_bin(uint32_t k)
{
    const uint32_t h = (k * 2654435761u) >> 29;
    return h < 3 ? 0 : h < 6 ? 1 : 255;
}
} // namespace

int main(int argc, char **argv)
{
    const int64_t n = argc > 1 ? std::atoll(argv[1]) : 4096;
    const int spp_n = argc > 2 ? std::atoi(argv[2]) : 4;
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
        sh.KtColor = rlsb::ParamRGB(0.2f, 0.9f, 0.7f).c();
        sh.Kt = rls_param{nullptr, 0.5f};
        rls_disney_closure dc = {};
        dc.base_color = rlsb::ParamRGB(0.8f, 0.5f, 0.3f).c();
        dc.subsurface = rls_param{nullptr, 0.1f};
        dc.metallic = rls_param{nullptr, 0.2f};
        dc.specular = rls_param{nullptr, 0.5f};
        dc.specular_tint = rls_param{nullptr, 0.1f};
        dc.roughness = rls_param{nullptr, 0.35f};
        dc.anisotropic = rls_param{nullptr, 0.3f};
        dc.sheen = rls_param{nullptr, 0.2f};
        dc.sheen_tint = rls_param{nullptr, 0.5f};
        dc.clearcoat = rls_param{nullptr, 0.3f};
        dc.clearcoat_gloss = rls_param{nullptr, 0.6f};
        rls_sphere_light lights[2] = {};
        const float centers[2][3] = {{-4.0f, 2.0f, 3.0f}, {6.0f, 1.0f, 2.0f}};
        const float radiances[2][3] = {{3.0f, 2.0f, 1.0f}, {1.0f, 4.0f, 2.0f}};
        for (int l = 0; l < 2; l++) {
            for (int k = 0; k < 3; k++) { lights[l].center[k] = centers[l][k]; lights[l].radiance[k] = radiances[l][k]; }
            lights[l].radius = 1.0f;
            lights[l].mis_mode = RLS_MIS_BOTH;
        }
        const rls_gi_depths depths = {4, 1, 1, 2};
        rlsb::Planes P(dev, std::vector<float>((size_t)(3 * n), 0.0f), 3);

        // three planes of `count` floats, plane k holding v[k]
        auto uniform = [&](int64_t count, const float *v) {
            std::vector<float> h((size_t)(3 * count));
            for (int k = 0; k < 3; k++) std::fill(h.begin() + (size_t)(k * count), h.begin() + (size_t)((k + 1) * count), v[k]);
            return rlsb::Planes(dev, h, 3);
        };
        const float one[3] = {1.0f, 1.0f, 1.0f}, zero[3] = {0.0f, 0.0f, 0.0f};

        // 1. the camera hits: every queue of the node; the glossy queue is the one followed
        rlsb::RayState camera = rlsb::RayState::camera(dev, n);
        rlsb::GgxNodeQueues nq(dev, n, 2, spp_n);
        rlsb::emitBounce(dev, c, sh, P, lights, 2, n, spp_n, kSeed, camera.c(), depths, nq);
        const int64_t rays = nq.glossy().count(), cap = nq.glossy().c().capacity;
        rlsb::RayState hits(dev, rays);
        rlsb::advanceState(dev, rays, nq.glossy().c().point, camera.c(), RLS_RT_GLOSSY, hits);

        // 2. the stand-in tracer: a bin and a frame per ray
        std::vector<uint8_t> bin_host((size_t)rays);
        for (int64_t k = 0; k < rays; k++) bin_host[(size_t)k] = hit_bin((uint32_t)k);
        rlsb::Planes binBytes(dev, (rays + 3) / 4 + 1, 1);                         // (>= rays bytes)
        const uint8_t *bin = reinterpret_cast<const uint8_t *>(binBytes.plane(0));
        if (rays > 0) rlsb::check(rls_copy_to_device(dev.ctx(), binBytes.plane(0), bin_host.data(), bin_host.size()));
        rlsb::Planes hit(dev, rays, 9);                                            // wo, N, T per ray
        rlsb::check(rls_gen_frame(dev.ctx(), kHitSeed, 0, rays, hit.vec3(0), hit.vec3(3), hit.vec3(6)));
        const rlsb::Planes hitP = uniform(rays, zero);                             // sg->P per ray

        // 3. route, and shade each bin's dense batch by its node
        rlsb::HitRoutes routes(dev, rays, 2);
        rlsb::routeHits(dev, bin, routes);
        rlsb::Planes L = uniform(cap, zero);                                       // the glossy queue's radiance, in ray order
        std::printf("{\"points\": %lld, \"spp_n\": %d, \"rays\": %lld, \"sizes\": [%lld, %lld, %lld]", (long long)n, spp_n,
                    (long long)rays, (long long)routes.size(0), (long long)routes.size(1), (long long)routes.size(2));
        for (int b = 0; b < 2; b++) {
            const int64_t m = routes.size(b);
            rlsb::Planes batch(dev, m, 9), Pb(dev, m, 3), out(dev, m, 3);
            rlsb::RayState state(dev, m);
            rlsb::gatherHits(dev, routes, b, rlsb::RoutePlanes().planes(hit, batch, 9).planes(hitP, Pb, 3).state(hits.c(), state.c()));
            if (b == 0) {
                rls_ggx_closure cb = c;
                cb.wo = batch.cvec3(0); cb.N = batch.cvec3(3); cb.T = batch.cvec3(6);
                rlsb::GgxNodeQueues q(dev, m, 2, spp_n);
                rlsb::emitBounce(dev, cb, sh, Pb, lights, 2, m, spp_n, kSeed, state.c(), depths, q, (uint64_t)n);
                const rlsb::Planes vis = uniform(q.shadow()->c().capacity, one);
                const rlsb::Planes Lg = uniform(q.glossy().c().capacity, kDeep), Lt = uniform(q.refract().c().capacity, kDeep),
                                   Ld = uniform(q.diffuse().c().capacity, kDeep);
                rlsb::Planes aovs(dev, m, 15);
                rlsb::resolveBounce(dev, cb, sh, lights, 2, state.c(), depths, q, vis, Lg, Lt, Ld, aovs, &out);
            } else {
                rls_disney_closure cb = dc;
                cb.wo = batch.cvec3(0); cb.N = batch.cvec3(3); cb.T = batch.cvec3(6);
                rlsb::DisneyNodeQueues q(dev, m, 2, spp_n);
                rlsb::emitBounce(dev, cb, Pb, lights, 2, m, spp_n, kSeed, state.c(), depths, q, (uint64_t)n);
                const rlsb::Planes vis = uniform(q.shadow()->c().capacity, one);
                const rlsb::Planes Ld = uniform(q.diffuse().c().capacity, kDeep), Ls = uniform(q.specular().c().capacity, kDeep);
                rlsb::Planes aovs(dev, m, 12);
                const rls_param kd = {nullptr, 0.5f}, ks = {nullptr, 0.25f};      // indirectDiffuseScale, indirectSpecularScale
                rlsb::resolveBounce(dev, cb, kd, ks, lights, 2, state.c(), depths, q, vis, Ld, Ls, aovs, &out);
            }
            rlsb::scatterToRays(dev, routes, b, rlsb::RoutePlanes().planes(out, L, 3));
            std::printf(", \"out%d\": \"%016llx\"", b, (unsigned long long)fnv(out.download()));
        }
        rlsb::fillMisses(dev, routes, kEnv, L);

        // 4. the camera batch with the routed radiance in its glossy queue
        {
            const rlsb::Planes vis = uniform(nq.shadow()->c().capacity, one);
            const rlsb::Planes Lt = uniform(nq.refract().c().capacity, kDeep), Ld = uniform(nq.diffuse().c().capacity, kDeep);
            rlsb::Planes aovs(dev, n, 15), out(dev, n, 3);
            rlsb::resolveBounce(dev, c, sh, lights, 2, camera.c(), depths, nq, vis, L, Lt, Ld, aovs, &out);
            const std::vector<float> ro = out.download();
            double mean = 0.0;
            for (float v : ro) mean += v;
            std::printf(", \"radiance\": \"%016llx\", \"aovs\": \"%016llx\", \"out\": \"%016llx\", \"mean_out\": %.9g}\n",
                        (unsigned long long)fnv(L.download()), (unsigned long long)fnv(aovs.download()),
                        (unsigned long long)fnv(ro), ro.empty() ? 0.0 : mean / (double)ro.size());
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "example_trace_path: %s\n", e.what());
        return 1;
    }
    return 0;
}
