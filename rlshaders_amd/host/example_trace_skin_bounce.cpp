// example_trace_skin_bounce.cpp -- rlSkin at the hits of secondary rays through the caller's tracer from C++ (rls_trace.hpp:
// SkinBounceQueues, emitBounce, resolveBounce, RayState, advanceState).  A camera wave of skin points is shaded under an
// all-camera state: the node's queues are emitted, the lights left unoccluded, a uniform radiance put on every glossy ray, the
// probe rays walked through each point's tangent plane on the host (E = 1 / pi), and the AOVs resolved.  The state is then
// advanced along the specular lobe's glossy queue with RLS_RT_GLOSSY -- each ray's hit is a glossy secondary point one bounce
// deeper -- and the first min(rays, points) of those rays are given stand-in hits: hit k has the surface of shading point k.
// That second wave is shaded under the advanced state: no glossy ray leaves a point with Rr = 1, the lobes' mean Fresnel is
// their light loops' alone, and sssWeight follows.
//
//   example_trace_skin_bounce [points] [spp_n]
// prints one JSON line: per wave the ray counts, the probe hits found and checksums (FNV-1a over the bits of the resolved planes
// and of the three hand-down scalars; over the advanced state's bytes), which tests/test_gpu_trace_skin_bounce_host_cpp.py
// compares with the Python path (rlshaders_amd/trace.py) on the same inputs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rls_trace.hpp"

namespace {
constexpr uint32_t kSeed = 1234;

uint64_t fnv_bytes(const uint8_t *p, size_t count)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < count; k++) { h ^= p[k]; h *= 1099511628211ull; }
    return h;
}
uint64_t fnv(const std::vector<float> &v) { return fnv_bytes(reinterpret_cast<const uint8_t *>(v.data()), 4 * v.size()); }
} // namespace

int main(int argc, char **argv)
{
    const int64_t n = argc > 1 ? std::atoll(argv[1]) : 4096;
    const int spp_n = argc > 2 ? std::atoi(argv[2]) : 4;
    const int spp = spp_n * spp_n;
    try {
        rlsb::Device dev(0);
        rlsb::Planes frame(dev, n, 9);
        rlsb::check(rls_gen_frame(dev.ctx(), kSeed, 0, n, frame.vec3(0), frame.vec3(3), frame.vec3(6)));
        rls_skin_closure kc = {};
        kc.wo = frame.cvec3(0); kc.N = frame.cvec3(3); kc.T = frame.cvec3(6);
        kc.sss_color = rlsb::ParamRGB(0.8f, 0.5f, 0.3f).c();
        kc.sss_weight = rls_param{nullptr, 0.9f};
        kc.sss_dist_multiplier = rls_param{nullptr, 0.5f};
        kc.sss_scatter_dist[0] = rls_param{nullptr, 0.1f};
        kc.sss_scatter_dist[1] = rls_param{nullptr, 0.2f};
        kc.sss_scatter_dist[2] = rls_param{nullptr, 0.4f};
        kc.specular_color = rlsb::ParamRGB(0.9f, 0.95f, 1.0f).c();
        kc.specular_weight = rls_param{nullptr, 0.6f};
        kc.specular_roughness = rls_param{nullptr, 0.5f};
        kc.specular_ior = rls_param{nullptr, 1.44f};
        kc.sheen_color = rlsb::ParamRGB(1.0f, 0.9f, 0.8f).c();
        kc.sheen_weight = rls_param{nullptr, 0.3f};
        kc.sheen_roughness = rls_param{nullptr, 0.35f};
        kc.sheen_ior = rls_param{nullptr, 1.3f};
        rls_sphere_light lights[2] = {};
        const float centers[2][3] = {{-4.0f, 2.0f, 3.0f}, {6.0f, 1.0f, 2.0f}};
        const float radiances[2][3] = {{3.0f, 2.0f, 1.0f}, {1.0f, 4.0f, 2.0f}};
        for (int l = 0; l < 2; l++) {
            for (int k = 0; k < 3; k++) { lights[l].center[k] = centers[l][k]; lights[l].radiance[k] = radiances[l][k]; }
            lights[l].radius = 1.0f;
            lights[l].mis_mode = RLS_MIS_BOTH;
        }
        // one glossy bounce is allowed (GI_glossy_depth 1)
        const rls_gi_depths depths = {4, 1, 1, 2};
        rlsb::Planes P(dev, std::vector<float>((size_t)(3 * n), 0.0f), 3);
        std::vector<float> nrm((size_t)(3 * n));
        for (int k = 0; k < 3; k++)
            rlsb::check(rls_copy_to_host(dev.ctx(), &nrm[(size_t)(k * n)], (&kc.N.x)[k], sizeof(float) * (size_t)n));
        const float env[3] = {0.7f, 0.8f, 0.9f};

        // one wave of m points under `state`: emit, the renderer's part, resolve, one JSON member
        auto shade = [&](const char *name, int64_t m, const rls_ray_state &state, uint64_t first_index, rlsb::SkinBounceQueues &q) {
            const int64_t cap = m * spp;
            rlsb::emitBounce(dev, kc, P, lights, 2, m, spp_n, kSeed, state, depths, q, first_index);
            const rlsb::SkinNodeQueues &nq = q.node();
            const int64_t rays[5] = {nq.sheenShadow()->count(), nq.specularShadow()->count(), nq.sheenGlossy().count(),
                                     nq.specularGlossy().count(), q.diffuseShadow()->count()};
            // nothing occludes a light; every glossy ray sees the same radiance
            rlsb::Planes vis(dev, std::vector<float>((size_t)(3 * nq.sheenShadow()->c().capacity), 1.0f), 3);
            std::vector<float> L((size_t)(3 * cap));
            for (int k = 0; k < 3; k++) std::fill(L.begin() + (size_t)(k * cap), L.begin() + (size_t)((k + 1) * cap), env[k]);
            rlsb::Planes radiance(dev, L, 3);
            // the probe walk: the one hit of a probe ray on its point's tangent plane, E = 1 / pi
            const rls_probe_queue &pq = nq.probes().c();
            std::vector<float> org((size_t)(3 * cap)), dir((size_t)(3 * cap)), md((size_t)cap);
            for (int k = 0; k < 3; k++) {
                rlsb::check(rls_copy_to_host(dev.ctx(), &org[(size_t)(k * cap)], (&pq.origin.x)[k], sizeof(float) * (size_t)cap));
                rlsb::check(rls_copy_to_host(dev.ctx(), &dir[(size_t)(k * cap)], (&pq.dir.x)[k], sizeof(float) * (size_t)cap));
            }
            rlsb::check(rls_copy_to_host(dev.ctx(), md.data(), pq.maxdist, sizeof(float) * (size_t)cap));
            std::vector<uint8_t> cnt((size_t)cap, 0);
            std::vector<float> hits((size_t)(9 * cap), 0.0f);             // P, N, irradiance: 3 planes each, one hit slot
            int64_t found = 0;
            for (int64_t j = 0; j < cap; j++) {
                const int64_t i = j / spp;
                float dn = 0.0f, on = 0.0f;
                for (int k = 0; k < 3; k++) {
                    dn += nrm[(size_t)(k * n + i)] * dir[(size_t)(k * cap + j)];
                    on += nrm[(size_t)(k * n + i)] * org[(size_t)(k * cap + j)];
                }
                const float t = dn != 0.0f ? -on / dn : 0.0f;
                if (!(t > 0.0f && t <= md[(size_t)j])) continue;
                cnt[(size_t)j] = 1;
                found++;
                for (int k = 0; k < 3; k++) {
                    hits[(size_t)(k * cap + j)] = org[(size_t)(k * cap + j)] + dir[(size_t)(k * cap + j)] * t;
                    hits[(size_t)((3 + k) * cap + j)] = nrm[(size_t)(k * n + i)];
                    hits[(size_t)((6 + k) * cap + j)] = 0.318309886f;
                }
            }
            rlsb::Planes hp(dev, hits, 9);
            void *dcnt = nullptr;
            rlsb::check(rls_device_alloc(dev.ctx(), (size_t)(cap > 0 ? cap : 1), &dcnt));
            rlsb::check(rls_copy_to_device(dev.ctx(), dcnt, cnt.data(), (size_t)cap));
            rls_probe_hits h = {};
            h.max_hits = 1; h.stride = cap; h.count = static_cast<const uint8_t *>(dcnt);
            h.P = hp.cvec3(0); h.N = hp.cvec3(3);
            h.irradiance = rls_crgb{hp.plane(6), hp.plane(7), hp.plane(8)};
            rlsb::Planes aovs(dev, m, 9), out(dev, m, 3);
            rlsb::resolveBounce(dev, kc, P, lights, 2, state, depths, q, vis, vis, radiance, radiance, h, vis, true, false, aovs, &out);
            std::vector<float> ra = aovs.download(), ro = out.download(), sc = nq.scalars().download();
            rls_device_free(dev.ctx(), dcnt);
            double mean = 0.0;
            for (float v : ro) mean += v;
            std::printf(", \"%s\": {\"points\": %lld, \"rays\": [%lld, %lld, %lld, %lld, %lld], \"hits\": %lld, \"aovs\": \"%016llx\", "
                        "\"out\": \"%016llx\", \"scalars\": \"%016llx\", \"mean_out\": %.9g}", name, (long long)m,
                        (long long)rays[0], (long long)rays[1], (long long)rays[2], (long long)rays[3], (long long)rays[4],
                        (long long)found, (unsigned long long)fnv(ra), (unsigned long long)fnv(ro), (unsigned long long)fnv(sc),
                        ro.empty() ? 0.0 : mean / (double)ro.size());
        };
        std::printf("{\"points\": %lld, \"spp_n\": %d", (long long)n, spp_n);

        // 1. the camera wave
        rlsb::RayState camera = rlsb::RayState::camera(dev, n);
        rlsb::SkinBounceQueues cq(dev, n, 2, spp_n);
        shade("camera", n, camera.c(), 0, cq);

        // 2. the state of the specular lobe's glossy rays' hits
        const int64_t glossy = cq.node().specularGlossy().count();
        rlsb::RayState hits(dev, glossy);
        rlsb::advanceState(dev, glossy, cq.node().specularGlossy().c().point, camera.c(), RLS_RT_GLOSSY, hits);
        const std::vector<uint8_t> all = hits.download();
        std::printf(", \"advanced\": {\"rays\": %lld, \"state\": \"%016llx\"}", (long long)glossy,
                    (unsigned long long)fnv_bytes(all.data(), all.size()));

        // 3. stand-in hits for the first m rays: hit k has the surface of shading point k, under the advanced planes' first m
        // entries, gathered into a state of their own
        const int64_t m = std::min(glossy, n);
        std::vector<uint8_t> first((size_t)(5 * m));
        for (int p = 0; p < 5; p++)
            std::copy(all.begin() + (size_t)(p * glossy), all.begin() + (size_t)(p * glossy + m), first.begin() + (size_t)(p * m));
        rlsb::RayState secondary(dev, first);
        rlsb::SkinBounceQueues sq(dev, m, 2, spp_n);
        shade("glossy_hits", m, secondary.c(), (uint64_t)n, sq);
        std::printf("}\n");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "example_trace_skin_bounce: %s\n", e.what());
        return 1;
    }
    return 0;
}
