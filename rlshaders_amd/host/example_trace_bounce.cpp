// example_trace_bounce.cpp -- a second bounce through the caller's tracer from C++ (rls_trace.hpp: RayState, emitBounce,
// resolveBounce, advanceState).  The camera hits of an rlGgx surface are shaded under an all-camera state: every queue of the
// node is emitted, "traced" against an analytic sky with no occluders, and resolved.  The state is then advanced along the
// glossy queue -- each ray's hit is a glossy secondary point one bounce deeper -- and the first min(rays, points) of those rays
// are given stand-in hits: hit k has the surface of shading point k.  They are shaded as rlGgx and as rlDisney points under
// the advanced state: no indirect rays leave a secondary point, rlGgx's refraction follows the depth limits, rlDisney's
// direct terms take the node's indirect scales.
//
//   example_trace_bounce [points] [spp_n]
// prints one JSON line: ray counts and checksums (FNV-1a over the bits of the resolved planes, and over the advanced state's
// bytes), which tests/test_gpu_trace_bounce_host_cpp.py compares with the Python path (rlshaders_amd/trace.py) on the same inputs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    const int64_t cap = n * spp_n * spp_n;
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
        dc.wo = c.wo; dc.N = c.N; dc.T = c.T;
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
        // one glossy bounce is allowed (GI_glossy_depth 1), refraction is traced to depth 2
        const rls_gi_depths depths = {4, 1, 1, 2};
        rlsb::Planes P(dev, std::vector<float>((size_t)(3 * n), 0.0f), 3);

        // the renderer's tracer: nothing occludes a light; every other ray escapes to a sky brighter towards +z, warm-tinted
        auto unoccluded = [&](const rlsb::ShadowQueue &sq, int64_t &count) {
            count = sq.count();
            return rlsb::Planes(dev, std::vector<float>((size_t)(3 * sq.c().capacity), 1.0f), 3);
        };
        auto lit = [&](const rlsb::RayQueue &q, int64_t &count) {
            count = q.count();
            std::vector<float> dz((size_t)count), L((size_t)(3 * cap), 0.0f);
            rlsb::check(rls_copy_to_host(dev.ctx(), dz.data(), q.c().dir.z, sizeof(float) * dz.size()));
            for (size_t k = 0; k < dz.size(); k++) {
                const float up = 0.25f + 0.75f * std::max(dz[k], 0.0f);
                L[k] = up; L[(size_t)cap + k] = up * 0.875f; L[(size_t)(2 * cap) + k] = up * 0.75f;
            }
            return rlsb::Planes(dev, L, 3);
        };
        auto report = [&](const char *name, int64_t points, const int64_t *rays, int nq, const rlsb::Planes &aovs,
                          const rlsb::Planes &out) {
            std::vector<float> ra = aovs.download(), ro = out.download();
            double mean = 0.0;
            for (float v : ro) mean += v;
            std::printf(", \"%s\": {\"points\": %lld, \"rays\": [", name, (long long)points);
            for (int k = 0; k < nq; k++) std::printf("%s%lld", k ? ", " : "", (long long)rays[k]);
            std::printf("], \"aovs\": \"%016llx\", \"out\": \"%016llx\", \"mean_out\": %.9g}", (unsigned long long)fnv(ra),
                        (unsigned long long)fnv(ro), ro.empty() ? 0.0 : mean / (double)ro.size());
        };
        std::printf("{\"points\": %lld, \"spp_n\": %d", (long long)n, spp_n);

        // 1. the camera hits
        rlsb::RayState camera = rlsb::RayState::camera(dev, n);
        rlsb::GgxNodeQueues nq(dev, n, 2, spp_n);
        rlsb::emitBounce(dev, c, sh, P, lights, 2, n, spp_n, kSeed, camera.c(), depths, nq);
        int64_t rays[4];
        {
            rlsb::Planes vis = unoccluded(*nq.shadow(), rays[0]);
            rlsb::Planes Lg = lit(nq.glossy(), rays[1]), Lt = lit(nq.refract(), rays[2]), Ld = lit(nq.diffuse(), rays[3]);
            rlsb::Planes aovs(dev, n, 15), out(dev, n, 3);
            rlsb::resolveBounce(dev, c, sh, lights, 2, camera.c(), depths, nq, vis, Lg, Lt, Ld, aovs, &out);
            report("camera", n, rays, 4, aovs, out);
        }

        // 2. the state of the glossy rays' hits
        const int64_t glossy = rays[1];
        rlsb::RayState hits(dev, glossy);
        rlsb::advanceState(dev, glossy, nq.glossy().c().point, camera.c(), RLS_RT_GLOSSY, hits);
        {
            const std::vector<uint8_t> h = hits.download();
            std::printf(", \"advanced\": {\"rays\": %lld, \"state\": \"%016llx\"}", (long long)glossy,
                        (unsigned long long)fnv_bytes(h.data(), h.size()));
        }

        // 3. stand-in hits for the first m rays: hit k has the surface of shading point k.  The state of a batch of m < rays
        // points: the advanced planes' first m entries, gathered into a state of their own
        const int64_t m = std::min(glossy, n);
        std::vector<uint8_t> all = hits.download(), first((size_t)(5 * m));
        for (int p = 0; p < 5; p++)
            std::copy(all.begin() + (size_t)(p * glossy), all.begin() + (size_t)(p * glossy + m), first.begin() + (size_t)(p * m));
        rlsb::RayState secondary(dev, first);
        {
            rlsb::GgxNodeQueues sq(dev, m, 2, spp_n);
            rlsb::emitBounce(dev, c, sh, P, lights, 2, m, spp_n, kSeed, secondary.c(), depths, sq, (uint64_t)n);
            rlsb::Planes vis = unoccluded(*sq.shadow(), rays[0]);
            rlsb::Planes Lg = lit(sq.glossy(), rays[1]), Lt = lit(sq.refract(), rays[2]), Ld = lit(sq.diffuse(), rays[3]);
            rlsb::Planes aovs(dev, m, 15), out(dev, m, 3);
            rlsb::resolveBounce(dev, c, sh, lights, 2, secondary.c(), depths, sq, vis, Lg, Lt, Ld, aovs, &out);
            report("glossy_hits", m, rays, 4, aovs, out);
        }
        {
            rlsb::DisneyNodeQueues sq(dev, m, 2, spp_n);
            rlsb::emitBounce(dev, dc, P, lights, 2, m, spp_n, kSeed, secondary.c(), depths, sq, (uint64_t)n);
            rlsb::Planes vis = unoccluded(*sq.shadow(), rays[0]);
            rlsb::Planes Ld = lit(sq.diffuse(), rays[1]), Ls = lit(sq.specular(), rays[2]);
            rlsb::Planes aovs(dev, m, 12), out(dev, m, 3);
            const rls_param kd = {nullptr, 0.5f}, ks = {nullptr, 0.25f};      // indirectDiffuseScale, indirectSpecularScale
            rlsb::resolveBounce(dev, dc, kd, ks, lights, 2, secondary.c(), depths, sq, vis, Ld, Ls, aovs, &out);
            report("disney_glossy_hits", m, rays, 3, aovs, out);
        }
        std::printf("}\n");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "example_trace_bounce: %s\n", e.what());
        return 1;
    }
    return 0;
}
