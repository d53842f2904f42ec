// example_trace.cpp -- the caller-traced rlGgx, rlDisney and rlSss integrators from C++ (rls_trace.hpp): emit
// integrateGlossy's and integrateRefract's sample rays and those of rlDisney's two lobes, "trace" them against an analytic
// sky on the host, resolve; emit rlSss's probe rays, walk them through each point's tangent plane on the host, resolve --
// once with the hits' irradiance formed by hand, once lit through the library (emitHits / resolveHits);
// emit the shadow rays of both nodes' light loops under two lights, shadow the second light with a half-space, resolve;
// emit every queue of the two whole nodes, shadow the second light with the same half-space and light the ray queues with the
// sky, resolve the AOVs in one call; emit the five queues of the rlSkin node, leave its lights unoccluded, light its glossy
// rays uniformly, walk its probe rays through each point's tangent plane, resolve the AOVs in one call.
//
//   example_trace [points] [spp_n]
// prints one JSON line: the ray counts and a checksum (FNV-1a over the bits of the resolved planes) per integrator, which
// tests/test_gpu_trace_host_cpp.py (the lit hits: tests/test_gpu_trace_hits_host_cpp.py; the light loops: tests/test_gpu_trace_lights_host_cpp.py; the whole nodes: tests/test_gpu_trace_shade_host_cpp.py, tests/test_gpu_trace_skin_host_cpp.py) compares with the Python path (rlshaders_amd/trace.py) on the same inputs.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rls_trace.hpp"

namespace {
constexpr uint32_t kSeed = 1234;

// the renderer's tracer, in a few lines: every ray escapes to a sky brighter towards +z, warm-tinted.  dz: the rays'
// z components; L: 3 planes of cap floats
void sky(const std::vector<float> &dz, int64_t cap, std::vector<float> &L)
{
    for (size_t k = 0; k < dz.size(); k++) {
        const float up = 0.25f + 0.75f * std::max(dz[k], 0.0f);
        L[k] = up;
        L[(size_t)cap + k] = up * 0.875f;
        L[(size_t)(2 * cap) + k] = up * 0.75f;
    }
}

uint64_t fnv(const std::vector<float> &v)
{
    uint64_t h = 1469598103934665603ull;
    for (float f : v) {
        uint32_t b;
        std::memcpy(&b, &f, 4);
        for (int k = 0; k < 4; k++) { h ^= (b >> (8 * k)) & 0xFFu; h *= 1099511628211ull; }
    }
    return h;
}
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
        // an rlDisney closure on the same frame, uniform parameters (tests/test_gpu_trace_disney_host_cpp.py: the same)
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

        std::printf("{");
        const rlsb::RayQueue::Kind kinds[4] = {rlsb::RayQueue::Glossy, rlsb::RayQueue::Refract, rlsb::RayQueue::DisneyDiffuse,
                                               rlsb::RayQueue::DisneyGlossy};
        const char *names[4] = {"glossy", "refract", "disney_diffuse", "disney_glossy"};
        for (int j = 0; j < 4; j++) {
            rlsb::RayQueue q(dev, n, spp_n, kinds[j]);
            rlsb::Planes side(dev, n, 1), out(dev, n, 3), radiance(dev, cap, 3);
            if (j == 0) rlsb::emitGlossy(dev, c, n, spp_n, kSeed, q, side.plane(0));
            else if (j == 1) rlsb::emitRefract(dev, c, n, spp_n, kSeed, q, side.plane(0));
            else rlsb::emitDisney(dev, dc, j == 2 ? RLS_RAY_DIFFUSE : RLS_RAY_GLOSSY, n, spp_n, kSeed, q, side.plane(0));
            const int64_t count = q.count();
            std::vector<float> dz((size_t)count), L((size_t)(3 * cap), 0.0f);
            rlsb::check(rls_copy_to_host(dev.ctx(), dz.data(), q.c().dir.z, sizeof(float) * dz.size()));
            sky(dz, cap, L);
            radiance.upload(L);
            if (j == 1) rlsb::resolveRefract(dev, q, radiance, out);
            else rlsb::resolveGlossy(dev, q, radiance, out);
            std::vector<float> res = out.download();
            double mean = 0.0;
            for (float v : res) mean += v;
            std::printf("%s\"%s\": {\"rays\": %lld, \"checksum\": \"%016llx\", \"mean\": %.9g}", j ? ", " : "",
                        names[j], (long long)count, (unsigned long long)fnv(res), mean / (double)res.size());
        }
        {
            // rlSss on the same frame: each shading point at the origin of its own tangent plane (normal N), lit from N
            // itself, E = 1 / pi.  The renderer's probe walk: the one hit of a ray on that plane, 0 < t <= maxdist.
            rls_sss_closure sc = {};
            sc.sss_color = rlsb::ParamRGB(0.8f, 0.5f, 0.3f).c();
            sc.sss_dist_multiplier = rls_param{nullptr, 1.0f};
            sc.sss_scatter_dist[0] = rls_param{nullptr, 0.05f};
            sc.sss_scatter_dist[1] = rls_param{nullptr, 0.1f};
            sc.sss_scatter_dist[2] = rls_param{nullptr, 0.2f};
            sc.N = c.N; sc.T = c.T; sc.has_dPdu = 1;
            rlsb::Planes P(dev, std::vector<float>((size_t)(3 * n), 0.0f), 3), out(dev, n, 3), depth(dev, n, 1);
            rlsb::ProbeQueue pq(dev, n, spp_n);
            rlsb::emitProbes(dev, sc, P, n, spp_n, kSeed, pq);
            const int spp = spp_n * spp_n;
            std::vector<float> org((size_t)(3 * cap)), dir((size_t)(3 * cap)), md((size_t)cap), nrm((size_t)(3 * n));
            for (int k = 0; k < 3; k++) {
                rlsb::check(rls_copy_to_host(dev.ctx(), &org[(size_t)(k * cap)], (&pq.c().origin.x)[k], sizeof(float) * (size_t)cap));
                rlsb::check(rls_copy_to_host(dev.ctx(), &dir[(size_t)(k * cap)], (&pq.c().dir.x)[k], sizeof(float) * (size_t)cap));
                rlsb::check(rls_copy_to_host(dev.ctx(), &nrm[(size_t)(k * n)], (&c.N.x)[k], sizeof(float) * (size_t)n));
            }
            rlsb::check(rls_copy_to_host(dev.ctx(), md.data(), pq.c().maxdist, sizeof(float) * (size_t)cap));
            std::vector<uint8_t> cnt((size_t)cap, 0);
            std::vector<float> hits((size_t)(9 * cap), 0.0f);             // P, N, irradiance: 3 planes each, one hit slot
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
                for (int k = 0; k < 3; k++) {
                    hits[(size_t)(k * cap + j)] = org[(size_t)(k * cap + j)] + dir[(size_t)(k * cap + j)] * t;
                    hits[(size_t)((3 + k) * cap + j)] = nrm[(size_t)(k * n + i)];
                    hits[(size_t)((6 + k) * cap + j)] = 0.318309886f;
                }
            }
            rlsb::Planes hp(dev, hits, 9);
            void *dcnt = nullptr;
            rlsb::check(rls_device_alloc(dev.ctx(), (size_t)cap, &dcnt));
            rlsb::check(rls_copy_to_device(dev.ctx(), dcnt, cnt.data(), (size_t)cap));
            rls_probe_hits h = {};
            h.max_hits = 1; h.stride = cap; h.count = static_cast<const uint8_t *>(dcnt);
            h.P = hp.cvec3(0); h.N = hp.cvec3(3);
            h.irradiance = rls_crgb{hp.plane(6), hp.plane(7), hp.plane(8)};
            rlsb::resolveScatter(dev, sc, P, pq, h, true, false, out, depth.plane(0));
            std::vector<float> res = out.download(), dres = depth.download();
            double mean = 0.0, mdepth = 0.0;
            for (float v : res) mean += v;
            for (float v : dres) mdepth += v;
            std::printf(", \"sss\": {\"rays\": %lld, \"checksum\": \"%016llx\", \"mean\": %.9g, \"mean_depth\": %.9g}",
                        (long long)pq.count(), (unsigned long long)fnv(res), mean / (double)res.size(), mdepth / (double)n);

            // The same hits shaded through the library instead of by hand (shadeProbeSample's light loop and diffuse ray):
            // one spherical light, unoccluded (visibility 1), the diffuse rays lit by the sky; E goes where the hits'
            // irradiance was, and the scatter resolve runs again on it.
            rls_sphere_light light = {};
            light.center[0] = 1.5f; light.center[1] = 2.5f; light.center[2] = 3.5f;
            light.radius = 1.25f; light.mis_mode = RLS_MIS_BOTH;
            light.radiance[0] = 3.0f; light.radiance[1] = 2.0f; light.radiance[2] = 0.5f;
            const int hit_spp_n = 2;
            rlsb::HitQueues hq(dev, n, spp_n, 1, cap, 1, hit_spp_n, true);
            rlsb::emitHits(dev, sc, P, pq, h, nullptr, true, &light, 1, kSeed, hq);
            const int64_t listed = hq.listed(), shadow = hq.shadowCount(), diffuse = hq.diffuseCount();
            const int64_t scap = hq.c().shadow.capacity;
            rlsb::Planes vis(dev, std::vector<float>((size_t)(3 * scap), 1.0f), 3), Ld(dev, cap, 3), E(dev, cap, 3);
            std::vector<float> ddz((size_t)diffuse), L((size_t)(3 * cap), 0.0f);
            rlsb::check(rls_copy_to_host(dev.ctx(), ddz.data(), hq.c().diffuse.dir.z, sizeof(float) * ddz.size()));
            sky(ddz, cap, L);
            Ld.upload(L);
            rlsb::resolveHits(dev, h, &light, 1, hq, vis, &Ld, E);
            rls_probe_hits lit = h;
            lit.irradiance = rls_crgb{E.plane(0), E.plane(1), E.plane(2)};
            rlsb::resolveScatter(dev, sc, P, pq, lit, true, false, out, nullptr);
            std::vector<float> eres = E.download(), lres = out.download();
            double emean = 0.0, lmean = 0.0;
            for (float v : eres) emean += v;
            for (float v : lres) lmean += v;
            std::printf(", \"sss_hits\": {\"hits\": %lld, \"shadow_rays\": %lld, \"diffuse_rays\": %lld, \"E_checksum\": "
                        "\"%016llx\", \"E_mean\": %.9g, \"checksum\": \"%016llx\", \"mean\": %.9g}",
                        (long long)listed, (long long)shadow, (long long)diffuse, (unsigned long long)fnv(eres),
                        emean / (double)eres.size(), (unsigned long long)fnv(lres), lmean / (double)lres.size());
            rls_device_free(dev.ctx(), dcnt);
        }
        {
            // The light loops of rlGgx and rlDisney on the same frame, every shading point at the origin: two spherical
            // lights, and a wall -- the half-space x > 3 -- in front of the second one.  The renderer's shadow tracer: a ray
            // from P = 0 along dir is blocked where it enters the half-space before maxdist.
            rls_sphere_light lights[2] = {};
            const float centers[2][3] = {{-4.0f, 2.0f, 3.0f}, {6.0f, 1.0f, 2.0f}};
            const float radiances[2][3] = {{3.0f, 2.0f, 1.0f}, {1.0f, 4.0f, 2.0f}};
            for (int l = 0; l < 2; l++) {
                for (int k = 0; k < 3; k++) { lights[l].center[k] = centers[l][k]; lights[l].radiance[k] = radiances[l][k]; }
                lights[l].radius = 1.0f;
                lights[l].mis_mode = RLS_MIS_BOTH;
            }
            rls_ggx_shader sh = {};
            sh.KdColor = rlsb::ParamRGB(0.7f, 0.5f, 0.2f).c();
            sh.Kd = rls_param{nullptr, 0.8f};
            sh.diffuseRoughness = rls_param{nullptr, 0.3f};
            sh.Ks = rls_param{nullptr, 0.6f};
            sh.KtColor = rlsb::ParamRGB(1.0f, 1.0f, 1.0f).c();
            rlsb::Planes P(dev, std::vector<float>((size_t)(3 * n), 0.0f), 3);
            const char *lnames[2] = {"ggx_lights", "disney_lights"};
            for (int j = 0; j < 2; j++) {
                rlsb::ShadowQueue sq(dev, n, 2, spp_n, j == 0 ? rlsb::ShadowQueue::Ggx : rlsb::ShadowQueue::Disney);
                if (j == 0) rlsb::emitDirect(dev, c, sh, P, lights, 2, n, spp_n, kSeed, sq);
                else rlsb::emitDirect(dev, dc, P, lights, 2, n, spp_n, kSeed, sq);
                const int64_t count = sq.count(), scap = sq.c().capacity;
                std::vector<float> dx((size_t)count), md((size_t)count), vis((size_t)(3 * scap), 0.0f);
                rlsb::check(rls_copy_to_host(dev.ctx(), dx.data(), sq.c().dir.x, sizeof(float) * dx.size()));
                rlsb::check(rls_copy_to_host(dev.ctx(), md.data(), sq.c().maxdist, sizeof(float) * md.size()));
                int64_t blocked = 0;
                for (int64_t k = 0; k < count; k++) {
                    const bool hit = md[(size_t)k] * dx[(size_t)k] > 3.0f;
                    blocked += hit ? 1 : 0;
                    for (int ch = 0; ch < 3; ch++) vis[(size_t)(ch * scap + k)] = hit ? 0.0f : 1.0f;
                }
                rlsb::Planes visibility(dev, vis, 3), dd(dev, n, 3), ds(dev, n, 3);
                if (j == 0) rlsb::resolveDirect(dev, c, sh, lights, 2, sq, visibility, dd, ds);
                else rlsb::resolveDirect(dev, lights, 2, sq, visibility, dd, ds);
                std::vector<float> rd = dd.download(), rs = ds.download();
                double md_ = 0.0, ms_ = 0.0;
                for (float v : rd) md_ += v;
                for (float v : rs) ms_ += v;
                std::printf(", \"%s\": {\"rays\": %lld, \"blocked\": %lld, \"direct_diffuse\": \"%016llx\", "
                            "\"direct_specular\": \"%016llx\", \"mean_diffuse\": %.9g, \"mean_specular\": %.9g}",
                            lnames[j], (long long)count, (long long)blocked, (unsigned long long)fnv(rd),
                            (unsigned long long)fnv(rs), md_ / (double)rd.size(), ms_ / (double)rs.size());
            }
        }
        {
            // The whole nodes on the same frame, every shading point at the origin, the two lights and the wall x > 3 of the
            // light loops above: the shadow queue is traced against the wall, every ray queue sees the sky.  rlGgx with
            // transmission (KtColor * Kt), its refraction traced.
            rls_sphere_light lights[2] = {};
            const float centers[2][3] = {{-4.0f, 2.0f, 3.0f}, {6.0f, 1.0f, 2.0f}};
            const float radiances[2][3] = {{3.0f, 2.0f, 1.0f}, {1.0f, 4.0f, 2.0f}};
            for (int l = 0; l < 2; l++) {
                for (int k = 0; k < 3; k++) { lights[l].center[k] = centers[l][k]; lights[l].radiance[k] = radiances[l][k]; }
                lights[l].radius = 1.0f;
                lights[l].mis_mode = RLS_MIS_BOTH;
            }
            rls_ggx_shader sh = {};
            sh.KdColor = rlsb::ParamRGB(0.7f, 0.5f, 0.2f).c();
            sh.Kd = rls_param{nullptr, 0.8f};
            sh.diffuseRoughness = rls_param{nullptr, 0.3f};
            sh.Ks = rls_param{nullptr, 0.6f};
            sh.KtColor = rlsb::ParamRGB(0.2f, 0.9f, 0.7f).c();
            sh.Kt = rls_param{nullptr, 0.5f};
            rlsb::Planes P(dev, std::vector<float>((size_t)(3 * n), 0.0f), 3);
            // the shadow tracer of the light loops' section; -> the visibility planes, the rays and the blocked rays
            auto shadowed = [&](const rlsb::ShadowQueue &sq, int64_t &count, int64_t &blocked) {
                count = sq.count();
                const int64_t scap = sq.c().capacity;
                std::vector<float> dx((size_t)count), md((size_t)count), vis((size_t)(3 * scap), 0.0f);
                rlsb::check(rls_copy_to_host(dev.ctx(), dx.data(), sq.c().dir.x, sizeof(float) * dx.size()));
                rlsb::check(rls_copy_to_host(dev.ctx(), md.data(), sq.c().maxdist, sizeof(float) * md.size()));
                blocked = 0;
                for (int64_t k = 0; k < count; k++) {
                    const bool hit = md[(size_t)k] * dx[(size_t)k] > 3.0f;
                    blocked += hit ? 1 : 0;
                    for (int ch = 0; ch < 3; ch++) vis[(size_t)(ch * scap + k)] = hit ? 0.0f : 1.0f;
                }
                return rlsb::Planes(dev, vis, 3);
            };
            // the sky along a ray queue's rays; -> the radiance planes and the rays
            auto lit = [&](const rlsb::RayQueue &q, int64_t &count) {
                count = q.count();
                std::vector<float> dz((size_t)count), L((size_t)(3 * cap), 0.0f);
                rlsb::check(rls_copy_to_host(dev.ctx(), dz.data(), q.c().dir.z, sizeof(float) * dz.size()));
                sky(dz, cap, L);
                return rlsb::Planes(dev, L, 3);
            };
            auto report = [&](const char *name, const int64_t *rays, int nq, int64_t blocked, const rlsb::Planes &aovs,
                              const rlsb::Planes &out) {
                std::vector<float> ra = aovs.download(), ro = out.download();
                double mean = 0.0;
                for (float v : ro) mean += v;
                std::printf(", \"%s\": {\"rays\": [", name);
                for (int k = 0; k < nq; k++) std::printf("%s%lld", k ? ", " : "", (long long)rays[k]);
                std::printf("], \"blocked\": %lld, \"aovs\": \"%016llx\", \"out\": \"%016llx\", \"mean_out\": %.9g}",
                            (long long)blocked, (unsigned long long)fnv(ra), (unsigned long long)fnv(ro), mean / (double)ro.size());
            };
            {
                rlsb::GgxNodeQueues nq(dev, n, 2, spp_n);
                rlsb::emitNode(dev, c, sh, P, lights, 2, true, n, spp_n, kSeed, nq);
                int64_t rays[4], blocked = 0;
                rlsb::Planes vis = shadowed(*nq.shadow(), rays[0], blocked);
                rlsb::Planes Lg = lit(nq.glossy(), rays[1]), Lt = lit(nq.refract(), rays[2]), Ld = lit(nq.diffuse(), rays[3]);
                rlsb::Planes aovs(dev, n, 15), out(dev, n, 3);
                rlsb::resolveNode(dev, c, sh, lights, 2, true, nq, vis, Lg, Lt, Ld, aovs, &out);
                report("ggx_node", rays, 4, blocked, aovs, out);
            }
            {
                rlsb::DisneyNodeQueues nq(dev, n, 2, spp_n);
                rlsb::emitNode(dev, dc, P, lights, 2, n, spp_n, kSeed, nq);
                int64_t rays[3], blocked = 0;
                rlsb::Planes vis = shadowed(*nq.shadow(), rays[0], blocked);
                rlsb::Planes Ld = lit(nq.diffuse(), rays[1]), Ls = lit(nq.specular(), rays[2]);
                rlsb::Planes aovs(dev, n, 12), out(dev, n, 3);
                rlsb::resolveNode(dev, lights, 2, nq, vis, Ld, Ls, aovs, &out);
                report("disney_node", rays, 3, blocked, aovs, out);
            }
        }
        {
            // The rlSkin node on the same frame, every shading point at the origin of its own tangent plane, the two lights of
            // the sections above unoccluded (visibility 1), a uniform radiance on every glossy ray, and the probe walk of the
            // rlSss section: the one hit of a probe ray on the point's tangent plane, E = 1 / pi.
            rls_sphere_light lights[2] = {};
            const float centers[2][3] = {{-4.0f, 2.0f, 3.0f}, {6.0f, 1.0f, 2.0f}};
            const float radiances[2][3] = {{3.0f, 2.0f, 1.0f}, {1.0f, 4.0f, 2.0f}};
            for (int l = 0; l < 2; l++) {
                for (int k = 0; k < 3; k++) { lights[l].center[k] = centers[l][k]; lights[l].radiance[k] = radiances[l][k]; }
                lights[l].radius = 1.0f;
                lights[l].mis_mode = RLS_MIS_BOTH;
            }
            rls_skin_closure kc = {};
            kc.wo = c.wo; kc.N = c.N; kc.T = c.T;
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
            rlsb::Planes P(dev, std::vector<float>((size_t)(3 * n), 0.0f), 3);
            rlsb::SkinNodeQueues nq(dev, n, 2, spp_n);
            rlsb::emitNode(dev, kc, P, lights, 2, n, spp_n, kSeed, nq);
            const int64_t rays[4] = {nq.sheenShadow()->count(), nq.specularShadow()->count(), nq.sheenGlossy().count(),
                                     nq.specularGlossy().count()};
            const int64_t scap = nq.sheenShadow()->c().capacity;
            rlsb::Planes vis(dev, std::vector<float>((size_t)(3 * scap), 1.0f), 3);
            const float env[3] = {0.7f, 0.8f, 0.9f};
            std::vector<float> L((size_t)(3 * cap));
            for (int k = 0; k < 3; k++) std::fill(L.begin() + (size_t)(k * cap), L.begin() + (size_t)((k + 1) * cap), env[k]);
            rlsb::Planes radiance(dev, L, 3);
            const rls_probe_queue &pq = nq.probes().c();
            const int spp = spp_n * spp_n;
            std::vector<float> org((size_t)(3 * cap)), dir((size_t)(3 * cap)), md((size_t)cap), nrm((size_t)(3 * n));
            for (int k = 0; k < 3; k++) {
                rlsb::check(rls_copy_to_host(dev.ctx(), &org[(size_t)(k * cap)], (&pq.origin.x)[k], sizeof(float) * (size_t)cap));
                rlsb::check(rls_copy_to_host(dev.ctx(), &dir[(size_t)(k * cap)], (&pq.dir.x)[k], sizeof(float) * (size_t)cap));
                rlsb::check(rls_copy_to_host(dev.ctx(), &nrm[(size_t)(k * n)], (&c.N.x)[k], sizeof(float) * (size_t)n));
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
            rlsb::check(rls_device_alloc(dev.ctx(), (size_t)cap, &dcnt));
            rlsb::check(rls_copy_to_device(dev.ctx(), dcnt, cnt.data(), (size_t)cap));
            rls_probe_hits h = {};
            h.max_hits = 1; h.stride = cap; h.count = static_cast<const uint8_t *>(dcnt);
            h.P = hp.cvec3(0); h.N = hp.cvec3(3);
            h.irradiance = rls_crgb{hp.plane(6), hp.plane(7), hp.plane(8)};
            rlsb::Planes aovs(dev, n, 9), out(dev, n, 3);
            rlsb::resolveNode(dev, kc, P, lights, 2, nq, vis, vis, radiance, radiance, h, true, false, aovs, &out);
            std::vector<float> ra = aovs.download(), ro = out.download(), sc = nq.scalars().download();
            rls_device_free(dev.ctx(), dcnt);
            double mean = 0.0;
            for (float v : ro) mean += v;
            std::printf(", \"skin_node\": {\"rays\": [%lld, %lld, %lld, %lld, %lld], \"hits\": %lld, \"aovs\": \"%016llx\", "
                        "\"out\": \"%016llx\", \"scalars\": \"%016llx\", \"mean_out\": %.9g}",
                        (long long)rays[0], (long long)rays[1], (long long)rays[2], (long long)rays[3], (long long)cap,
                        (long long)found, (unsigned long long)fnv(ra), (unsigned long long)fnv(ro), (unsigned long long)fnv(sc),
                        mean / (double)ro.size());
        }
        std::printf(", \"points\": %lld, \"spp_n\": %d}\n", (long long)n, spp_n);
    } catch (const rlsb::Error &e) {
        std::fprintf(stderr, "example_trace: %s (status %d)\n", e.what(), (int)e.status);
        return 1;
    }
    return 0;
}
