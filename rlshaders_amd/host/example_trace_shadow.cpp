// example_trace_shadow.cpp -- coloured shadows through the caller's tracer from C++ (rls_trace.hpp: ggxOpacity, skinOpacity,
// ShadowHits, foldVisibility).  rlGgx points under two lights emit their light loop's shadow queue.  The stand-in tracer gives
// every shadow ray one hit on a tinted rlGgx sheet (Kt = 0.5) and every odd ray a second hit on an rlSkin surface; the two
// surfaces' sg->out_opacity at a shadow ray's point come from the library into a two-entry table, the hits name their surface by
// index, the fold turns them into the visibility of every ray, and resolveDirect lights the points under those shadows.
//
//   example_trace_shadow [points] [spp_n]
// prints one JSON line: the ray count and checksums (FNV-1a over the bits of the visibility of the queue's rays and of the two
// AOVs), which tests/test_gpu_trace_opacity_host_cpp.py compares with the Python path (rlshaders_amd/trace.py) on the same inputs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rls_trace.hpp"

namespace {
constexpr uint32_t kSeed = 1234;

uint64_t fnv(const std::vector<float> &v)
{
    const uint8_t *p = reinterpret_cast<const uint8_t *>(v.data());
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < 4 * v.size(); k++) { h ^= p[k]; h *= 1099511628211ull; }
    return h;
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
        const int64_t rays = sq.count();

        // 2. the two surfaces a shadow ray can cross, shaded as shadow rays' points: entry 0 the tinted rlGgx sheet
        // (1 - KtColor * Kt), entry 1 the rlSkin surface (clamp(opacity * opacity_color), nothing before it on the ray)
        std::vector<uint8_t> type(5 * 2, 0);
        type[0] = type[1] = RLS_RT_SHADOW;
        rlsb::RayState surfaces(dev, type);
        rlsb::Planes table(dev, 2, 3);
        rls_ggx_opacity sheet = {};
        sheet.opacity = rls_param{nullptr, 1.0f};
        sheet.opacity_color = rlsb::ParamRGB(1.0f, 1.0f, 1.0f).c();
        sheet.KtColor = rlsb::ParamRGB(0.2f, 0.9f, 0.7f).c();
        sheet.Kt = rls_param{nullptr, 0.5f};
        rlsb::ggxOpacity(dev, sheet, 1, surfaces.c().ray_type, table.rgb());
        rls_skin_opacity skin = {};
        skin.opacity = rls_param{nullptr, 0.75f};
        skin.opacity_color = rlsb::ParamRGB(0.9f, 0.8f, 0.6f).c();
        rlsb::skinOpacity(dev, skin, 1, surfaces.c(1).ray_type, rlsb::Planes(),
                          rls_rgb{table.plane(0) + 1, table.plane(1) + 1, table.plane(2) + 1});

        // 3. the renderer's tracer: ray j crosses the sheet, odd rays the skin surface behind it
        const int maxHits = 2;
        rlsb::ShadowHits hits(dev, rays, maxHits, rlsb::ShadowHits::Indexed);
        std::vector<uint8_t> count((size_t)rays);
        std::vector<uint32_t> index((size_t)(maxHits * rays), 0u);
        for (int64_t j = 0; j < rays; j++) {
            count[(size_t)j] = (uint8_t)(1 + (j & 1));
            index[(size_t)(rays + j)] = 1u;
        }
        if (rays > 0) {
            rlsb::check(rls_copy_to_device(dev.ctx(), hits.count(), count.data(), count.size()));
            rlsb::check(rls_copy_to_device(dev.ctx(), hits.index(), index.data(), index.size() * sizeof(uint32_t)));
        }

        // 4. fold the hits into the visibility, resolve the light loop under it
        const int64_t cap = sq.c().capacity > 0 ? sq.c().capacity : 1;
        rlsb::Planes visibility(dev, cap, 3), dd(dev, n, 3), ds(dev, n, 3);
        rlsb::foldVisibility(dev, rays, hits.c(table, 2), rlsb::Planes(), visibility);
        rlsb::resolveDirect(dev, c, sh, lights, 2, sq, visibility, dd, ds);

        const std::vector<float> all = visibility.download();
        std::vector<float> vis;
        for (int k = 0; k < 3; k++) vis.insert(vis.end(), all.begin() + (size_t)(k * cap), all.begin() + (size_t)(k * cap + rays));
        double mean = 0.0;
        for (float v : vis) mean += v;
        std::printf("{\"points\": %lld, \"spp_n\": %d, \"rays\": %lld, \"visibility\": \"%016llx\", \"direct_diffuse\": \"%016llx\", "
                    "\"direct_specular\": \"%016llx\", \"mean_visibility\": %.9g}\n", (long long)n, spp_n, (long long)rays,
                    (unsigned long long)fnv(vis), (unsigned long long)fnv(dd.download()), (unsigned long long)fnv(ds.download()),
                    vis.empty() ? 0.0 : mean / (double)vis.size());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "example_trace_shadow: %s\n", e.what());
        return 1;
    }
    return 0;
}
