// example_nearest_any.cpp -- a light loop's shadow rays answered in one launch (rls_nearest_any.hpp over rls_nearest.hpp and
// rls_shadow_walk.hpp): rlGgx points under two lights emit their shadow queue (rlsb::emitDirect); above them lies a quad and, on
// the way to the first light, a tessellated sphere (a subdivided octahedron, 512 triangles).
//
//   "opaque": both surfaces opaque.  One rls_nearest_any_hits launch writes the visibility (blocked rays 0, the others 1) and
//     rlsb::resolveDirect lights the points; beside it the full shadow walk over nearest hits with an all-ones opacity table.
//     The two visibilities and the two pairs of AOVs agree bit for bit.
//   "mixed": the quad tinted and semi-transparent, the sphere opaque.  The two-phase route -- the flag table from the opacity
//     table, one any-hit launch, the walk begun again on the reach plane so that only the veiled rays are walked, from the
//     visibility the launch wrote -- beside the full walk.  Clear and veiled rays agree bit for bit; a blocked ray is all zero
//     here, and all zero in the full walk wherever that walk met an opaque surface (at grazing geometry it may not).
//
// usage: example_nearest_any [points] [spp_n] [max_steps]; prints one JSON line: per part the rays by state, the rays walked by
// each route, checksums (FNV-1a over the bits) of the visibilities and AOVs and the counts of rays that differ.  Exits 1 where a
// claimed equality fails; tests/test_gpu_nearest_any_host_cpp.py runs it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "rls_nearest_any.hpp"
#include "rls_shadow_walk.hpp"

namespace {
constexpr uint32_t kSeed = 1234;
constexpr float kQuadZ = 0.8f, kQuadHalf = 10.0f;                      // the quad: surface 0
const float kQuadKt[3] = {0.2f, 0.9f, 0.7f};
const double kCenter[3] = {-1.63, 0.82, 1.23};                         // the sphere: surface 1
constexpr double kRadius = 0.25;
constexpr int kLevel = 3, kSurfaces = 2;

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

// the visibility of the queue's rays, plane by plane
std::vector<float> raysOf(const rlsb::Planes &vis, int64_t rays)
{
    const std::vector<float> all = vis.download();
    const int64_t slots = vis.size();
    std::vector<float> out;
    for (int k = 0; k < 3; k++) out.insert(out.end(), all.begin() + (size_t)(k * slots), all.begin() + (size_t)(k * slots + rays));
    return out;
}

// an octahedron subdivided kLevel times about kCenter, then the quad's four vertices and two triangles
void buildMesh(std::vector<float> &V, std::vector<uint32_t> &T, std::vector<uint32_t> &S)
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
    for (size_t i = 0; i < U.size(); i++) V.push_back((float)(kCenter[i % 3] + kRadius * U[i]));
    T = F;
    S.assign(T.size() / 3, 1u);
    const uint32_t q = (uint32_t)(V.size() / 3);
    const float corners[4][2] = {{-kQuadHalf, -kQuadHalf}, {kQuadHalf, -kQuadHalf}, {kQuadHalf, kQuadHalf}, {-kQuadHalf, kQuadHalf}};
    for (const auto &c : corners) { V.push_back(c[0]); V.push_back(c[1]); V.push_back(kQuadZ); }
    const uint32_t quad[6] = {q, q + 1, q + 2, q, q + 2, q + 3};
    T.insert(T.end(), quad, quad + 6);
    S.push_back(0u); S.push_back(0u);
}

// the full shadow walk over nearest hits -> the rays its first list held
int64_t fullWalk(const rlsb::Device &dev, const rlsb::NearestScene &scene, const rlsb::ShadowQueue &sq, const rlsb::Planes &P,
                 const rlsb::Planes &table, int maxSteps, rlsb::ShadowWalk &walk)
{
    walk.begin(sq, P, maxSteps);
    rlsb::NearestFound found(dev, sq.c().capacity, rlsb::NearestFound::ForShadowWalk);
    found.resetLast(dev);
    int64_t first = -1;
    for (int64_t m; (m = walk.active()) > 0;) {
        if (first < 0) first = m;
        scene.hits(walk.rays(), m, found);
        walk.step(found.shadowFound(rlsb::detail::crgb(table), (uint32_t)kSurfaces), m);
    }
    return first < 0 ? 0 : first;
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

        std::vector<float> V;
        std::vector<uint32_t> T, S;
        buildMesh(V, T, S);
        rls_nearest_mesh mesh = {};
        mesh.nv = (int64_t)(V.size() / 3); mesh.nt = (int64_t)(T.size() / 3);
        mesh.vertices = V.data(); mesh.triangles = T.data(); mesh.surface = S.data();
        rlsb::NearestScene scene(dev, mesh);

        rlsb::ShadowQueue sq(dev, n, 2, spp_n, rlsb::ShadowQueue::Ggx);
        rlsb::emitDirect(dev, c, sh, P, lights, 2, n, spp_n, kSeed, sq);
        const int64_t cap = sq.c().capacity, rays = sq.count();

        // the two opacity tables: every entry exactly 1; and the quad 1 - KtColor * Kt at Kt = 0.5 beside the opaque sphere
        rlsb::Planes ones(dev, std::vector<float>((size_t)(3 * kSurfaces), 1.0f), 3);
        std::vector<uint8_t> type((size_t)(5 * kSurfaces), 0);
        for (int k = 0; k < kSurfaces; k++) type[(size_t)k] = RLS_RT_SHADOW;
        rlsb::RayState shadowPoints(dev, type);
        rlsb::Planes mixed(dev, kSurfaces, 3);
        for (int k = 0; k < kSurfaces; k++) {
            rls_ggx_opacity o = {};
            o.opacity = rls_param{nullptr, 1.0f};
            o.opacity_color = rlsb::ParamRGB(1.0f, 1.0f, 1.0f).c();
            o.KtColor = k == 0 ? rlsb::ParamRGB(kQuadKt[0], kQuadKt[1], kQuadKt[2]).c() : rlsb::ParamRGB(1.0f, 1.0f, 1.0f).c();
            o.Kt = rls_param{nullptr, k == 0 ? 0.5f : 0.0f};
            rlsb::ggxOpacity(dev, o, 1, shadowPoints.c(k).ray_type, rls_rgb{mixed.plane(0) + k, mixed.plane(1) + k, mixed.plane(2) + k});
        }

        bool ok = true;
        std::printf("{\"points\": %lld, \"spp_n\": %d, \"triangles\": %lld, \"rays\": %lld, ", (long long)n, spp_n, (long long)mesh.nt, (long long)rays);

        // ---- opaque: one launch, then the resolve; beside it the full walk -------------------------------------------------------
        {
            rlsb::NearestAny any(dev, cap);
            rlsb::Planes vis(dev, cap > 0 ? cap : 1, 3);
            any.hits(scene, rlsb::NearestAny::raysOf(sq, P), vis.rgb());     // no flag table: every triangle is opaque
            rlsb::Planes dd(dev, n, 3), ds(dev, n, 3);
            rlsb::resolveDirect(dev, c, sh, lights, 2, sq, vis, dd, ds);

            rlsb::ShadowWalk walk(dev, cap);
            const int64_t walked = fullWalk(dev, scene, sq, P, ones, max_steps, walk);
            rlsb::Planes wd(dev, n, 3), ws(dev, n, 3);
            rlsb::resolveDirect(dev, c, sh, lights, 2, sq, walk.visibility(), wd, ws);

            const std::vector<float> a = raysOf(vis, rays), b = raysOf(walk.visibility(), rays);
            const std::vector<uint8_t> state = download(dev, any.state(), rays);
            long long by[3] = {0, 0, 0}, differ = 0;
            for (int64_t j = 0; j < rays; j++) {
                by[state[(size_t)j] < 3 ? state[(size_t)j] : 0]++;
                for (int k = 0; k < 3; k++) differ += std::memcmp(&a[(size_t)(k * rays + j)], &b[(size_t)(k * rays + j)], 4) != 0;
            }
            const uint64_t hd = fnv(dd.download()), hs = fnv(ds.download()), gd = fnv(wd.download()), gs = fnv(ws.download());
            ok = ok && differ == 0 && by[2] == 0 && hd == gd && hs == gs;
            std::printf("\"opaque\": {\"clear\": %lld, \"blocked\": %lld, \"veiled\": %lld, \"walk_listed\": %lld, \"differ\": %lld, "
                        "\"visibility\": \"%016llx\", \"walk_visibility\": \"%016llx\", \"direct_diffuse\": \"%016llx\", \"direct_specular\": \"%016llx\", "
                        "\"walk_direct_diffuse\": \"%016llx\", \"walk_direct_specular\": \"%016llx\"}, ", by[0], by[1], by[2], (long long)walked,
                        differ, (unsigned long long)fnv(a), (unsigned long long)fnv(b), (unsigned long long)hd, (unsigned long long)hs,
                        (unsigned long long)gd, (unsigned long long)gs);
        }

        // ---- mixed: the two-phase route beside the full walk -----------------------------------------------------------------------
        {
            rlsb::NearestAny any(dev, cap);
            any.opaqueFrom(rlsb::detail::crgb(mixed), (uint32_t)kSurfaces);
            rlsb::ShadowWalk two(dev, cap);
            const rls_rgb vis = two.c().visibility;
            any.hits(scene, rlsb::NearestAny::raysOf(sq, P), vis);
            two.begin(any.veiled(sq.c()), sq.c().offsets + sq.points(), P.cvec3(), max_steps, rlsb::NearestAny::asBase(vis));
            rlsb::NearestFound found(dev, cap, rlsb::NearestFound::ForShadowWalk);
            found.resetLast(dev);
            int64_t walked = -1;
            for (int64_t m; (m = two.active()) > 0;) {
                if (walked < 0) walked = m;
                scene.hits(two.rays(), m, found);
                two.step(found.shadowFound(rlsb::detail::crgb(mixed), (uint32_t)kSurfaces), m);
            }
            if (walked < 0) walked = 0;

            rlsb::ShadowWalk full(dev, cap);
            const int64_t listed = fullWalk(dev, scene, sq, P, mixed, max_steps, full);

            const std::vector<float> a = raysOf(two.visibility(), rays), b = raysOf(full.visibility(), rays);
            const std::vector<uint8_t> state = download(dev, any.state(), rays), flags = download(dev, any.flags(), kSurfaces);
            long long by[3] = {0, 0, 0}, differ = 0, blockedNonZero = 0, fullNonZero = 0;
            for (int64_t j = 0; j < rays; j++) {
                const uint8_t s = state[(size_t)j] < 3 ? state[(size_t)j] : 0;
                by[s]++;
                bool same = true, zero = true, fullZero = true;
                for (int k = 0; k < 3; k++) {
                    const float x = a[(size_t)(k * rays + j)], y = b[(size_t)(k * rays + j)];
                    same = same && std::memcmp(&x, &y, 4) == 0;
                    zero = zero && x == 0.0f;
                    fullZero = fullZero && y == 0.0f;
                }
                if (s != RLS_NEAREST_ANY_BLOCKED) differ += !same;
                else { blockedNonZero += !zero; fullNonZero += !fullZero; }
            }
            ok = ok && differ == 0 && blockedNonZero == 0 && walked == by[2] && walked < rays && flags[0] == 0 && flags[1] == 1 &&
                 by[1] > 0 && by[2] > 0 && fullNonZero * 100 <= by[1];
            std::printf("\"mixed\": {\"clear\": %lld, \"blocked\": %lld, \"veiled\": %lld, \"walked\": %lld, \"walk_listed\": %lld, \"differ\": %lld, "
                        "\"blocked_not_zero\": %lld, \"walk_blocked_not_zero\": %lld, \"visibility\": \"%016llx\", \"walk_visibility\": \"%016llx\"}, ",
                        by[0], by[1], by[2], (long long)walked, (long long)listed, differ, blockedNonZero, fullNonZero,
                        (unsigned long long)fnv(a), (unsigned long long)fnv(b));
        }
        std::printf("\"ok\": %s}\n", ok ? "true" : "false");
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "example_nearest_any: %s\n", e.what());
        return 1;
    }
}
