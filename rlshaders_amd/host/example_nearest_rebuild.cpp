// example_nearest_rebuild.cpp -- example_nearest's scene over three frames, its sphere twisting (rls_nearest_rebuild.hpp over
// rls_nearest.hpp): a tinted quad above rlGgx points under two lights and an opaque tessellated sphere on the way to the first
// light.  Every frame the sphere is twisted about its vertical axis -- by 0, 0.5 and 2 radians end to end --, its vertices and
// shading normals go to the device, and rlsb::NearestRebuild::update rebuilds the tree of the ONE scene made before the first
// frame there, on the device: no host builder runs again and nothing is allocated.  The light loop's shadow rays are then walked
// through the rebuilt scene (rlsb::ShadowWalk) and rlSss's probe rays of points on the twisted sphere too (rlsb::ProbeWalk), as
// example_nearest walks them.  Beside it the same two walks run on a FRESH rlsb::NearestScene built from the frame's vertices:
// the rebuilt tree is the tree that scene holds, so the checksums agree frame by frame -- and so does the tree itself, whose
// links and leaf order are compared here.
//
// usage: example_nearest_rebuild [points] [spp_n] [max_steps]; prints one JSON line: the scene's size and, per frame, under
// "rebuilt" and "fresh" the steps, the rays left black, checksums (FNV-1a over the bits) of the visibility and the two AOVs and
// of the probes' stored hits, and "tree": whether links and leaf order equal the fresh scene's;
// tests/test_gpu_nearest_rebuild_host_cpp.py compares them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "rls_nearest_rebuild.hpp"
#include "rls_shadow_walk.hpp"
#include "rls_walk.hpp"

namespace {
constexpr uint32_t kSeed = 1234;
constexpr int kFrames = 3;
constexpr float kQuadZ = 0.8f, kQuadHalf = 10.0f;                      // the quad: surface 0
const float kQuadKt[3] = {0.2f, 0.9f, 0.7f};
const double kCenter[3] = {-1.63, 0.82, 1.23};                         // the sphere: surface 1
constexpr double kRadius = 0.25;
constexpr int kLevel = 3;

uint64_t fnv(const void *data, size_t bytes, uint64_t h = 1469598103934665603ull)
{
    const uint8_t *p = static_cast<const uint8_t *>(data);
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

// the unit sphere: an octahedron subdivided kLevel times, every new vertex the normalised sum of its edge's ends
void unitSphere(std::vector<double> &U, std::vector<uint32_t> &F)
{
    U = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
    F = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
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
}

// frame f: the sphere twisted about y by `radians` end to end over its height; frame 0 is example_nearest's sphere
struct Pose { double radians; };
Pose poseOf(int f)
{
    const double r[kFrames] = {0.0, 0.5, 2.0};
    return Pose{r[f]};
}
// a point of the twisted sphere from a unit direction, and a shading normal (the direction turned with the point)
void posed(const Pose &p, const double u[3], float P[3], float N[3])
{
    const double a = p.radians * (u[1] + 1.0) * 0.5, c = std::cos(a), s = std::sin(a);
    const double t[3] = {c * u[0] + s * u[2], u[1], -s * u[0] + c * u[2]};
    for (int k = 0; k < 3; k++) { P[k] = (float)(kCenter[k] + kRadius * t[k]); N[k] = (float)t[k]; }
}

struct Inputs {
    int64_t n;
    int spp_n, max_steps;
    const rls_ggx_closure *c;
    const rls_ggx_shader *sh;
    const rls_sphere_light *lights;
    const rlsb::Planes *P, *frame, *table;
};

// the two walks of example_nearest over `scene`; Pp: the probes' points -> one JSON object
std::string walks(const rlsb::Device &dev, const rlsb::NearestScene &scene, const Inputs &in, const rlsb::Planes &Pp)
{
    const int64_t n = in.n;
    char buf[512];
    std::string out = "{\"steps\": [";
    rlsb::ShadowQueue sq(dev, n, 2, in.spp_n, rlsb::ShadowQueue::Ggx);
    rlsb::emitDirect(dev, *in.c, *in.sh, *in.P, in.lights, 2, n, in.spp_n, kSeed, sq);
    const int64_t cap = sq.c().capacity;
    rlsb::ShadowWalk walk(dev, cap);
    walk.begin(sq, *in.P, in.max_steps);
    rlsb::NearestFound found(dev, cap, rlsb::NearestFound::ForShadowWalk);
    found.resetLast(dev);
    int steps = 0;
    for (int64_t m; (m = walk.active()) > 0; steps++) {
        out += (steps ? ", " : "") + std::to_string((long long)m);
        scene.hits(walk.rays(), m, found);
        walk.step(found.shadowFound(rls_crgb{in.table->plane(0), in.table->plane(1), in.table->plane(2)}, 2u), m);
    }
    rlsb::Planes dd(dev, n, 3), ds(dev, n, 3);
    rlsb::resolveDirect(dev, *in.c, *in.sh, in.lights, 2, sq, walk.visibility(), dd, ds);
    const int64_t rays = sq.count(), slots = cap > 0 ? cap : 1;
    const std::vector<float> all = walk.visibility().download();
    std::vector<float> vis;
    for (int k = 0; k < 3; k++) vis.insert(vis.end(), all.begin() + (size_t)(k * slots), all.begin() + (size_t)(k * slots + rays));
    long long black = 0;
    for (int64_t j = 0; j < rays; j++)
        if (vis[(size_t)j] == 0.0f && vis[(size_t)(rays + j)] == 0.0f && vis[(size_t)(2 * rays + j)] == 0.0f) black++;
    std::snprintf(buf, sizeof buf, "], \"rays\": %lld, \"black\": %lld, \"visibility\": \"%016llx\", \"direct_diffuse\": \"%016llx\", "
                  "\"direct_specular\": \"%016llx\", \"probes\": {\"steps\": [", (long long)rays, black, (unsigned long long)fnv(vis),
                  (unsigned long long)fnv(dd.download()), (unsigned long long)fnv(ds.download()));
    out += buf;

    rls_sss_closure sc = {};
    sc.sss_color = rlsb::ParamRGB(0.8f, 0.5f, 0.3f).c();
    sc.sss_dist_multiplier = rls_param{nullptr, 1.0f};
    sc.sss_scatter_dist[0] = rls_param{nullptr, 0.05f};
    sc.sss_scatter_dist[1] = rls_param{nullptr, 0.1f};
    sc.sss_scatter_dist[2] = rls_param{nullptr, 0.2f};
    sc.N = in.frame->cvec3(3); sc.T = in.frame->cvec3(6); sc.has_dPdu = 1;
    const int64_t prays = n * in.spp_n * in.spp_n, pslots = prays > 0 ? prays : 1;
    rlsb::ProbeQueue pq(dev, n, in.spp_n);
    rlsb::emitProbes(dev, sc, Pp, n, in.spp_n, kSeed, pq);
    rlsb::ProbeWalk pwalk(dev, prays);
    pwalk.begin(pq, Pp);
    rlsb::NearestFound pfound(dev, prays, rlsb::NearestFound::ForWalk);
    pfound.resetLast(dev);
    int psteps = 0;
    for (int64_t m; (m = pwalk.active()) > 0; psteps++) {
        out += (psteps ? ", " : "") + std::to_string((long long)m);
        scene.hits(pwalk.rays(), m, pfound);
        pwalk.step(pfound.walkFound(false), m);
    }
    const rls_walk_hits &wh = pwalk.c().hits;
    const std::vector<uint8_t> cnt = download(dev, wh.count, prays);
    std::vector<float> hitP, hitN;
    for (int a = 0; a < 3; a++) {
        const std::vector<float> pa = download(dev, (&wh.P.x)[a], pslots * wh.max_hits), na = download(dev, (&wh.N.x)[a], pslots * wh.max_hits);
        for (int k = 0; k < wh.max_hits; k++)
            for (int64_t j = 0; j < prays; j++)
                if (k < cnt[(size_t)j]) { hitP.push_back(pa[(size_t)(k * wh.stride + j)]); hitN.push_back(na[(size_t)(k * wh.stride + j)]); }
    }
    long long stored = 0;
    for (uint8_t c8 : cnt) stored += c8;
    std::snprintf(buf, sizeof buf, "], \"hits\": %lld, \"count\": \"%016llx\", \"P\": \"%016llx\", \"N\": \"%016llx\"}}", stored,
                  (unsigned long long)fnv(cnt.data(), cnt.size()), (unsigned long long)fnv(hitP), (unsigned long long)fnv(hitN));
    return out + buf;
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

        // the two surfaces, shaded as shadow rays' points: the quad 1 - KtColor * Kt at Kt = 0.5, the sphere (Kt = 0) opaque
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

        // the mesh: the sphere's triangles, then the quad's two; per frame the sphere's vertices and normals are posed
        std::vector<double> U;
        std::vector<uint32_t> T;
        unitSphere(U, T);
        const size_t sv = U.size() / 3;
        std::vector<uint32_t> S(T.size() / 3, 1u);
        const uint32_t q = (uint32_t)sv, quad[6] = {q, q + 1, q + 2, q, q + 2, q + 3};
        T.insert(T.end(), quad, quad + 6);
        S.push_back(0u); S.push_back(0u);
        auto meshOf = [&](int f, std::vector<float> &V, std::vector<float> &Nn) {
            const Pose pose = poseOf(f);
            V.assign(3 * (sv + 4), 0.0f); Nn.assign(3 * (sv + 4), 0.0f);
            for (size_t i = 0; i < sv; i++) posed(pose, &U[3 * i], &V[3 * i], &Nn[3 * i]);
            const float corners[4][2] = {{-kQuadHalf, -kQuadHalf}, {kQuadHalf, -kQuadHalf}, {kQuadHalf, kQuadHalf}, {-kQuadHalf, kQuadHalf}};
            for (size_t k = 0; k < 4; k++) {
                V[3 * (sv + k)] = corners[k][0]; V[3 * (sv + k) + 1] = corners[k][1]; V[3 * (sv + k) + 2] = kQuadZ;
                Nn[3 * (sv + k) + 2] = 1.0f;
            }
        };
        std::vector<float> V, Nn;
        meshOf(0, V, Nn);
        rls_nearest_mesh mesh = {};
        mesh.nv = (int64_t)(V.size() / 3); mesh.nt = (int64_t)(T.size() / 3);
        mesh.vertices = V.data(); mesh.triangles = T.data(); mesh.surface = S.data(); mesh.normals = Nn.data();
        rlsb::NearestScene scene(dev, mesh);                         // built once, on frame 0's mesh
        rlsb::NearestRebuild rebuild(dev, scene);
        const rls_nearest_rebuild_info info = rebuild.info();
        std::printf("{\"points\": %lld, \"spp_n\": %d, \"triangles\": %lld, \"nodes\": %lld, \"levels\": %d, \"frames\": [", (long long)n, spp_n,
                    (long long)info.nt, (long long)info.nodes, info.levels);

        const Inputs in = {n, spp_n, max_steps, &c, &sh, lights, &P, &frame, &table};
        const std::vector<float> dirs = frame.download();            // the probes' points: where the points' normals point
        for (int f = 0; f < kFrames; f++) {
            meshOf(f, V, Nn);
            const Pose pose = poseOf(f);
            std::vector<float> Ph((size_t)(3 * n));
            for (int64_t i = 0; i < n; i++) {
                const double u[3] = {dirs[(size_t)(3 * n + i)], dirs[(size_t)(4 * n + i)], dirs[(size_t)(5 * n + i)]};
                float p[3], nn[3];
                posed(pose, u, p, nn);
                for (int a = 0; a < 3; a++) Ph[(size_t)(a * n + i)] = p[a];
            }
            rlsb::Planes Pp(dev, Ph, 3);
            // the deformer's output, on the device: [nv * 3] vertices and normals (one plane each, as the mesh holds them)
            rlsb::Planes Vd(dev, V, 1), Nd(dev, Nn, 1);
            rebuild.update(Vd.plane(0), Nd.plane(0));
            const std::string moved = walks(dev, scene, in, Pp);
            mesh.vertices = V.data(); mesh.normals = Nn.data();
            rlsb::NearestScene fresh(dev, mesh);
            const std::string built = walks(dev, fresh, in, Pp);
            // the tree itself: the fresh scene's, read through a rebuild of its own that is never updated
            rlsb::NearestRebuild reader(dev, fresh);
            std::vector<float> b0, b1;
            std::vector<uint32_t> l0, l1, p0, p1;
            rebuild.readTree(b0, l0, p0);
            reader.readTree(b1, l1, p1);
            bool boxes = b0.size() == b1.size();
            for (size_t k = 0; boxes && k < b0.size(); k++) boxes = b0[k] == b1[k];
            std::printf("%s{\"frame\": %d, \"radians\": %.1f, \"tree\": %s, \"rebuilt\": %s, \"fresh\": %s}", f ? ", " : "", f, pose.radians,
                        l0 == l1 && p0 == p1 && boxes ? "true" : "false", moved.c_str(), built.c_str());
        }
        std::printf("], \"device_bytes\": %lld, \"updates\": %lld}\n", (long long)info.device_bytes, (long long)rebuild.info().updates);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "example_nearest_rebuild: %s\n", e.what());
        return 1;
    }
    return 0;
}
