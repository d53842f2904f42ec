// example_nearest_group.cpp -- three instances of ONE tessellated sphere under a group (rls_nearest_group.hpp over rls_nearest.hpp):
// two overlapping translucent ones on the way from rlGgx points to the first light, an opaque one on the way to the second.  The
// light loop's shadow rays are walked through the group (rlsb::ShadowWalk: the based surface id indexes the opacity table), and a
// glossy queue's rays are traced through it and routed by the node bin of the instance they hit (rlsb::HitRoutes).  Then one
// instance is turned and moved -- two matrices written on the device, rlsb::NearestGroup::update -- and both run again.  Beside
// each run the same queries go through a FRESH group made with the same matrices: a query's result is a function of instances,
// meshes and ray alone, so the checksums agree.
//
// usage: example_nearest_group [points] [spp_n] [max_steps]; prints one JSON line: per frame, under "group" and "fresh", the
// walk's steps, the rays left black, checksums (FNV-1a over the bits) of the visibility and of the found planes of the glossy
// rays, and the rays routed to each bin.  Exits 1 where a group and its fresh twin differ, or where the move changed nothing;
// tests/test_gpu_nearest_group_host_cpp.py runs it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "rls_nearest_group.hpp"
#include "rls_shadow_walk.hpp"

namespace {
constexpr uint32_t kSeed = 1234;
constexpr int kLevel = 3, kInstances = 3;
constexpr double kRadius = 0.25;

uint64_t fnv(const void *data, size_t bytes, uint64_t h = 1469598103934665603ull)
{
    const uint8_t *p = static_cast<const uint8_t *>(data);
    for (size_t k = 0; k < bytes; k++) { h ^= p[k]; h *= 1099511628211ull; }
    return h;
}

template <class T>
std::vector<T> download(const rlsb::Device &dev, const T *p, int64_t count)
{
    std::vector<T> v((size_t)count);
    if (count > 0) rlsb::check(rls_copy_to_host(dev.ctx(), v.data(), p, sizeof(T) * v.size()));
    return v;
}

// the unit sphere: an octahedron subdivided kLevel times, every new vertex the normalised sum of its edge's ends
void unitSphere(std::vector<float> &V, std::vector<uint32_t> &F)
{
    std::vector<double> U = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
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
    V.assign(U.begin(), U.end());
}

// a placement: the unit sphere scaled to kRadius * stretch along x, turned by `turn` about z, its centre at c.  to_world = [R S | c],
// to_object = [S^-1 R^T | -S^-1 R^T c], both computed in double and rounded once.
struct Pose { double c[3], turn, stretch; };
void place(const Pose &p, const rls_nearest_scene *scene, uint32_t base, rls_nearest_instance &out)
{
    const double cs = std::cos(p.turn), sn = std::sin(p.turn), S[3] = {kRadius * p.stretch, kRadius, kRadius};
    const double R[3][3] = {{cs, -sn, 0}, {sn, cs, 0}, {0, 0, 1}};
    out.scene = scene;
    out.surface_base = base;
    for (int r = 0; r < 3; r++) {
        double t = 0;
        for (int k = 0; k < 3; k++) {
            out.to_world[4 * r + k] = (float)(R[r][k] * S[k]);
            out.to_object[4 * r + k] = (float)(R[k][r] / S[r]);
            t += R[k][r] * p.c[k];
        }
        out.to_world[4 * r + 3] = (float)p.c[r];
        out.to_object[4 * r + 3] = (float)(-t / S[r]);
    }
}

struct Inputs {
    int64_t n;
    int spp_n, max_steps;
    const rls_ggx_closure *c;
    const rls_ggx_shader *sh;
    const rls_sphere_light *lights;
    const rlsb::Planes *P, *table;
    const uint8_t *bins;              // device: the node bin of each based surface id
};

// the shadow walk and the routed glossy queue over `group` -> one JSON object
std::string frame(const rlsb::Device &dev, const rlsb::NearestGroup &group, const Inputs &in)
{
    const int64_t n = in.n;
    char buf[640];
    std::string out = "{\"steps\": [";
    rlsb::ShadowQueue sq(dev, n, 2, in.spp_n, rlsb::ShadowQueue::Ggx);
    rlsb::emitDirect(dev, *in.c, *in.sh, *in.P, in.lights, 2, n, in.spp_n, kSeed, sq);
    const int64_t cap = sq.c().capacity;
    rlsb::ShadowWalk walk(dev, cap);
    walk.begin(sq, *in.P, in.max_steps);
    rlsb::NearestGroupFound found(dev, cap, rlsb::NearestFound::ForShadowWalk);
    found.resetLast(dev);
    int steps = 0;
    for (int64_t m; (m = walk.active()) > 0; steps++) {
        out += (steps ? ", " : "") + std::to_string((long long)m);
        group.hits(walk.rays(), m, found);
        walk.step(found.found().shadowFound(rls_crgb{in.table->plane(0), in.table->plane(1), in.table->plane(2)}, (uint32_t)kInstances), m);
    }
    const int64_t rays = sq.count(), slots = cap > 0 ? cap : 1;
    const std::vector<float> all = walk.visibility().download();
    std::vector<float> vis;
    for (int k = 0; k < 3; k++) vis.insert(vis.end(), all.begin() + (size_t)(k * slots), all.begin() + (size_t)(k * slots + rays));
    long long black = 0, tinted = 0;
    for (int64_t j = 0; j < rays; j++) {
        const float r = vis[(size_t)j], g = vis[(size_t)(rays + j)], b = vis[(size_t)(2 * rays + j)];
        if (r == 0.0f && g == 0.0f && b == 0.0f) black++;
        else if (!(r == 1.0f && g == 1.0f && b == 1.0f)) tinted++;
    }
    std::snprintf(buf, sizeof buf, "], \"rays\": %lld, \"black\": %lld, \"tinted\": %lld, \"visibility\": \"%016llx\", \"glossy\": {", (long long)rays,
                  black, tinted, (unsigned long long)fnv(vis.data(), 4 * vis.size()));
    out += buf;

    // the glossy queue: origins through its point plane, no reach; the found planes a node call would be gathered from
    rlsb::RayQueue gq(dev, n, in.spp_n, rlsb::RayQueue::Glossy);
    rlsb::emitGlossy(dev, *in.c, n, in.spp_n, kSeed, gq);
    const int64_t gcap = gq.c().capacity, grays = gq.count();
    rlsb::NearestGroupFound gf(dev, gcap, rlsb::NearestFound::ForRouting | rlsb::NearestFound::Prim);
    gf.found().binsFrom(in.bins, (uint32_t)kInstances);
    rls_nearest_rays r = {};
    r.rays = gcap; r.count = gq.c().offsets + n;
    r.origin = in.P->cvec3(0); r.via = gq.c().point;
    r.dir = rls_cvec3{gq.c().dir.x, gq.c().dir.y, gq.c().dir.z};
    group.hits(r, gf);
    rlsb::HitRoutes routes(dev, gcap, 2);
    // entries past the queue's count were not traced: their bin bytes are whatever the buffer held, so route the traced rays only
    rlsb::check(rls_trace_route_hits(dev.ctx(), grays, gf.found().bin(), &routes.c()));
    const rls_nearest_found &f = gf.found().c();
    const std::vector<uint8_t> hit = download(dev, f.hit, grays);
    const std::vector<uint32_t> inst = download(dev, gf.instance(), grays), prim = download(dev, f.prim, grays);
    const std::vector<float> t = download(dev, f.t, grays), Nx = download(dev, f.N.x, grays), Tx = download(dev, f.T.x, grays),
                             Px = download(dev, f.P.x, grays);
    uint64_t h = fnv(hit.data(), hit.size());
    long long hits = 0, per[kInstances] = {0, 0, 0};
    for (int64_t j = 0; j < grays; j++)
        if (hit[(size_t)j]) {
            hits++;
            per[inst[(size_t)j] < (uint32_t)kInstances ? inst[(size_t)j] : 0]++;
            const uint32_t w[6] = {inst[(size_t)j], prim[(size_t)j]};
            h = fnv(w, 8, h);
            const float v[4] = {t[(size_t)j], Nx[(size_t)j], Tx[(size_t)j], Px[(size_t)j]};
            h = fnv(v, 16, h);
        }
    std::snprintf(buf, sizeof buf, "\"rays\": %lld, \"hits\": %lld, \"instances\": [%lld, %lld, %lld], \"found\": \"%016llx\", \"routed\": [%lld, %lld], "
                  "\"missed\": %lld}}", (long long)grays, hits, per[0], per[1], per[2], (unsigned long long)h, (long long)routes.size(0),
                  (long long)routes.size(1), (long long)routes.size(2));
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
        rlsb::Planes fr(dev, n, 9);
        rlsb::check(rls_gen_frame(dev.ctx(), kSeed, 0, n, fr.vec3(0), fr.vec3(3), fr.vec3(6)));
        rls_ggx_closure c = {};
        c.wo = fr.cvec3(0); c.N = fr.cvec3(3); c.T = fr.cvec3(6);
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

        // the based surface ids 0, 1, 2 = the instances, shaded as shadow rays' points: the first two 1 - KtColor * Kt at
        // Kt = 0.5, the third (Kt = 0) opaque; and their node bins for the routing: the translucent ones bin 0, the opaque one 1
        std::vector<uint8_t> type((size_t)(5 * kInstances), 0);
        for (int k = 0; k < kInstances; k++) type[(size_t)k] = RLS_RT_SHADOW;
        rlsb::RayState shadowPoints(dev, type);
        rlsb::Planes table(dev, kInstances, 3);
        const float kt[kInstances][3] = {{0.2f, 0.9f, 0.7f}, {0.8f, 0.3f, 0.5f}, {1.0f, 1.0f, 1.0f}};
        for (int k = 0; k < kInstances; k++) {
            rls_ggx_opacity o = {};
            o.opacity = rls_param{nullptr, 1.0f};
            o.opacity_color = rlsb::ParamRGB(1.0f, 1.0f, 1.0f).c();
            o.KtColor = rlsb::ParamRGB(kt[k][0], kt[k][1], kt[k][2]).c();
            o.Kt = rls_param{nullptr, k < 2 ? 0.5f : 0.0f};
            rlsb::ggxOpacity(dev, o, 1, shadowPoints.c(k).ray_type, rls_rgb{table.plane(0) + k, table.plane(1) + k, table.plane(2) + k});
        }
        rlsb::detail::DeviceBuffers bufs(dev);
        uint8_t *bins = bufs.alloc<uint8_t>(kInstances);
        const uint8_t binOf[kInstances] = {0, 0, 1};
        rlsb::check(rls_copy_to_device(dev.ctx(), bins, binOf, sizeof binOf));

        // ONE mesh, one tree; three placements of it
        std::vector<float> V;
        std::vector<uint32_t> T;
        unitSphere(V, T);
        rls_nearest_mesh mesh = {};
        mesh.nv = (int64_t)(V.size() / 3); mesh.nt = (int64_t)(T.size() / 3);
        mesh.vertices = V.data(); mesh.triangles = T.data(); mesh.normals = V.data();      // the unit sphere's normals are its points
        rlsb::NearestScene scene(dev, mesh);
        Pose poses[kInstances] = {{{-1.63, 0.82, 1.23}, 0.0, 1.0}, {{-1.43, 0.72, 1.05}, 0.4, 1.5}, {{1.8, 0.3, 0.6}, -0.7, 2.0}};
        std::vector<rls_nearest_instance> placed((size_t)kInstances);
        for (int k = 0; k < kInstances; k++) place(poses[k], scene.c(), (uint32_t)k, placed[(size_t)k]);
        rlsb::NearestGroup group(dev, placed);
        const rls_nearest_group_info info = group.info();
        std::printf("{\"points\": %lld, \"spp_n\": %d, \"triangles\": %lld, \"instances\": %lld, \"scenes\": %lld, \"top_nodes\": %lld, \"frames\": [",
                    (long long)n, spp_n, (long long)mesh.nt, (long long)info.instances, (long long)info.scenes, (long long)info.top_nodes);

        const Inputs in = {n, spp_n, max_steps, &c, &sh, lights, &P, &table, bins};
        float *planes = bufs.alloc<float>(2 * 12 * kInstances);        // to_object [3 * 12], then to_world [3 * 12]
        int64_t *parked = bufs.alloc<int64_t>(1);
        bool ok = true;
        std::string before;
        for (int f = 0; f < 2; f++) {
            if (f == 1) {                                                // the opaque instance swings in front of the first light too
                poses[2] = Pose{{-1.9, 0.95, 1.45}, 0.9, 1.2};
                place(poses[2], scene.c(), 2u, placed[2]);
                std::vector<float> host((size_t)(2 * 12 * kInstances));
                for (int k = 0; k < kInstances; k++)
                    for (int e = 0; e < 12; e++) {
                        host[(size_t)(12 * k + e)] = placed[(size_t)k].to_object[e];
                        host[(size_t)(12 * (kInstances + k) + e)] = placed[(size_t)k].to_world[e];
                    }
                rlsb::check(rls_copy_to_device(dev.ctx(), planes, host.data(), sizeof(float) * host.size()));
                group.update(planes, planes + 12 * kInstances, parked);  // no tree is built again, no triangle is touched
                ok = ok && download(dev, parked, 1)[0] == 0;
            }
            const std::string moved = frame(dev, group, in);
            rlsb::NearestGroup fresh(dev, placed);
            const std::string again = frame(dev, fresh, in);
            std::printf("%s{\"frame\": %d, \"group\": %s, \"fresh\": %s}", f ? ", " : "", f, moved.c_str(), again.c_str());
            ok = ok && moved == again;
            if (f == 0) before = moved;
            else ok = ok && moved != before;
        }
        std::printf("], \"updates\": %lld, \"ok\": %s}\n", (long long)group.info().updates, ok ? "true" : "false");
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "example_nearest_group: %s\n", e.what());
        return 1;
    }
}
