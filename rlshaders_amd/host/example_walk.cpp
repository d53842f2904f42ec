// example_walk.cpp -- rlSss's probe rays walked on the device (rls_walk.hpp): shading points on a sphere, integrateScatter's probe
// rays emitted (rlsb::emitProbes), every round the nearest hit of the active rays from a ten-line closest-hit function on the
// host -- all a wavefront renderer has -- handed to rlsb::ProbeWalk::step, then rlsb::resolveScatter on the hits the walk wrote.
// From a hit's own position the sphere is found again at t ~ 0: the walk refuses those hits (the AI_EPSILON test against the last
// accepted position) and spends a trial on each, as the reference does.
//
// usage: example_walk [n] [spp_n]; prints one JSON line: the active rays before every step, the hits stored, and checksums
// (FNV-1a over the bits) of the hit counts and of the resolved planes, which tests/test_gpu_walk_host_cpp.py compares with the
// Python path (rlshaders_amd.walk).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rls_walk.hpp"

namespace {
constexpr uint32_t kSeed = 1234;
constexpr float kRadius = 0.5f;              // the sphere, about the origin

uint64_t fnv(const void *data, size_t bytes)
{
    uint64_t h = 1469598103934665603ull;
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t k = 0; k < bytes; k++) { h ^= p[k]; h *= 1099511628211ull; }
    return h;
}

// the renderer's tracer: the closest hit of the sphere in (0, maxdist] from o along d -> t, or 0 for none
float closestHit(const float o[3], const float d[3], float maxdist)
{
    const float a = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], b = (o[0] * d[0] + o[1] * d[1]) + o[2] * d[2];
    const float c = ((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]) - kRadius * kRadius;
    const float disc = b * b - a * c;
    if (!(disc >= 0.0f) || a == 0.0f) return 0.0f;
    const float sq = std::sqrt(disc), t0 = (-b - sq) / a, t1 = (-b + sq) / a;
    const float t = t0 > 0.0f ? t0 : t1;
    return t > 0.0f && t <= maxdist ? t : 0.0f;
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
    const int spp_n = argc > 2 ? std::atoi(argv[2]) : 2;
    const int64_t rays = n * spp_n * spp_n;
    try {
        rlsb::Device dev(0);
        rlsb::Planes frame(dev, n, 9);
        rlsb::check(rls_gen_frame(dev.ctx(), kSeed, 0, n, frame.vec3(0), frame.vec3(3), frame.vec3(6)));
        rls_sss_closure sc = {};
        sc.sss_color = rlsb::ParamRGB(0.8f, 0.5f, 0.3f).c();
        sc.sss_dist_multiplier = rls_param{nullptr, 1.0f};
        sc.sss_scatter_dist[0] = rls_param{nullptr, 0.05f};
        sc.sss_scatter_dist[1] = rls_param{nullptr, 0.1f};
        sc.sss_scatter_dist[2] = rls_param{nullptr, 0.2f};
        sc.N = frame.cvec3(3); sc.T = frame.cvec3(6); sc.has_dPdu = 1;
        // the shading points: on the sphere, where their normals point
        std::vector<float> pts = frame.download();
        std::vector<float> Ph((size_t)(3 * n));
        for (size_t k = 0; k < Ph.size(); k++) Ph[k] = kRadius * pts[(size_t)(3 * n) + k];
        rlsb::Planes P(dev, Ph, 3), out(dev, n, 3), depth(dev, n, 1);

        rlsb::ProbeQueue pq(dev, n, spp_n);
        rlsb::emitProbes(dev, sc, P, n, spp_n, kSeed, pq);
        rlsb::ProbeWalk walk(dev, rays);
        walk.begin(pq, P);

        std::printf("{\"rays\": %lld, \"steps\": [", (long long)rays);
        rlsb::Planes found(dev, rays, 10);                          // t, P, N, Ns of the listed rays
        void *dhit = nullptr;
        rlsb::check(rls_device_alloc(dev.ctx(), (size_t)(rays > 0 ? rays : 1), &dhit));
        int steps = 0;
        for (int64_t m; (m = walk.active()) > 0; steps++) {
            std::printf("%s%lld", steps ? ", " : "", (long long)m);
            const rls_walk_rays &r = walk.rays();
            std::vector<float> o[3], d[3], md = download(dev, r.maxdist, m);
            for (int k = 0; k < 3; k++) { o[k] = download(dev, (&r.origin.x)[k], m); d[k] = download(dev, (&r.dir.x)[k], m); }
            std::vector<uint8_t> hit((size_t)rays, 0);
            std::vector<float> f((size_t)(10 * rays), 0.0f);
            for (int64_t k = 0; k < m; k++) {
                const float ok[3] = {o[0][(size_t)k], o[1][(size_t)k], o[2][(size_t)k]};
                const float dk[3] = {d[0][(size_t)k], d[1][(size_t)k], d[2][(size_t)k]};
                const float t = closestHit(ok, dk, md[(size_t)k]);
                if (t == 0.0f) continue;
                hit[(size_t)k] = 1;
                f[(size_t)k] = t;
                for (int a = 0; a < 3; a++) {
                    const float p = ok[a] + dk[a] * t, nrm = p / kRadius;
                    f[(size_t)((1 + a) * rays + k)] = p;
                    f[(size_t)((4 + a) * rays + k)] = nrm;           // sg->N
                    f[(size_t)((7 + a) * rays + k)] = nrm;           // sg->Ns
                }
            }
            found.upload(f);
            rlsb::check(rls_copy_to_device(dev.ctx(), dhit, hit.data(), (size_t)rays));
            rls_walk_found wf = {};
            wf.hit = static_cast<const uint8_t *>(dhit); wf.t = found.plane(0);
            wf.P = found.cvec3(1); wf.N = found.cvec3(4); wf.Ns = found.cvec3(7);
            walk.step(wf, m);
        }
        rlsb::check(rls_device_free(dev.ctx(), dhit));

        // E = 1 / pi at every hit slot (only the slots below a ray's count are read)
        rlsb::Planes E(dev, std::vector<float>((size_t)(3 * RLS_MAX_PROBE_HITS * rays), 0.318309886f), 3);
        rlsb::resolveScatter(dev, sc, P, pq, walk.hits(rls_crgb{E.plane(0), E.plane(1), E.plane(2)}), false, false, out, depth.plane(0));
        std::vector<float> res = out.download(), dres = depth.download();
        std::vector<uint8_t> cnt = download(dev, walk.c().hits.count, rays);
        long long stored = 0;
        for (uint8_t c : cnt) stored += c;
        double mean = 0.0, mdepth = 0.0;
        for (float v : res) mean += v;
        for (float v : dres) mdepth += v;
        std::printf("], \"hits\": %lld, \"count_checksum\": \"%016llx\", \"checksum\": \"%016llx\", \"mean\": %.9g, \"mean_depth\": %.9g}\n",
                    stored, (unsigned long long)fnv(cnt.data(), cnt.size()), (unsigned long long)fnv(res.data(), res.size() * sizeof(float)),
                    mean / (double)(res.empty() ? 1 : res.size()), mdepth / (double)(n > 0 ? n : 1));
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "example_walk: %s\n", e.what());
        return 1;
    }
}
