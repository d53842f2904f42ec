// rls_trace.hpp -- C++14 host-side mirror of the caller-traced rlGgx, rlDisney and rlSss integrators
// (include/rlshaders_amd_trace.h, librls_trace.so).  Header-only, in the style of rls_batch.hpp, whose Device / Planes /
// check it uses.
//
// Where the reference traces inside integrateGlossy / integrateRefract (AiBRDFIntegrate, src/rlGgx.h:172-179; AiTrace,
// src/rlGgx.h:228-244) or rlDisney's integrateDiffuse / integrateGlossy (AiBRDFIntegrate, src/rlDisney.cpp:240-243,
// 279-283), a renderer's bucket flush does three steps:
//     rlsb::RayQueue q(dev, n, spp_n, rlsb::RayQueue::Glossy);
//     rlsb::emitGlossy(dev, closure, n, spp_n, seed, q, avgReflectWeight);   // every sample ray, compacted
//     ... trace q.dir() [q.count() rays] with the renderer's tracer, one radiance per ray -> radiance (3 planes) ...
//     rlsb::resolveGlossy(dev, q, radiance, sum);                           // sum of radiance x f/pdf per point
// rlDisney: a RayQueue of kind DisneyDiffuse / DisneyGlossy per lobe, emitDisney, and resolveGlossy likewise.
// rlSss (integrateScatter's probe rays, src/rlSss.h:224-279):
//     rlsb::ProbeQueue pq(dev, n, spp_n);
//     rlsb::emitProbes(dev, sss, P, n, spp_n, seed, pq);                   // one probe ray per sample, dense
//     ... walk every ray through the object, fill an rls_probe_hits (count, P, N, irradiance per hit slot) ...
//     rlsb::resolveScatter(dev, sss, P, pq, hits, cavity, literal, result); // integrateScatter's result
// The irradiance of those hits through the renderer's tracer too (shadeProbeSample's light loop and diffuse ray, :415-418):
//     rlsb::HitQueues hq(dev, n, spp_n, hits.max_hits, hitCapacity, n_lights, hit_spp_n, traceDiffuse);
//     rlsb::emitHits(dev, sss, P, pq, hits, nullptr, cavity, lights, n_lights, seed, hq);   // hits.irradiance is not read
//     ... trace hq.c().shadow from the hits' positions for a visibility, hq.c().diffuse for a radiance ...
//     rlsb::resolveHits(dev, hits, lights, n_lights, hq, visibility, &radiance, E);    // E: what hits.irradiance points at
// The light loops (`while (AiLightsGetSample(sg))`, src/rlGgx.cpp:285-299, src/rlDisney.cpp:695-705):
//     rlsb::ShadowQueue sq(dev, n, n_lights, spp_n, rlsb::ShadowQueue::Ggx);
//     rlsb::emitDirect(dev, ggx, shader, P, lights, n_lights, n, spp_n, seed, sq);   // one shadow ray per term-carrying sample
//     ... trace ray k from P[point[k]] along dir[k] up to maxdist[k], one visibility per ray and channel (3 planes) ...
//     rlsb::resolveDirect(dev, ggx, shader, lights, n_lights, sq, visibility, directDiffuse, directSpecular);
// Whole nodes (shader_evaluate of rlGgx / rlDisney, every loop at once):
//     rlsb::GgxNodeQueues nq(dev, n, n_lights, spp_n);                     // shadow (with lights), glossy, refract, diffuse
//     rlsb::emitNode(dev, ggx, shader, P, lights, n_lights, traced, n, spp_n, seed, nq);
//     ... trace every queue: a visibility per shadow ray, a radiance per ray of the ray queues ...
//     rlsb::resolveNode(dev, ggx, shader, lights, n_lights, traced, nq, visibility, Lglossy, Lrefract, Ldiffuse, aovs, &out);
// The same nodes at the hits of secondary rays, the ray type and depth counters per point (RayState):
//     rlsb::emitBounce(dev, ggx, shader, P, lights, n_lights, n, spp_n, seed, state.c(), depths, nq);
//     rlsb::resolveBounce(dev, ggx, shader, lights, n_lights, state.c(), depths, nq, visibility, Lglossy, Lrefract, Ldiffuse, aovs, &out);
//     rlsb::advanceState(dev, rays, nq.glossy().c().point, state.c(), RLS_RT_GLOSSY, child);   // the state of those rays' hits
// The visibility of shadow rays from the opacities of the surfaces they cross (the nodes' opacity and shadow-ray branches):
//     rlsb::ggxOpacity(dev, sheet, m, hitState.c().ray_type, table.rgb());  // sg->out_opacity of m surfaces (also disney-, skinOpacity)
//     rlsb::ShadowHits hits(dev, rays, maxHits, rlsb::ShadowHits::Indexed); // the tracer fills hits.count() and hits.index()
//     rlsb::foldVisibility(dev, rays, hits.c(table, m), rlsb::Planes(), visibility);   // -> resolveDirect / resolveNode
// From one bounce to the next: the traced queue's hits split by the node they landed on, each node's batch gathered, its out put back:
//     rlsb::HitRoutes routes(dev, rays, bins);  rlsb::routeHits(dev, hitBin, routes);           // hitBin: one byte per ray
//     rlsb::gatherHits(dev, routes, b, rlsb::RoutePlanes().planes(hitP, P_b, 3).state(hitState.c(), state_b.c()));
//     ... emitBounce / trace / resolveBounce on routes.size(b) points per bin ...
//     rlsb::scatterToRays(dev, routes, b, rlsb::RoutePlanes().planes(out_b, radiance, 3));  rlsb::fillMisses(dev, routes, env, radiance);
// Nothing here synchronises the host except RayQueue::count(), ShadowQueue::count() (they read offsets[n]) and
// HitRoutes::bounds() (offsets, once per route).
#pragma once

#include <algorithm>
#include <cstdint>
#include <memory>
#include <vector>

#include "rls_batch.hpp"
#include "rlshaders_amd_trace.h"

namespace rlsb {

namespace detail {
// The device allocations of one queue object, freed together -- also when the object's constructor throws half way, this
// being a member of it.
class DeviceBuffers {
public:
    explicit DeviceBuffers(const Device &d) : dev_(&d) {}
    ~DeviceBuffers() { for (void *p : bufs_) rls_device_free(dev_->ctx(), p); }
    DeviceBuffers(const DeviceBuffers &) = delete;
    DeviceBuffers &operator=(const DeviceBuffers &) = delete;

    void *alloc(size_t bytes)
    {
        bufs_.reserve(bufs_.size() + 1);                    // (no throw between the allocation and its entry)
        void *p = nullptr;
        check(rls_device_alloc(dev_->ctx(), bytes > 0 ? bytes : 1, &p));
        bufs_.push_back(p);
        return p;
    }
    template <class T>
    T *alloc(int64_t count) { return static_cast<T *>(alloc(sizeof(T) * (size_t)count)); }
    rls_vec3 vec3(int64_t count) { return rls_vec3{alloc<float>(count), alloc<float>(count), alloc<float>(count)}; }
    // one count of a queue, an int64_t in device memory (synchronises)
    int64_t read(const int64_t *p) const
    {
        int64_t c = 0;
        check(rls_copy_to_host(dev_->ctx(), &c, p, sizeof(c)));
        return c;
    }

private:
    const Device *dev_;
    std::vector<void *> bufs_;
};

inline rls_crgb crgb(const Planes &p) { return p.empty() ? rls_crgb{nullptr, nullptr, nullptr} : rls_crgb{p.plane(0), p.plane(1), p.plane(2)}; }
template <class Q>
inline void checkNodeQueues(const Q &q, int64_t n, int n_lights, int spp_n, const char *who)
{
    if (q.points() != n || q.lights() != n_lights || q.sppN() != spp_n) throw Error(RLS_ERR_INVALID_ARGUMENT, who);
}
} // namespace detail

// The device buffers of one emit: per-ray planes for n * spp_n^2 rays, offsets [n + 1] and the emit's scratch.
class RayQueue {
public:
    // NodeDiffuse: the rlGgx node's Oren-Nayar queue -- one weight plane like Refract, no kind plane
    enum Kind { Glossy, Refract, DisneyDiffuse, DisneyGlossy, NodeDiffuse };

    RayQueue(const Device &d, int64_t n, int spp_n, Kind kind) : bufs_(d), n_(n), spp_n_(spp_n), kind_(kind)
    {
        const int64_t cap = n * spp_n * spp_n;
        size_t scratch = 0;
        check(rls_trace_scratch_bytes(n, spp_n, &scratch));
        q_.capacity = cap;
        q_.offsets = bufs_.alloc<int64_t>(n + 1);
        q_.dir = bufs_.vec3(cap);
        q_.weight.r = bufs_.alloc<float>(cap);
        if (kind != Refract && kind != NodeDiffuse) { q_.weight.g = bufs_.alloc<float>(cap); q_.weight.b = bufs_.alloc<float>(cap); }
        q_.point = bufs_.alloc<uint32_t>(cap);
        q_.sample = bufs_.alloc<uint8_t>(cap);
        if (kind == Refract) q_.kind = bufs_.alloc<uint8_t>(cap);
        q_.scratch = bufs_.alloc(scratch);
        q_.scratch_bytes = scratch;
    }
    RayQueue(const RayQueue &) = delete;
    RayQueue &operator=(const RayQueue &) = delete;

    const rls_ray_queue &c() const { return q_; }
    int64_t points() const { return n_; }
    int sppN() const { return spp_n_; }
    Kind kind() const { return kind_; }
    // offsets[n]: the number of rays (synchronises)
    int64_t count() const { return bufs_.read(q_.offsets + n_); }

private:
    detail::DeviceBuffers bufs_;
    int64_t n_;
    int spp_n_;
    Kind kind_;
    rls_ray_queue q_{};
};

// integrateGlossy's sample rays (src/rlGgx.h:172-179); avgReflectWeight: n floats (getAvgReflectWeight, :181-184) or nullptr
inline void emitGlossy(const Device &d, const rls_ggx_closure &c, int64_t n, int spp_n, uint32_t seed, RayQueue &q,
                       float *avgReflectWeight = nullptr, uint64_t first_index = 0)
{
    if (q.kind() != RayQueue::Glossy)
        throw Error(RLS_ERR_INVALID_ARGUMENT, q.kind() == RayQueue::Refract ? "emitGlossy: a refraction queue"
                                                                           : "emitGlossy: an rlDisney queue");
    check(rls_trace_ggx_glossy_emit(d.ctx(), n, &c, spp_n, seed, first_index, &q.c(), avgReflectWeight));
}

// integrateRefract's sample rays (src/rlGgx.h:228-241); tirFraction: n floats or nullptr
inline void emitRefract(const Device &d, const rls_ggx_closure &c, int64_t n, int spp_n, uint32_t seed, RayQueue &q,
                        float *tirFraction = nullptr, uint64_t first_index = 0)
{
    if (q.kind() != RayQueue::Refract)
        throw Error(RLS_ERR_INVALID_ARGUMENT, q.kind() == RayQueue::Glossy ? "emitRefract: a glossy queue"
                                                                          : "emitRefract: an rlDisney queue");
    check(rls_trace_ggx_refract_emit(d.ctx(), n, &c, spp_n, seed, first_index, &q.c(), tirFraction));
}

// the sample rays of one rlDisney lobe (src/rlDisney.cpp:240-243, 279-283): lobe RLS_RAY_DIFFUSE into a DisneyDiffuse
// queue, RLS_RAY_GLOSSY into a DisneyGlossy one; validCount: n floats (rls_disney_integrate's count for the lobe) or nullptr
inline void emitDisney(const Device &d, const rls_disney_closure &c, int lobe, int64_t n, int spp_n, uint32_t seed,
                       RayQueue &q, float *validCount = nullptr, uint64_t first_index = 0)
{
    const RayQueue::Kind want = lobe == RLS_RAY_DIFFUSE ? RayQueue::DisneyDiffuse : RayQueue::DisneyGlossy;
    if (q.kind() != want) throw Error(RLS_ERR_INVALID_ARGUMENT, "emitDisney: a queue of another integrator or lobe");
    check(rls_trace_disney_emit(d.ctx(), n, &c, lobe, spp_n, seed, first_index, &q.c(), validCount));
}

// a Glossy, DisneyDiffuse or DisneyGlossy queue; radiance: 3 planes of >= q.count() floats, one per ray; out: 3 planes of
// n floats
inline void resolveGlossy(const Device &d, const RayQueue &q, const Planes &radiance, Planes &sum)
{
    check(rls_trace_ggx_glossy_resolve(d.ctx(), q.points(), &q.c(), detail::crgb(radiance), sum.rgb()));
}

inline void resolveRefract(const Device &d, const RayQueue &q, const Planes &radiance, Planes &result)
{
    check(rls_trace_ggx_refract_resolve(d.ctx(), q.points(), &q.c(), q.sppN(), detail::crgb(radiance), result.rgb()));
}

// integrateScatter's probe rays: n * spp_n^2 rays, ray j = i * spp_n^2 + s (no compaction: count() is known on the host)
class ProbeQueue {
public:
    ProbeQueue(const Device &d, int64_t n, int spp_n) : bufs_(d), n_(n), spp_n_(spp_n)
    {
        const int64_t cap = n * spp_n * spp_n;
        q_.capacity = cap;
        q_.offsets = bufs_.alloc<int64_t>(n + 1);
        q_.origin = bufs_.vec3(cap);
        q_.dir = bufs_.vec3(cap);
        q_.maxdist = bufs_.alloc<float>(cap);
        q_.point = bufs_.alloc<uint32_t>(cap);
        q_.sample = bufs_.alloc<uint8_t>(cap);
    }
    ProbeQueue(const ProbeQueue &) = delete;
    ProbeQueue &operator=(const ProbeQueue &) = delete;

    const rls_probe_queue &c() const { return q_; }
    int64_t points() const { return n_; }
    int sppN() const { return spp_n_; }
    int64_t count() const { return q_.capacity; }

private:
    detail::DeviceBuffers bufs_;
    int64_t n_;
    int spp_n_;
    rls_probe_queue q_{};
};

// integrateScatter's probe rays (getProbeRay, src/rlSss.h:224-228); P: 3 planes of n floats, sg->P
inline void emitProbes(const Device &d, const rls_sss_closure &c, const Planes &P, int64_t n, int spp_n, uint32_t seed,
                       ProbeQueue &q, uint64_t first_index = 0)
{
    if (q.points() != n || q.sppN() != spp_n) throw Error(RLS_ERR_INVALID_ARGUMENT, "emitProbes: a queue of another size");
    check(rls_trace_sss_probe_emit(d.ctx(), n, &c, P.cvec3(), spp_n, seed,
                                   first_index, &q.c()));
}

// integrateScatter's combination of the caller's hits (src/rlSss.h:245-279); c and P those of the emit; result: 3 planes
// of n floats; meanDepth: n floats or nullptr
inline void resolveScatter(const Device &d, const rls_sss_closure &c, const Planes &P, const ProbeQueue &q,
                           const rls_probe_hits &hits, bool cavityFade, bool literalMatrix, Planes &result,
                           float *meanDepth = nullptr)
{
    check(rls_trace_sss_scatter_resolve(d.ctx(), q.points(), &c, P.cvec3(), q.sppN(),
                                        &q.c(), &hits, cavityFade ? 1 : 0, literalMatrix ? 1 : 0, result.rgb(),
                                        meanDepth));
}

// The shaded probe hits of one emitHits and the rays leaving them (rls_hit_queues): the list (hit_count, hit_element), the
// light loop's shadow queue over the list (no weight_specular; absent without lights), integrateDiffuse's ray queue (with
// traceDiffuse) and the scratch.  hitCapacity: the hits the list holds; max_hits * n * spp_n^2 holds every slot.
class HitQueues {
public:
    HitQueues(const Device &d, int64_t n, int spp_n, int max_hits, int64_t hitCapacity, int n_lights, int hit_spp_n,
              bool traceDiffuse)
        : bufs_(d), n_(n), spp_n_(spp_n), n_lights_(n_lights), hit_spp_n_(hit_spp_n), diffuse_(traceDiffuse)
    {
        size_t scratch = 0;
        check(rls_trace_sss_hits_scratch_bytes(n, spp_n, max_hits, hitCapacity, n_lights, hit_spp_n, &scratch));
        const int64_t cap = hitCapacity, scap = cap * n_lights * 2 * hit_spp_n * hit_spp_n;
        q_.hit_capacity = cap;
        q_.hit_count = bufs_.alloc<int64_t>(1);
        q_.hit_element = bufs_.alloc<int64_t>(cap);
        if (n_lights > 0) {
            rls_shadow_queue &s = q_.shadow;
            s.capacity = scap;
            s.offsets = bufs_.alloc<int64_t>(cap + 1);
            s.dir = bufs_.vec3(scap);
            s.maxdist = bufs_.alloc<float>(scap);
            s.weight_diffuse.r = bufs_.alloc<float>(scap);
            s.kind = bufs_.alloc<uint8_t>(scap);
            s.point = bufs_.alloc<uint32_t>(scap);
            s.sample = bufs_.alloc<uint8_t>(scap);
        }
        if (traceDiffuse) {
            rls_ray_queue &r = q_.diffuse;
            r.capacity = cap;
            r.offsets = bufs_.alloc<int64_t>(cap + 1);
            r.dir = bufs_.vec3(cap);
            r.weight.r = bufs_.alloc<float>(cap);
            r.point = bufs_.alloc<uint32_t>(cap);
        }
        q_.scratch = bufs_.alloc(scratch);
        q_.scratch_bytes = scratch;
    }
    HitQueues(const HitQueues &) = delete;
    HitQueues &operator=(const HitQueues &) = delete;

    const rls_hit_queues &c() const { return q_; }
    int64_t points() const { return n_; }
    int sppN() const { return spp_n_; }
    int lights() const { return n_lights_; }
    int hitSppN() const { return hit_spp_n_; }
    bool traceDiffuse() const { return diffuse_; }
    // the TRUE number of shaded hits, the shadow rays, the diffuse rays (each synchronises)
    int64_t hitCount() const { return bufs_.read(q_.hit_count); }
    int64_t listed() const { const int64_t c = hitCount(); return c < q_.hit_capacity ? c : q_.hit_capacity; }
    int64_t shadowCount() const { return n_lights_ > 0 ? bufs_.read(q_.shadow.offsets + q_.hit_capacity) : 0; }
    int64_t diffuseCount() const { return diffuse_ ? bufs_.read(q_.diffuse.offsets + q_.hit_capacity) : 0; }

private:
    detail::DeviceBuffers bufs_;
    int64_t n_;
    int spp_n_, n_lights_, hit_spp_n_;
    bool diffuse_;
    rls_hit_queues q_{};
};

// shadeProbeSample's rays at the caller's hits (src/rlSss.h:415-418): c, P, q, cavityFade those of the scatter resolve the
// hits go to; hits: count, P, N (irradiance is not read); hitT: the tangents at the hits, 3 planes in the hits' layout, or
// nullptr for the library's own; the hit with element e samples from hash(seed, hit_first_index + e)
inline void emitHits(const Device &d, const rls_sss_closure &c, const Planes &P, const ProbeQueue &q, const rls_probe_hits &hits,
                     const Planes *hitT, bool cavityFade, const rls_sphere_light *lights, int n_lights, uint32_t seed,
                     HitQueues &hq, uint64_t hit_first_index = 0)
{
    if (hq.points() != q.points() || hq.sppN() != q.sppN() || hq.lights() != n_lights)
        throw Error(RLS_ERR_INVALID_ARGUMENT, "emitHits: queues of another size or light count");
    const rls_cvec3 T = hitT ? hitT->cvec3() : rls_cvec3{nullptr, nullptr, nullptr};
    check(rls_trace_sss_hits_emit(d.ctx(), q.points(), &c, P.cvec3(), q.sppN(), &q.c(), &hits,
                                  T, cavityFade ? 1 : 0, lights, n_lights, hq.hitSppN(), hq.traceDiffuse() ? 1 : 0, seed,
                                  hit_first_index, &hq.c()));
}

// E at every hit slot from what the renderer traced: visibility 3 planes of >= hq.shadowCount() floats (not read without
// lights), radiance 3 planes of >= hq.diffuseCount() floats or nullptr without traceDiffuse; E: 3 planes of max_hits * stride
// floats, the layout of hits.irradiance (exactly 0 at every hit that is not listed)
inline void resolveHits(const Device &d, const rls_probe_hits &hits, const rls_sphere_light *lights, int n_lights,
                        const HitQueues &hq, const Planes &visibility, const Planes *radiance, Planes &E)
{
    if (hq.lights() != n_lights) throw Error(RLS_ERR_INVALID_ARGUMENT, "resolveHits: queues of another light count");
    const rls_crgb L = radiance ? detail::crgb(*radiance) : rls_crgb{nullptr, nullptr, nullptr};
    check(rls_trace_sss_hits_resolve(d.ctx(), &hits, lights, n_lights, hq.hitSppN(), hq.traceDiffuse() ? 1 : 0, &hq.c(),
                                     detail::crgb(visibility), L, E.rgb()));
}

// The device buffers of one light-loop emit (rls_shadow_queue): per-ray planes for n * n_lights * 3 * spp_n^2 rays, offsets
// [n + 1] and the emit's scratch.  Ggx: weight_diffuse is its .r plane alone.  Skin: a lobe's light loop of the rlSkin node --
// no weight_diffuse, two rays a sample at most (n * n_lights * 2 * spp_n^2 rays).  SkinScatter: integrateScatter's Oren-Nayar
// light loop at the diffuse rays' points of an rlSkin bounce emit -- Skin's capacity, weight_diffuse.r alone, no weight_specular.
class ShadowQueue {
public:
    enum Node { Ggx, Disney, Skin, SkinScatter };

    ShadowQueue(const Device &d, int64_t n, int n_lights, int spp_n, Node node)
        : bufs_(d), n_(n), n_lights_(n_lights), spp_n_(spp_n), node_(node)
    {
        const int64_t cap = n * n_lights * (node == Skin || node == SkinScatter ? 2 : 3) * spp_n * spp_n;
        size_t scratch = 0;
        check(rls_trace_shadow_scratch_bytes(n, n_lights, spp_n, &scratch));
        q_.capacity = cap;
        q_.offsets = bufs_.alloc<int64_t>(n + 1);
        q_.dir = bufs_.vec3(cap);
        q_.maxdist = bufs_.alloc<float>(cap);
        if (node != SkinScatter) q_.weight_specular = rls_rgb{bufs_.alloc<float>(cap), bufs_.alloc<float>(cap), bufs_.alloc<float>(cap)};
        if (node != Skin) q_.weight_diffuse.r = bufs_.alloc<float>(cap);
        if (node == Disney) { q_.weight_diffuse.g = bufs_.alloc<float>(cap); q_.weight_diffuse.b = bufs_.alloc<float>(cap); }
        q_.kind = bufs_.alloc<uint8_t>(cap);
        q_.point = bufs_.alloc<uint32_t>(cap);
        q_.sample = bufs_.alloc<uint8_t>(cap);
        q_.scratch = bufs_.alloc(scratch);
        q_.scratch_bytes = scratch;
    }
    ShadowQueue(const ShadowQueue &) = delete;
    ShadowQueue &operator=(const ShadowQueue &) = delete;

    const rls_shadow_queue &c() const { return q_; }
    int64_t points() const { return n_; }
    int lights() const { return n_lights_; }
    int sppN() const { return spp_n_; }
    Node node() const { return node_; }
    // offsets[n]: the number of rays (synchronises)
    int64_t count() const { return bufs_.read(q_.offsets + n_); }

private:
    detail::DeviceBuffers bufs_;
    int64_t n_;
    int n_lights_, spp_n_;
    Node node_;
    rls_shadow_queue q_{};
};

inline void checkShadowQueue(const ShadowQueue &q, ShadowQueue::Node node, int64_t n, int n_lights, int spp_n, const char *who)
{
    if (q.node() != node || q.points() != n || q.lights() != n_lights || q.sppN() != spp_n)
        throw Error(RLS_ERR_INVALID_ARGUMENT, who);
}

// the shadow rays of rlGgx's light loop (src/rlGgx.cpp:285-299): the arguments of rls_ggx_direct_lighting; P: 3 planes of n
// floats, sg->P
inline void emitDirect(const Device &d, const rls_ggx_closure &c, const rls_ggx_shader &sh, const Planes &P,
                       const rls_sphere_light *lights, int n_lights, int64_t n, int spp_n, uint32_t seed, ShadowQueue &q,
                       uint64_t first_index = 0)
{
    checkShadowQueue(q, ShadowQueue::Ggx, n, n_lights, spp_n, "emitDirect: a queue of another node, size or light count");
    check(rls_trace_ggx_direct_emit(d.ctx(), n, &c, &sh, P.cvec3(), lights, n_lights,
                                    spp_n, seed, first_index, &q.c()));
}

// the shadow rays of rlDisney's light loop (src/rlDisney.cpp:695-705): the arguments of rls_disney_direct_lighting
inline void emitDirect(const Device &d, const rls_disney_closure &c, const Planes &P, const rls_sphere_light *lights,
                       int n_lights, int64_t n, int spp_n, uint32_t seed, ShadowQueue &q, uint64_t first_index = 0)
{
    checkShadowQueue(q, ShadowQueue::Disney, n, n_lights, spp_n, "emitDirect: a queue of another node, size or light count");
    check(rls_trace_disney_direct_emit(d.ctx(), n, &c, P.cvec3(), lights, n_lights, spp_n,
                                       seed, first_index, &q.c()));
}

// the light loop's AOVs with the traced visibility: 3 planes of >= q.count() floats, one per ray and channel; c, sh, lights:
// those of the emit; directDiffuse, directSpecular: 3 planes of n floats each
inline void resolveDirect(const Device &d, const rls_ggx_closure &c, const rls_ggx_shader &sh, const rls_sphere_light *lights,
                          int n_lights, const ShadowQueue &q, const Planes &visibility, Planes &directDiffuse,
                          Planes &directSpecular)
{
    checkShadowQueue(q, ShadowQueue::Ggx, q.points(), n_lights, q.sppN(), "resolveDirect: a queue of another node or light count");
    check(rls_trace_ggx_direct_resolve(d.ctx(), q.points(), &c, &sh, lights, n_lights, q.sppN(), &q.c(), detail::crgb(visibility),
                                       directDiffuse.rgb(), directSpecular.rgb()));
}

inline void resolveDirect(const Device &d, const rls_sphere_light *lights, int n_lights, const ShadowQueue &q,
                          const Planes &visibility, Planes &directDiffuse, Planes &directSpecular)
{
    checkShadowQueue(q, ShadowQueue::Disney, q.points(), n_lights, q.sppN(), "resolveDirect: a queue of another node or light count");
    check(rls_trace_disney_direct_resolve(d.ctx(), q.points(), lights, n_lights, q.sppN(), &q.c(), detail::crgb(visibility),
                                          directDiffuse.rgb(), directSpecular.rgb()));
}

// The queues of a whole-node emit (rls_ggx_node_queues): the light loop's shadow queue (none with n_lights == 0) and one ray
// queue per indirect loop.  Each queue owns its scratch.
class GgxNodeQueues {
public:
    GgxNodeQueues(const Device &d, int64_t n, int n_lights, int spp_n)
        : n_(n), n_lights_(n_lights), spp_n_(spp_n), shadow_(n_lights > 0 ? new ShadowQueue(d, n, n_lights, spp_n, ShadowQueue::Ggx) : nullptr),
          glossy_(d, n, spp_n, RayQueue::Glossy), refract_(d, n, spp_n, RayQueue::Refract), diffuse_(d, n, spp_n, RayQueue::NodeDiffuse)
    {
        q_.shadow = shadow_ ? &shadow_->c() : nullptr;
        q_.glossy = &glossy_.c(); q_.refract = &refract_.c(); q_.diffuse = &diffuse_.c();
    }
    GgxNodeQueues(const GgxNodeQueues &) = delete;
    GgxNodeQueues &operator=(const GgxNodeQueues &) = delete;

    const rls_ggx_node_queues &c() const { return q_; }
    const ShadowQueue *shadow() const { return shadow_.get(); }    // nullptr without lights
    const RayQueue &glossy() const { return glossy_; }
    const RayQueue &refract() const { return refract_; }
    const RayQueue &diffuse() const { return diffuse_; }
    int64_t points() const { return n_; }
    int lights() const { return n_lights_; }
    int sppN() const { return spp_n_; }

private:
    int64_t n_;
    int n_lights_, spp_n_;
    std::unique_ptr<ShadowQueue> shadow_;
    RayQueue glossy_, refract_, diffuse_;
    rls_ggx_node_queues q_{};
};

// rls_disney_node_queues: the shadow queue (none with n_lights == 0), integrateDiffuse's and integrateGlossy's queues
class DisneyNodeQueues {
public:
    DisneyNodeQueues(const Device &d, int64_t n, int n_lights, int spp_n)
        : n_(n), n_lights_(n_lights), spp_n_(spp_n),
          shadow_(n_lights > 0 ? new ShadowQueue(d, n, n_lights, spp_n, ShadowQueue::Disney) : nullptr),
          diffuse_(d, n, spp_n, RayQueue::DisneyDiffuse), specular_(d, n, spp_n, RayQueue::DisneyGlossy)
    {
        q_.shadow = shadow_ ? &shadow_->c() : nullptr;
        q_.diffuse = &diffuse_.c(); q_.specular = &specular_.c();
    }
    DisneyNodeQueues(const DisneyNodeQueues &) = delete;
    DisneyNodeQueues &operator=(const DisneyNodeQueues &) = delete;

    const rls_disney_node_queues &c() const { return q_; }
    const ShadowQueue *shadow() const { return shadow_.get(); }
    const RayQueue &diffuse() const { return diffuse_; }
    const RayQueue &specular() const { return specular_; }
    int64_t points() const { return n_; }
    int lights() const { return n_lights_; }
    int sppN() const { return spp_n_; }

private:
    int64_t n_;
    int n_lights_, spp_n_;
    std::unique_ptr<ShadowQueue> shadow_;
    RayQueue diffuse_, specular_;
    rls_disney_node_queues q_{};
};

// rls_skin_node_queues: per GGX lobe the light loop's shadow queue (none with n_lights == 0) and integrateGlossy's queue,
// integrateScatter's probe queue, and the three hand-down scalars (n floats each), which the emit writes and the resolve reads
class SkinNodeQueues {
public:
    SkinNodeQueues(const Device &d, int64_t n, int n_lights, int spp_n)
        : n_(n), n_lights_(n_lights), spp_n_(spp_n),
          sheen_shadow_(n_lights > 0 ? new ShadowQueue(d, n, n_lights, spp_n, ShadowQueue::Skin) : nullptr),
          specular_shadow_(n_lights > 0 ? new ShadowQueue(d, n, n_lights, spp_n, ShadowQueue::Skin) : nullptr),
          sheen_glossy_(d, n, spp_n, RayQueue::Glossy), specular_glossy_(d, n, spp_n, RayQueue::Glossy), probes_(d, n, spp_n),
          scalars_(d, n, 3)
    {
        q_.sheen_shadow = sheen_shadow_ ? &sheen_shadow_->c() : nullptr;
        q_.specular_shadow = specular_shadow_ ? &specular_shadow_->c() : nullptr;
        q_.sheen_glossy = &sheen_glossy_.c(); q_.specular_glossy = &specular_glossy_.c(); q_.probes = &probes_.c();
        q_.sheenFresnel = scalars_.plane(0); q_.specularFresnel = scalars_.plane(1); q_.sssWeight = scalars_.plane(2);
    }
    SkinNodeQueues(const SkinNodeQueues &) = delete;
    SkinNodeQueues &operator=(const SkinNodeQueues &) = delete;

    const rls_skin_node_queues &c() const { return q_; }
    const ShadowQueue *sheenShadow() const { return sheen_shadow_.get(); }    // nullptr without lights
    const ShadowQueue *specularShadow() const { return specular_shadow_.get(); }
    const RayQueue &sheenGlossy() const { return sheen_glossy_; }
    const RayQueue &specularGlossy() const { return specular_glossy_; }
    const ProbeQueue &probes() const { return probes_; }
    const Planes &scalars() const { return scalars_; }            // sheenFresnel, specularFresnel, sssWeight
    int64_t points() const { return n_; }
    int lights() const { return n_lights_; }
    int sppN() const { return spp_n_; }

private:
    int64_t n_;
    int n_lights_, spp_n_;
    std::unique_ptr<ShadowQueue> sheen_shadow_, specular_shadow_;
    RayQueue sheen_glossy_, specular_glossy_;
    ProbeQueue probes_;
    Planes scalars_;
    rls_skin_node_queues q_{};
};

// rls_skin_bounce_queues: the node's queues and the shadow queue of integrateScatter's light loop at the diffuse rays' points
// (none with n_lights == 0)
class SkinBounceQueues {
public:
    SkinBounceQueues(const Device &d, int64_t n, int n_lights, int spp_n)
        : node_(d, n, n_lights, spp_n),
          diffuse_shadow_(n_lights > 0 ? new ShadowQueue(d, n, n_lights, spp_n, ShadowQueue::SkinScatter) : nullptr)
    {
        q_.node = node_.c();
        q_.diffuse_shadow = diffuse_shadow_ ? &diffuse_shadow_->c() : nullptr;
    }
    SkinBounceQueues(const SkinBounceQueues &) = delete;
    SkinBounceQueues &operator=(const SkinBounceQueues &) = delete;

    const rls_skin_bounce_queues &c() const { return q_; }
    const SkinNodeQueues &node() const { return node_; }
    const ShadowQueue *diffuseShadow() const { return diffuse_shadow_.get(); } // nullptr without lights
    int64_t points() const { return node_.points(); }
    int lights() const { return node_.lights(); }
    int sppN() const { return node_.sppN(); }

private:
    SkinNodeQueues node_;
    std::unique_ptr<ShadowQueue> diffuse_shadow_;
    rls_skin_bounce_queues q_{};
};

// what resolveNode and resolveBounce of a node both fill: the traced struct from the caller's planes, the AOV struct from aovs
// (the planes in the struct's order, 3 each) and out (sg->out.RGB or nullptr)
namespace detail {
inline rls_ggx_node_traced ggxTraced(const Planes &visibility, const Planes &glossy, const Planes &refract, const Planes &diffuse)
{
    return rls_ggx_node_traced{crgb(visibility), crgb(glossy), crgb(refract), crgb(diffuse)};
}
inline rls_ggx_shade_out ggxOut(Planes &aovs, Planes *out)
{
    rls_ggx_shade_out o = {};
    o.direct_diffuse = aovs.rgb(0); o.direct_specular = aovs.rgb(3); o.refraction = aovs.rgb(6);
    o.indirect_diffuse = aovs.rgb(9); o.indirect_specular = aovs.rgb(12);
    if (out) o.out = out->rgb();
    return o;
}
inline rls_disney_node_traced disneyTraced(const Planes &visibility, const Planes &diffuse, const Planes &specular)
{
    return rls_disney_node_traced{crgb(visibility), crgb(diffuse), crgb(specular)};
}
inline rls_disney_shade_out disneyOut(Planes &aovs, Planes *out)
{
    rls_disney_shade_out o = {};
    o.direct_diffuse = aovs.rgb(0); o.direct_specular = aovs.rgb(3); o.indirect_diffuse = aovs.rgb(6);
    o.indirect_specular = aovs.rgb(9);
    if (out) o.out = out->rgb();
    return o;
}
inline rls_skin_node_traced skinTraced(const Planes &sheenVisibility, const Planes &specularVisibility, const Planes &sheenGlossy,
                                       const Planes &specularGlossy, const rls_probe_hits &hits)
{
    return rls_skin_node_traced{crgb(sheenVisibility), crgb(specularVisibility), crgb(sheenGlossy), crgb(specularGlossy), &hits};
}
inline rls_skin_integrate_out skinOut(Planes &aovs, Planes *out)
{
    rls_skin_integrate_out o = {};
    o.sheen = aovs.rgb(0); o.specular = aovs.rgb(3); o.sss = aovs.rgb(6);
    if (out) o.out = out->rgb();
    return o;
}
} // namespace detail

// every ray of rlGgx's shader_evaluate as rls_ggx_shade samples it (rls_trace_ggx_shade_emit): the arguments of rls_ggx_shade
// without env; traced false: the one ray of integrateRefract's untraced branch
inline void emitNode(const Device &d, const rls_ggx_closure &c, const rls_ggx_shader &sh, const Planes &P,
                     const rls_sphere_light *lights, int n_lights, bool traced, int64_t n, int spp_n, uint32_t seed,
                     GgxNodeQueues &q, uint64_t first_index = 0)
{
    detail::checkNodeQueues(q, n, n_lights, spp_n, "emitNode: queues of another size or light count");
    check(rls_trace_ggx_shade_emit(d.ctx(), n, &c, &sh, P.cvec3(), lights, n_lights,
                                   traced ? 1 : 0, spp_n, seed, first_index, &q.c()));
}

// every ray of rlDisney's shader_evaluate as rls_disney_shade samples it (rls_trace_disney_shade_emit)
inline void emitNode(const Device &d, const rls_disney_closure &c, const Planes &P, const rls_sphere_light *lights,
                     int n_lights, int64_t n, int spp_n, uint32_t seed, DisneyNodeQueues &q, uint64_t first_index = 0)
{
    detail::checkNodeQueues(q, n, n_lights, spp_n, "emitNode: queues of another size or light count");
    check(rls_trace_disney_shade_emit(d.ctx(), n, &c, P.cvec3(), lights, n_lights, spp_n,
                                      seed, first_index, &q.c()));
}

// rls_ggx_shade's AOVs from what the renderer traced.  visibility (an empty Planes without lights) and the three radiances:
// 3 planes of >= the queue's count floats each.  aovs: 15 planes of n floats -- direct_diffuse, direct_specular, refraction,
// indirect_diffuse, indirect_specular, 3 each; out: sg->out.RGB, 3 planes of n floats, or nullptr
inline void resolveNode(const Device &d, const rls_ggx_closure &c, const rls_ggx_shader &sh, const rls_sphere_light *lights,
                        int n_lights, bool traced, const GgxNodeQueues &q, const Planes &visibility, const Planes &glossy,
                        const Planes &refract, const Planes &diffuse, Planes &aovs, Planes *out = nullptr)
{
    detail::checkNodeQueues(q, q.points(), n_lights, q.sppN(), "resolveNode: queues of another light count");
    const rls_ggx_node_traced t = detail::ggxTraced(visibility, glossy, refract, diffuse);
    const rls_ggx_shade_out o = detail::ggxOut(aovs, out);
    check(rls_trace_ggx_shade_resolve(d.ctx(), q.points(), &c, &sh, lights, n_lights, traced ? 1 : 0, q.sppN(), &q.c(), &t, &o));
}

// rls_disney_shade's AOVs.  aovs: 12 planes -- direct_diffuse, direct_specular, indirect_diffuse, indirect_specular
inline void resolveNode(const Device &d, const rls_sphere_light *lights, int n_lights, const DisneyNodeQueues &q,
                        const Planes &visibility, const Planes &diffuse, const Planes &specular, Planes &aovs,
                        Planes *out = nullptr)
{
    detail::checkNodeQueues(q, q.points(), n_lights, q.sppN(), "resolveNode: queues of another light count");
    const rls_disney_node_traced t = detail::disneyTraced(visibility, diffuse, specular);
    const rls_disney_shade_out o = detail::disneyOut(aovs, out);
    check(rls_trace_disney_shade_resolve(d.ctx(), q.points(), lights, n_lights, q.sppN(), &q.c(), &t, &o));
}

// sg->Rt and the sg->Rr* counters of n shading points (rls_ray_state): five planes of n bytes in one device allocation, in the
// struct's order -- ray_type, Rr, Rr_diff, Rr_gloss, Rr_refr
class RayState {
public:
    RayState(const Device &d, int64_t n) : dev_(&d), n_(n)
    {
        void *p = nullptr;
        check(rls_device_alloc(d.ctx(), (size_t)(5 * n > 0 ? 5 * n : 1), &p));
        ptr_ = static_cast<uint8_t *>(p);
    }
    // host: 5 * n bytes, plane by plane
    RayState(const Device &d, const std::vector<uint8_t> &host) : RayState(d, (int64_t)(host.size() / 5))
    {
        if (!host.empty()) check(rls_copy_to_device(d.ctx(), ptr_, host.data(), host.size()));
    }
    // camera rays at depth 0
    static RayState camera(const Device &d, int64_t n)
    {
        std::vector<uint8_t> h((size_t)(5 * n), 0);
        std::fill(h.begin(), h.begin() + (size_t)n, (uint8_t)RLS_RT_CAMERA);
        return RayState(d, h);
    }
    ~RayState() { if (ptr_) rls_device_free(dev_->ctx(), ptr_); }
    RayState(RayState &&o) noexcept : dev_(o.dev_), ptr_(o.ptr_), n_(o.n_) { o.ptr_ = nullptr; }
    RayState(const RayState &) = delete;
    RayState &operator=(const RayState &) = delete;

    // the planes from point `first` on: the state of a chunk, or of the first points of a longer state
    rls_ray_state c(int64_t first = 0) const
    {
        return rls_ray_state{plane(0) + first, plane(1) + first, plane(2) + first, plane(3) + first, plane(4) + first};
    }
    uint8_t *plane(int k) const { return ptr_ + (size_t)k * (size_t)n_; }
    int64_t points() const { return n_; }
    std::vector<uint8_t> download() const
    {
        std::vector<uint8_t> h((size_t)(5 * n_));
        if (!h.empty()) check(rls_copy_to_host(dev_->ctx(), h.data(), ptr_, h.size()));
        return h;
    }

private:
    const Device *dev_;
    uint8_t *ptr_ = nullptr;
    int64_t n_;
};

// rlGgx / rlDisney at the hits of secondary rays (rls_trace_ggx_bounce_emit / rls_trace_disney_bounce_emit): emitNode with the
// ray state per point and the options' GI depths in place of `traced`; state: n points' planes (RayState::c)
inline void emitBounce(const Device &d, const rls_ggx_closure &c, const rls_ggx_shader &sh, const Planes &P,
                       const rls_sphere_light *lights, int n_lights, int64_t n, int spp_n, uint32_t seed,
                       const rls_ray_state &state, const rls_gi_depths &depths, GgxNodeQueues &q, uint64_t first_index = 0)
{
    detail::checkNodeQueues(q, n, n_lights, spp_n, "emitBounce: queues of another size or light count");
    check(rls_trace_ggx_bounce_emit(d.ctx(), n, &c, &sh, P.cvec3(), lights, n_lights, spp_n,
                                    seed, first_index, &state, &depths, &q.c()));
}
inline void emitBounce(const Device &d, const rls_disney_closure &c, const Planes &P, const rls_sphere_light *lights,
                       int n_lights, int64_t n, int spp_n, uint32_t seed, const rls_ray_state &state,
                       const rls_gi_depths &depths, DisneyNodeQueues &q, uint64_t first_index = 0)
{
    detail::checkNodeQueues(q, n, n_lights, spp_n, "emitBounce: queues of another size or light count");
    check(rls_trace_disney_bounce_emit(d.ctx(), n, &c, P.cvec3(), lights, n_lights, spp_n,
                                       seed, first_index, &state, &depths, &q.c()));
}

// resolveNode under the emit's state and depths: planes as there
inline void resolveBounce(const Device &d, const rls_ggx_closure &c, const rls_ggx_shader &sh, const rls_sphere_light *lights,
                          int n_lights, const rls_ray_state &state, const rls_gi_depths &depths, const GgxNodeQueues &q,
                          const Planes &visibility, const Planes &glossy, const Planes &refract, const Planes &diffuse,
                          Planes &aovs, Planes *out = nullptr)
{
    detail::checkNodeQueues(q, q.points(), n_lights, q.sppN(), "resolveBounce: queues of another light count");
    const rls_ggx_node_traced t = detail::ggxTraced(visibility, glossy, refract, diffuse);
    const rls_ggx_shade_out o = detail::ggxOut(aovs, out);
    check(rls_trace_ggx_bounce_resolve(d.ctx(), q.points(), &c, &sh, lights, n_lights, q.sppN(), &state, &depths, &q.c(), &t, &o));
}
// rlDisney: c as the emit took it (its materials index serves the scales), the node's indirectDiffuseScale / indirectSpecularScale
inline void resolveBounce(const Device &d, const rls_disney_closure &c, rls_param indirectDiffuseScale,
                          rls_param indirectSpecularScale, const rls_sphere_light *lights, int n_lights,
                          const rls_ray_state &state, const rls_gi_depths &depths, const DisneyNodeQueues &q,
                          const Planes &visibility, const Planes &diffuse, const Planes &specular, Planes &aovs,
                          Planes *out = nullptr)
{
    detail::checkNodeQueues(q, q.points(), n_lights, q.sppN(), "resolveBounce: queues of another light count");
    const rls_disney_node_traced t = detail::disneyTraced(visibility, diffuse, specular);
    const rls_disney_shade_out o = detail::disneyOut(aovs, out);
    check(rls_trace_disney_bounce_resolve(d.ctx(), q.points(), &c, indirectDiffuseScale, indirectSpecularScale, lights, n_lights,
                                          q.sppN(), &state, &depths, &q.c(), &t, &o));
}

// the state of the hits of a queue's `rays` rays (rls_trace_ray_state_advance): point: the queue's point plane; parent: the state
// the queue was emitted under; ray_type: the RLS_RT_* bits of its rays; child: >= rays points
inline void advanceState(const Device &d, int64_t rays, const uint32_t *point, const rls_ray_state &parent, int ray_type,
                         RayState &child)
{
    if (child.points() < rays) throw Error(RLS_ERR_INVALID_ARGUMENT, "advanceState: child holds fewer points than the queue has rays");
    const rls_ray_state cs = child.c();
    check(rls_trace_ray_state_advance(d.ctx(), rays, point, &parent, ray_type, &cs));
}

// every ray of rlSkin's shader_evaluate as rls_skin_integrate samples it (rls_trace_skin_emit): the arguments of
// rls_skin_integrate without scene and env
inline void emitNode(const Device &d, const rls_skin_closure &c, const Planes &P, const rls_sphere_light *lights, int n_lights,
                     int64_t n, int spp_n, uint32_t seed, SkinNodeQueues &q, uint64_t first_index = 0)
{
    detail::checkNodeQueues(q, n, n_lights, spp_n, "emitNode: queues of another size or light count");
    check(rls_trace_skin_emit(d.ctx(), n, &c, P.cvec3(), lights, n_lights, spp_n, seed,
                              first_index, &q.c()));
}

// rls_skin_integrate's AOVs from what the renderer traced.  The visibilities (empty Planes without lights) and the radiances:
// 3 planes of >= the queue's count floats each; hits: as resolveScatter takes them.  aovs: 9 planes of n floats -- sheen,
// specular, sss; out: sg->out.RGB, 3 planes of n floats, or nullptr
inline void resolveNode(const Device &d, const rls_skin_closure &c, const Planes &P, const rls_sphere_light *lights, int n_lights,
                        const SkinNodeQueues &q, const Planes &sheenVisibility, const Planes &specularVisibility,
                        const Planes &sheenGlossy, const Planes &specularGlossy, const rls_probe_hits &hits, bool cavityFade,
                        bool literalMatrix, Planes &aovs, Planes *out = nullptr)
{
    detail::checkNodeQueues(q, q.points(), n_lights, q.sppN(), "resolveNode: queues of another light count");
    const rls_skin_node_traced t = detail::skinTraced(sheenVisibility, specularVisibility, sheenGlossy, specularGlossy, hits);
    const rls_skin_integrate_out o = detail::skinOut(aovs, out);
    check(rls_trace_skin_resolve(d.ctx(), q.points(), &c, P.cvec3(), lights, n_lights,
                                 cavityFade ? 1 : 0, literalMatrix ? 1 : 0, q.sppN(), &q.c(), &t, &o));
}

// rlSkin at the hits of secondary rays (rls_trace_skin_bounce_emit / _resolve): emitNode / resolveNode with the ray state per
// point and the options' GI depths; diffuseVisibility: for q.diffuseShadow()'s rays (an empty Planes without lights)
inline void emitBounce(const Device &d, const rls_skin_closure &c, const Planes &P, const rls_sphere_light *lights, int n_lights,
                       int64_t n, int spp_n, uint32_t seed, const rls_ray_state &state, const rls_gi_depths &depths,
                       SkinBounceQueues &q, uint64_t first_index = 0)
{
    detail::checkNodeQueues(q, n, n_lights, spp_n, "emitBounce: queues of another size or light count");
    check(rls_trace_skin_bounce_emit(d.ctx(), n, &c, P.cvec3(), lights, n_lights, spp_n, seed,
                                     first_index, &state, &depths, &q.c()));
}
inline void resolveBounce(const Device &d, const rls_skin_closure &c, const Planes &P, const rls_sphere_light *lights,
                          int n_lights, const rls_ray_state &state, const rls_gi_depths &depths, const SkinBounceQueues &q,
                          const Planes &sheenVisibility, const Planes &specularVisibility, const Planes &sheenGlossy,
                          const Planes &specularGlossy, const rls_probe_hits &hits, const Planes &diffuseVisibility,
                          bool cavityFade, bool literalMatrix, Planes &aovs, Planes *out = nullptr)
{
    detail::checkNodeQueues(q, q.points(), n_lights, q.sppN(), "resolveBounce: queues of another light count");
    const rls_skin_bounce_traced t = {detail::skinTraced(sheenVisibility, specularVisibility, sheenGlossy, specularGlossy, hits),
                                      detail::crgb(diffuseVisibility)};
    const rls_skin_integrate_out o = detail::skinOut(aovs, out);
    check(rls_trace_skin_bounce_resolve(d.ctx(), q.points(), &c, P.cvec3(), lights, n_lights,
                                        cavityFade ? 1 : 0, literalMatrix ? 1 : 0, q.sppN(), &state, &depths, &q.c(), &t, &o));
}

// sg->out_opacity of the three nodes at n points (rls_trace_ggx_opacity / _disney_opacity / _skin_opacity): rayType: the state's
// ray_type plane (RayState::c().ray_type) or nullptr, no point being a shadow ray's; outOpacity: 3 planes of n floats
// (Planes::rgb(), or planes inside a longer table).  rlSkin: incoming, the sg->out_opacity the node found, an empty Planes reading
// as 1; it may hold outOpacity's planes.
inline void ggxOpacity(const Device &d, const rls_ggx_opacity &p, int64_t n, const uint8_t *rayType, const rls_rgb &outOpacity)
{
    check(rls_trace_ggx_opacity(d.ctx(), n, &p, rayType, outOpacity));
}
inline void disneyOpacity(const Device &d, const rls_disney_opacity &p, int64_t n, const uint8_t *rayType,
                          const rls_rgb &outOpacity)
{
    check(rls_trace_disney_opacity(d.ctx(), n, &p, rayType, outOpacity));
}
inline void skinOpacity(const Device &d, const rls_skin_opacity &p, int64_t n, const uint8_t *rayType, const Planes &incoming,
                        const rls_rgb &outOpacity)
{
    check(rls_trace_skin_opacity(d.ctx(), n, &p, rayType, detail::crgb(incoming), outOpacity));
}

// The hits of `rays` shadow rays (rls_shadow_hits) in device buffers of its own: count [rays] and, per element k * rays + j
// (stride = rays), either the hit's out_opacity (Direct: opacity() is 3 planes of maxHits * rays floats) or the index of its
// surface in a caller's table of out_opacity values (Indexed: index(), maxHits * rays entries; the table, 3 planes of tableCount
// floats -- what an opacity call wrote for tableCount surfaces -- is passed to c()).  The caller's tracer fills them.
class ShadowHits {
public:
    enum Form { Direct, Indexed };

    ShadowHits(const Device &d, int64_t rays, int maxHits, Form form) : bufs_(d), rays_(rays), max_hits_(maxHits), form_(form)
    {
        const int64_t elements = rays * maxHits;
        count_ = bufs_.alloc<uint8_t>(rays);
        if (form == Direct) opacity_ = bufs_.alloc<float>(3 * elements);
        else index_ = bufs_.alloc<uint32_t>(elements);
    }
    ShadowHits(const ShadowHits &) = delete;
    ShadowHits &operator=(const ShadowHits &) = delete;

    int64_t rays() const { return rays_; }
    int maxHits() const { return max_hits_; }
    uint8_t *count() const { return count_; }
    float *opacity(int channel) const { return opacity_ + (size_t)channel * (size_t)rays_ * (size_t)max_hits_; }
    uint32_t *index() const { return index_; }
    // Direct
    rls_shadow_hits c() const
    {
        if (form_ != Direct) throw Error(RLS_ERR_INVALID_ARGUMENT, "ShadowHits::c: indexed hits need their table");
        return rls_shadow_hits{max_hits_, rays_, count_, rls_crgb{opacity(0), opacity(1), opacity(2)}, nullptr, 0u};
    }
    // Indexed: table: 3 planes of tableCount floats
    rls_shadow_hits c(const Planes &table, uint32_t tableCount) const
    {
        if (form_ != Indexed) throw Error(RLS_ERR_INVALID_ARGUMENT, "ShadowHits::c: direct hits take no table");
        return rls_shadow_hits{max_hits_, rays_, count_, detail::crgb(table), index_, tableCount};
    }

private:
    detail::DeviceBuffers bufs_;
    int64_t rays_;
    int max_hits_;
    Form form_;
    uint8_t *count_ = nullptr;
    float *opacity_ = nullptr;
    uint32_t *index_ = nullptr;
};

// the visibility of the shadow rays from their hits' opacities (rls_trace_shadow_visibility): base (an empty Planes: 1) times
// (1 - opacity) of every hit, in hit order; visibility: 3 planes of >= rays floats, what resolveDirect and the node resolves take
inline void foldVisibility(const Device &d, int64_t rays, const rls_shadow_hits &hits, const Planes &base, Planes &visibility)
{
    check(rls_trace_shadow_visibility(d.ctx(), rays, &hits, detail::crgb(base), visibility.rgb()));
}

// The stable partition of a traced queue's `rays` rays by the node bin they hit (rls_hit_routes) in device buffers of its own:
// offsets [bins + 2], order [rays], slot [rays] (where asked) and the scratch.  routeHits fills it; bounds() reads offsets once
// per route (synchronises): bin b's rays are index(b) [size(b)], ascending, b == bins the misses.
class HitRoutes {
public:
    HitRoutes(const Device &d, int64_t rays, int bins, bool slot = false) : bufs_(d), dev_(&d), rays_(rays)
    {
        size_t scratch = 0;
        check(rls_trace_route_scratch_bytes(rays, bins, &scratch));
        r_.bins = bins;
        r_.offsets = bufs_.alloc<int64_t>(bins + 2);
        r_.order = bufs_.alloc<uint32_t>(rays);
        if (slot) r_.slot = bufs_.alloc<uint32_t>(rays);
        r_.scratch = bufs_.alloc(scratch);
        r_.scratch_bytes = scratch;
    }
    HitRoutes(const HitRoutes &) = delete;
    HitRoutes &operator=(const HitRoutes &) = delete;

    const rls_hit_routes &c() const { return r_; }
    int64_t rays() const { return rays_; }
    int bins() const { return r_.bins; }
    void routed() { host_.clear(); }
    const std::vector<int64_t> &bounds() const
    {
        if (host_.empty()) {
            host_.resize((size_t)r_.bins + 2);
            check(rls_copy_to_host(dev_->ctx(), host_.data(), r_.offsets, host_.size() * sizeof(int64_t)));
        }
        return host_;
    }
    int64_t size(int b) const { return bounds().at((size_t)b + 1) - bounds().at((size_t)b); }
    const uint32_t *index(int b) const { return r_.order + bounds().at((size_t)b); }

private:
    detail::DeviceBuffers bufs_;
    const Device *dev_;
    int64_t rays_;
    rls_hit_routes r_{};
    mutable std::vector<int64_t> host_;
};

// bin: one byte per ray, the node bin of the surface it hit; a value >= routes.bins() (255 by convention) a miss
inline void routeHits(const Device &d, const uint8_t *bin, HitRoutes &routes)
{
    routes.routed();
    check(rls_trace_route_hits(d.ctx(), routes.rays(), bin, &routes.c()));
}

// The planes one mover call takes, pair by pair: word(src, dst) a plane of floats or 32-bit ids, byte(src, dst) a plane of
// bytes; state(src, dst) the five planes of an rls_ray_state; planes(src, first, dst, count) `count` planes of two Planes.
class RoutePlanes {
public:
    RoutePlanes &word(const void *src, void *dst)
    {
        if (p_.n_w32 >= RLS_ROUTE_MAX_W32) throw Error(RLS_ERR_INVALID_ARGUMENT, "RoutePlanes: more than RLS_ROUTE_MAX_W32 word planes");
        p_.src_w32[p_.n_w32] = src; p_.dst_w32[p_.n_w32++] = dst;
        return *this;
    }
    RoutePlanes &byte(const uint8_t *src, uint8_t *dst)
    {
        if (p_.n_u8 >= RLS_ROUTE_MAX_U8) throw Error(RLS_ERR_INVALID_ARGUMENT, "RoutePlanes: more than RLS_ROUTE_MAX_U8 byte planes");
        p_.src_u8[p_.n_u8] = src; p_.dst_u8[p_.n_u8++] = dst;
        return *this;
    }
    RoutePlanes &planes(const Planes &src, Planes &dst, int count, int srcFirst = 0, int dstFirst = 0)
    {
        for (int k = 0; k < count; k++) word(src.plane(srcFirst + k), dst.plane(dstFirst + k));
        return *this;
    }
    RoutePlanes &state(const rls_ray_state &src, const rls_ray_state &dst)
    {
        return byte(src.ray_type, const_cast<uint8_t *>(dst.ray_type)).byte(src.Rr, const_cast<uint8_t *>(dst.Rr))
            .byte(src.Rr_diff, const_cast<uint8_t *>(dst.Rr_diff)).byte(src.Rr_gloss, const_cast<uint8_t *>(dst.Rr_gloss))
            .byte(src.Rr_refr, const_cast<uint8_t *>(dst.Rr_refr));
    }
    const rls_route_planes &c() const { return p_; }

private:
    rls_route_planes p_{};
};

// bin b's columns of the per-ray src planes into the dense dst planes (rls_trace_route_gather); an empty bin moves nothing
inline void gatherHits(const Device &d, const HitRoutes &routes, int b, const RoutePlanes &planes)
{
    if (routes.size(b) > 0) check(rls_trace_route_gather(d.ctx(), routes.size(b), routes.index(b), &planes.c()));
}
// bin b's dense src planes back to its rays' places in the per-ray dst planes (rls_trace_route_scatter)
inline void scatterToRays(const Device &d, const HitRoutes &routes, int b, const RoutePlanes &planes)
{
    if (routes.size(b) > 0) check(rls_trace_route_scatter(d.ctx(), routes.size(b), routes.index(b), &planes.c()));
}
// value[p] into the misses' places of dst's first `count` planes (rls_trace_route_fill): the environment's radiance
inline void fillMisses(const Device &d, const HitRoutes &routes, const float *value, Planes &dst, int count = 3)
{
    float *planes[RLS_ROUTE_MAX_W32] = {};
    if (count < 1 || count > RLS_ROUTE_MAX_W32) throw Error(RLS_ERR_INVALID_ARGUMENT, "fillMisses: count outside 1 .. RLS_ROUTE_MAX_W32");
    for (int k = 0; k < count; k++) planes[k] = dst.plane(k);
    const int misses = routes.bins();
    if (routes.size(misses) > 0) check(rls_trace_route_fill(d.ctx(), routes.size(misses), routes.index(misses), count, planes, value));
}

} // namespace rlsb
