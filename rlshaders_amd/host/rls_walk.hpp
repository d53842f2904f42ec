// rls_walk.hpp -- C++14 host-side mirror of rlSss's probe walk (include/rlshaders_amd_walk.h, librls_walk.so).  Header-only, in
// the style of rls_trace.hpp, whose ProbeQueue it walks and whose Device / Planes / check / DeviceBuffers it uses.
//
// Between emitProbes and resolveScatter the reference walks every probe ray through the object (SssSampler::traceProbe,
// src/rlSss.h:288-357); with this class the renderer's part of that is a nearest-hit query:
//     rlsb::ProbeQueue pq(dev, n, spp_n);
//     rlsb::emitProbes(dev, sss, P, n, spp_n, seed, pq);
//     rlsb::ProbeWalk walk(dev, pq.count());                               // two lists, the hits, the scratch: all its own
//     walk.begin(pq, P);                                                   // the rays with maxdist > 0 listed
//     for (int64_t m; (m = walk.active()) > 0;) {                          // at most RLS_WALK_TRIALS rounds
//         ... the nearest hit in (0, maxdist] of walk.rays()'s first m entries -> an rls_walk_found ...
//         walk.step(found, m);
//     }
//     rlsb::resolveScatter(dev, sss, P, pq, walk.hits(E), cavity, literal, result);   // E: the renderer's irradiance planes
// active() is the one call that synchronises; step(found) without a bound walks the list's capacity and can be recorded into
// a Graph.
#pragma once

#include "rls_trace.hpp"
#include "rlshaders_amd_walk.h"

namespace rlsb {

namespace detail {
// The two active lists of a walk (rls_walk_rays: the probe walk's and the shadow walk's alike), stated once: the ten buffers of
// each out of the walk's own DeviceBuffers, the list the next step reads, and the flip after a step.
struct WalkLists {
    rls_walk_rays lists[2] = {};
    int at = 0;
    void alloc(DeviceBuffers &bufs, int64_t rays)
    {
        for (rls_walk_rays &l : lists) {
            l.capacity = rays;
            l.count = bufs.alloc<int64_t>(1);
            l.ray = bufs.alloc<uint32_t>(rays);
            l.origin = bufs.vec3(rays);
            l.dir = bufs.vec3(rays);
            l.maxdist = bufs.alloc<float>(rays);
            l.trials = bufs.alloc<uint8_t>(rays);
        }
    }
    const rls_walk_rays &first() { at = 0; return lists[0]; }     // what begin writes
    const rls_walk_rays &in() const { return lists[at]; }          // what a step reads
    const rls_walk_rays &out() const { return lists[at ^ 1]; }     // ... and writes, before the flip
    void flip() { at ^= 1; }
};
} // namespace detail

// One walk's device buffers -- the two active lists, the hits, the scratch -- owned here and nowhere else: allocated through one
// DeviceBuffers member, so a constructor that throws half way frees what it had.
class ProbeWalk {
public:
    ProbeWalk(const Device &d, int64_t rays, int maxHits = RLS_MAX_PROBE_HITS) : dev_(&d), bufs_(d)
    {
        w_.rays = rays;
        w_.hits.max_hits = maxHits;
        w_.hits.stride = rays;
        size_t scratch = 0;
        check(rls_walk_scratch_bytes(rays, &scratch));
        lists_.alloc(bufs_, rays);
        w_.hits.count = bufs_.alloc<uint8_t>(rays);
        w_.hits.P = bufs_.vec3(rays * maxHits);
        w_.hits.N = bufs_.vec3(rays * maxHits);
        w_.scratch = bufs_.alloc(scratch);
        w_.scratch_bytes = scratch;
    }
    ProbeWalk(const ProbeWalk &) = delete;
    ProbeWalk &operator=(const ProbeWalk &) = delete;

    // start on q's rays about the shading points P (3 planes of q.points() floats); own: one id per point or nullptr
    void begin(const ProbeQueue &q, const Planes &P, const uint32_t *own = nullptr, int foreign = RLS_WALK_FOREIGN_STOPS)
    {
        if (q.count() != w_.rays) throw Error(RLS_ERR_INVALID_ARGUMENT, "ProbeWalk::begin: a queue of another size");
        w_.spp = q.sppN() * q.sppN();
        w_.P = P.cvec3();
        w_.own = own;
        w_.foreign = foreign;
        check(rls_walk_begin(dev_->ctx(), &w_, &q.c(), &lists_.first()));
    }
    // the list the next step reads
    const rls_walk_rays &rays() const { return lists_.in(); }
    // its count (synchronises)
    int64_t active() const
    {
        int64_t m = 0;
        check(rls_walk_active(dev_->ctx(), &lists_.in(), &m));
        return m;
    }
    // found: the nearest hits of the listed rays; bound: an upper bound on active(), < 0 for the capacity
    void step(const rls_walk_found &found, int64_t bound = -1)
    {
        check(rls_walk_step(dev_->ctx(), &w_, &lists_.in(), &found, bound, &lists_.out()));
        lists_.flip();
    }
    // what the resolves and emitHits read: the walk's count, P, N and the caller's irradiance planes (max_hits * rays floats each)
    rls_probe_hits hits(rls_crgb irradiance = rls_crgb{nullptr, nullptr, nullptr}) const
    {
        rls_probe_hits h = {};
        h.max_hits = w_.hits.max_hits; h.stride = w_.hits.stride; h.count = w_.hits.count;
        h.P = rls_cvec3{w_.hits.P.x, w_.hits.P.y, w_.hits.P.z};
        h.N = rls_cvec3{w_.hits.N.x, w_.hits.N.y, w_.hits.N.z};
        h.irradiance = irradiance;
        return h;
    }
    const rls_walk &c() const { return w_; }

private:
    const Device *dev_;
    detail::DeviceBuffers bufs_;
    detail::WalkLists lists_;
    rls_walk w_{};
};

} // namespace rlsb
