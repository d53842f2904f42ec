// rls_shadow_walk.hpp -- C++14 host-side mirror of the shadow rays' walk (include/rlshaders_amd_shadow_walk.h,
// librls_shadow_walk.so).  Header-only, in the style of rls_walk.hpp; it walks rls_trace.hpp's ShadowQueue and uses its Device /
// Planes / check / DeviceBuffers.
//
// Between emitDirect (or a node's emit) and the resolve, the renderer owes a visibility per shadow ray; with this class its part
// of that is a nearest-hit query:
//     rlsb::ShadowQueue sq(dev, n, n_lights, spp_n, rlsb::ShadowQueue::Ggx);
//     rlsb::emitDirect(dev, ggx, shader, P, lights, n_lights, n, spp_n, seed, sq);
//     rlsb::ShadowWalk walk(dev, sq.c().capacity);                         // two lists, the visibility, the scratch: all its own
//     walk.begin(sq, P, maxSteps);                                         // T = 1, the rays with maxdist > 0 listed
//     for (int64_t m; (m = walk.active()) > 0;) {                          // at most maxSteps rounds
//         ... the nearest hit in (0, maxdist] of walk.rays()'s first m entries and its opacity -> an rls_shadow_walk_found ...
//         walk.step(found, m);
//     }
//     rlsb::resolveDirect(dev, ggx, shader, lights, n_lights, sq, walk.visibility(), directDiffuse, directSpecular);
// active() is the one call that synchronises; begin reads the queue's ray count on the device, and step(found) without a bound
// walks the list's capacity, so a whole walk can be recorded into a Graph.
#pragma once

#include "rls_walk.hpp"                                   // detail::WalkLists: the active lists are the probe walk's, as in C
#include "rlshaders_amd_shadow_walk.h"

namespace rlsb {

// One walk's device buffers -- the two active lists and the scratch through one DeviceBuffers member, the visibility in one
// Planes member -- owned here and nowhere else: a constructor that throws half way frees what it had.
class ShadowWalk {
public:
    // rays: an upper bound on the rays of the queues this walk will begin on (a queue's capacity)
    ShadowWalk(const Device &d, int64_t rays) : dev_(&d), bufs_(d)
    {
        w_.rays = rays;
        size_t scratch = 0;
        check(rls_shadow_walk_scratch_bytes(rays, &scratch));
        lists_.alloc(bufs_, rays);
        w_.scratch = bufs_.alloc(scratch);
        w_.scratch_bytes = scratch;
        vis_ = Planes(d, rays > 0 ? rays : 1, 3);
        w_.visibility = vis_.rgb();
    }
    ShadowWalk(const ShadowWalk &) = delete;
    ShadowWalk &operator=(const ShadowWalk &) = delete;

    // start on q's rays (their number is read on the device, q's offsets[points]) from the origins O[point[j]] -- sg->P per point
    // -- or O[via[point[j]]]; base: 3 planes of >= rays floats, or empty for T = 1
    void begin(const ShadowQueue &q, const Planes &O, int maxSteps, const Planes &base = Planes(), const int64_t *via = nullptr)
    {
        if (q.c().capacity > w_.rays) throw Error(RLS_ERR_INVALID_ARGUMENT, "ShadowWalk::begin: a queue larger than the walk");
        begin(q.c(), q.c().offsets + q.points(), O.cvec3(), maxSteps, detail::crgb(base), via);
    }
    // the same on any rls_shadow_queue (the shadow queue of an rls_hit_queues, of a node's queue set); count: device, NULL-able
    void begin(const rls_shadow_queue &q, const int64_t *count, rls_cvec3 O, int maxSteps,
               rls_crgb base = rls_crgb{nullptr, nullptr, nullptr}, const int64_t *via = nullptr)
    {
        w_.count = count;
        w_.max_steps = maxSteps;
        w_.O = O;
        w_.via = via;
        w_.base = base;
        check(rls_shadow_walk_begin(dev_->ctx(), &w_, &q, &lists_.first()));
    }
    // the list the next step reads
    const rls_walk_rays &rays() const { return lists_.in(); }
    // its count (synchronises)
    int64_t active() const
    {
        int64_t m = 0;
        check(rls_shadow_walk_active(dev_->ctx(), &lists_.in(), &m));
        return m;
    }
    // found: the nearest hits of the listed rays and their opacity; bound: an upper bound on active(), < 0 for the capacity
    void step(const rls_shadow_walk_found &found, int64_t bound = -1)
    {
        check(rls_shadow_walk_step(dev_->ctx(), &w_, &lists_.in(), &found, bound, &lists_.out()));
        lists_.flip();
    }
    // T of every ray, valid after begin and after every step: what resolveDirect and the node resolves take as visibility
    const Planes &visibility() const { return vis_; }
    const rls_shadow_walk &c() const { return w_; }

private:
    const Device *dev_;
    detail::DeviceBuffers bufs_;
    detail::WalkLists lists_;
    Planes vis_;
    rls_shadow_walk w_{};
};

} // namespace rlsb
