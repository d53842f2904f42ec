// rls_nearest_any.hpp -- C++14 host-side mirror of the any-hit shadow queries (include/rlshaders_amd_nearest_any.h,
// librls_nearest_any.so).  Header-only, in the style of rls_nearest_group.hpp; it queries rls_nearest.hpp's NearestScene.
//
// A light loop's shadow rays through a scene, the walk begun on the veiled rays alone:
//     rlsb::NearestScene scene(dev, mesh);
//     rlsb::ShadowWalk walk(dev, sq.c().capacity);                           // its visibility planes are the query's too
//     rlsb::NearestAny any(dev, sq.c().capacity);
//     any.opaqueFrom(rlsb::detail::crgb(table), surfaces);                   // the flag table, from the opacity table
//     any.hits(scene, any.raysOf(sq, P), walk.c().visibility);               // one launch: blocked rays base * 0, the others base
//     walk.begin(any.veiled(sq), sq.c().offsets + sq.points(), P.cvec3(), maxSteps, any.asBase(walk.c().visibility));
//     for (int64_t m; (m = walk.active()) > 0;) { scene.hits(walk.rays(), m, found); walk.step(found.shadowFound(...), m); }
// No call here synchronises.
#pragma once

#include "rls_nearest.hpp"
#include "rlshaders_amd_nearest_any.h"

namespace rlsb {

// The state and reach planes of up to `rays` rays and a flag table, owned here and nowhere else.
class NearestAny {
public:
    // ids: the entries of the planes indexed by ray id (reach), by default `rays`
    NearestAny(const Device &d, int64_t rays, int64_t ids = -1) : dev_(&d), bufs_(d), rays_(rays)
    {
        const int64_t n = rays > 0 ? rays : 1;
        state_ = bufs_.alloc<uint8_t>(n);
        reach_ = bufs_.alloc<float>(ids < 0 ? n : ids > 0 ? ids : 1);
    }
    NearestAny(const NearestAny &) = delete;
    NearestAny &operator=(const NearestAny &) = delete;

    // the flag table of an opacity table of `surfaces` entries (rls_trace_*_opacity's): queries from now on read it
    void opaqueFrom(rls_crgb table, uint32_t surfaces)
    {
        flags_ = bufs_.alloc<uint8_t>(surfaces > 0 ? surfaces : 1);
        check(rls_nearest_any_opaque(dev_->ctx(), &table, surfaces, flags_));
        surfaces_ = surfaces;
    }
    // every triangle is opaque again
    void allOpaque() { flags_ = nullptr; surfaces_ = 0; }

    // a shadow queue's rays as the query reads them: origin = O through the queue's point plane, its dir, maxdist and device count
    static rls_nearest_rays raysOf(const rls_shadow_queue &q, const int64_t *count, rls_cvec3 O)
    {
        rls_nearest_rays r = {};
        r.rays = q.capacity; r.count = count; r.origin = O; r.via = q.point;
        r.dir = rls_cvec3{q.dir.x, q.dir.y, q.dir.z};
        r.maxdist = q.maxdist;
        return r;
    }
    static rls_nearest_rays raysOf(const ShadowQueue &q, const Planes &O) { return raysOf(q.c(), q.c().offsets + q.points(), O.cvec3()); }
    // the same queue with the reach plane for its maxdist: what the second begin takes
    rls_shadow_queue veiled(const rls_shadow_queue &q) const
    {
        rls_shadow_queue v = q;
        v.maxdist = reach_;
        return v;
    }
    static rls_crgb asBase(rls_rgb v) { return rls_crgb{v.r, v.g, v.b}; }

    rls_nearest_any_found found(rls_rgb visibility, rls_crgb base = rls_crgb{nullptr, nullptr, nullptr}, const uint32_t *last = nullptr) const
    {
        rls_nearest_any_found f = {};
        f.state = state_; f.opaque = flags_; f.opaque_count = surfaces_;
        f.base = base; f.visibility = visibility; f.reach = reach_; f.last = last;
        return f;
    }
    // the state of every ray / of every entry of a walk's list (bound: an upper bound on its count, < 0: its capacity)
    void hits(const NearestScene &scene, const rls_nearest_rays &rays, rls_rgb visibility,
              rls_crgb base = rls_crgb{nullptr, nullptr, nullptr}, const uint32_t *last = nullptr) const
    {
        const rls_nearest_any_found f = found(visibility, base, last);
        check(rls_nearest_any_hits(dev_->ctx(), scene.c(), &rays, &f));
    }
    void hits(const NearestScene &scene, const rls_walk_rays &list, int64_t bound, rls_rgb visibility,
              rls_crgb base = rls_crgb{nullptr, nullptr, nullptr}, const uint32_t *last = nullptr) const
    {
        const rls_nearest_any_found f = found(visibility, base, last);
        check(rls_nearest_any_walk_hits(dev_->ctx(), scene.c(), &list, bound, &f));
    }
    const uint8_t *state() const { return state_; }
    const float *reach() const { return reach_; }
    const uint8_t *flags() const { return flags_; }
    int64_t rays() const { return rays_; }

private:
    const Device *dev_;
    detail::DeviceBuffers bufs_;
    uint8_t *state_ = nullptr, *flags_ = nullptr;
    float *reach_ = nullptr;
    uint32_t surfaces_ = 0;
    int64_t rays_;
};

} // namespace rlsb
