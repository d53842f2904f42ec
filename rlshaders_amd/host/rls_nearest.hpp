// rls_nearest.hpp -- C++14 host-side mirror of the nearest-hit queries (include/rlshaders_amd_nearest.h, librls_nearest.so).
// Header-only, in the style of rls_shadow_walk.hpp; it uses rls_trace.hpp's Device / check / DeviceBuffers.
//
// The renderer's part of both walks and of every traced queue, on the device:
//     rlsb::NearestScene scene(dev, mesh);                                   // the tree is built and uploaded here
//     rlsb::NearestFound found(dev, rays, rlsb::NearestFound::ForShadowWalk); // its planes are its own
//     rlsb::ShadowWalk walk(dev, sq.c().capacity);  walk.begin(sq, P, maxSteps);
//     for (int64_t m; (m = walk.active()) > 0;) {
//         scene.hits(walk.rays(), m, found);                                 // the nearest hits of the listed rays
//         walk.step(found.shadowFound(table.rgb(), surfaces), m);            // surface indexes the opacity table
//     }
// No call here synchronises; hits(list, -1, found) traces the list's capacity, so a whole walk can be recorded into a Graph.
#pragma once

#include <vector>

#include "rls_trace.hpp"
#include "rlshaders_amd_nearest.h"
#include "rlshaders_amd_shadow_walk.h"

namespace rlsb {

// A scene: the one owner of its rls_nearest_scene.
class NearestScene {
public:
    NearestScene(const Device &d, const rls_nearest_mesh &mesh) : dev_(&d) { check(rls_nearest_scene_create(d.ctx(), &mesh, &s_)); }
    ~NearestScene() { rls_nearest_scene_destroy(s_); }
    NearestScene(const NearestScene &) = delete;
    NearestScene &operator=(const NearestScene &) = delete;

    rls_nearest_scene_info info() const
    {
        rls_nearest_scene_info i{};
        check(rls_nearest_scene_get_info(s_, &i));
        return i;
    }
    // the nearest hit of every ray / of every entry of a walk's list (bound: an upper bound on its count, < 0: its capacity)
    void hits(const rls_nearest_rays &rays, const rls_nearest_found &found) const { check(rls_nearest_hits(dev_->ctx(), s_, &rays, &found)); }
    void hits(const rls_walk_rays &list, int64_t bound, const rls_nearest_found &found) const
    {
        check(rls_nearest_walk_hits(dev_->ctx(), s_, &list, bound, &found));
    }
    const rls_nearest_scene *c() const { return s_; }

private:
    const Device *dev_;
    rls_nearest_scene *s_ = nullptr;
};

// The found planes of up to `rays` rays, owned here and nowhere else: a constructor that throws half way frees what it had.
class NearestFound {
public:
    enum Want : unsigned {
        P = 1, N = 2, Ns = 4, T = 8, Wo = 16, Prim = 32, Surface = 64, UV = 128, Bin = 256, Last = 512,
        ForWalk = P | N | Ns | Surface | Last,          // rls_walk_found: hit, t, P, N, Ns, object = surface
        ForShadowWalk = P | Surface | Last,              // rls_shadow_walk_found: hit, t, P, index = surface
        ForRouting = P | N | Ns | T | Wo | Surface | Bin,
        All = 1023
    };
    // ids: the entries of `last` (the rays of the queue a walk began on), by default `rays`
    NearestFound(const Device &d, int64_t rays, unsigned planes = All, int64_t ids = -1) : bufs_(d), rays_(rays)
    {
        const int64_t n = rays > 0 ? rays : 1;
        f_.hit = bufs_.alloc<uint8_t>(n);
        f_.t = bufs_.alloc<float>(n);
        if (planes & P) f_.P = bufs_.vec3(n);
        if (planes & N) f_.N = bufs_.vec3(n);
        if (planes & Ns) f_.Ns = bufs_.vec3(n);
        if (planes & T) f_.T = bufs_.vec3(n);
        if (planes & Wo) f_.wo = bufs_.vec3(n);
        if (planes & Prim) f_.prim = bufs_.alloc<uint32_t>(n);
        if (planes & Surface) f_.surface = bufs_.alloc<uint32_t>(n);
        if (planes & UV) { f_.u = bufs_.alloc<float>(n); f_.v = bufs_.alloc<float>(n); }
        if (planes & Bin) bin_ = bufs_.alloc<uint8_t>(n);
        if (planes & Last) {
            ids_ = ids < 0 ? n : ids > 0 ? ids : 1;
            f_.last = bufs_.alloc<uint32_t>(ids_);
        }
    }
    NearestFound(const NearestFound &) = delete;
    NearestFound &operator=(const NearestFound &) = delete;

    // every ray skips nothing again (a copy from the host: it synchronises)
    void resetLast(const Device &d)
    {
        if (!f_.last) return;
        const std::vector<uint32_t> none((size_t)ids_, RLS_NEAREST_NO_PRIM);
        check(rls_copy_to_device(d.ctx(), f_.last, none.data(), sizeof(uint32_t) * none.size()));
    }
    // the bin plane is written from this table of `count` bytes (device) from now on
    void binsFrom(const uint8_t *binOfSurface, uint32_t count)
    {
        f_.bin = bin_;
        f_.bin_of_surface = binOfSurface;
        f_.bin_count = count;
    }
    const rls_nearest_found &c() const { return f_; }
    operator const rls_nearest_found &() const { return f_; }
    int64_t rays() const { return rays_; }
    const uint8_t *bin() const { return bin_; }

    // the same planes as the walks read them: no adapter kernel
    rls_walk_found walkFound(bool objects = true) const
    {
        return rls_walk_found{f_.hit, f_.t, cv(f_.P), cv(f_.N), cv(f_.Ns), objects ? f_.surface : nullptr};
    }
    rls_shadow_walk_found shadowFound(rls_crgb opacityTable, uint32_t surfaces) const
    {
        return rls_shadow_walk_found{f_.hit, f_.t, cv(f_.P), opacityTable, f_.surface, surfaces};
    }

private:
    static rls_cvec3 cv(rls_vec3 v) { return rls_cvec3{v.x, v.y, v.z}; }
    detail::DeviceBuffers bufs_;
    rls_nearest_found f_{};
    uint8_t *bin_ = nullptr;
    int64_t rays_, ids_ = 0;
};

} // namespace rlsb
