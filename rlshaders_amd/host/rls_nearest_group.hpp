// rls_nearest_group.hpp -- C++14 host-side mirror of instanced scenes (include/rlshaders_amd_nearest_group.h,
// librls_nearest_group.so).  Header-only, in the style of rls_nearest.hpp, whose NearestScene it places.
//
// Many copies of one mesh, some of them moving rigidly:
//     rlsb::NearestScene scene(dev, mesh);                                   // one mesh, one tree
//     std::vector<rls_nearest_instance> placed = ...;                        // scene.c(), to_object, to_world, surface_base each
//     rlsb::NearestGroup group(dev, placed);                                 // the top tree is built on the host, once
//     rlsb::NearestGroupFound found(dev, rays, rlsb::NearestFound::ForShadowWalk);
//     per frame:  group.update(toObject, toWorld);                           // device float [instances * 12] each; no synchronisation
//                 group.hits(walk.rays(), m, found);                         // found.found(): what the walks' steps take
// Every query after an update returns, bit for bit, what a fresh NearestGroup with those matrices returns.
#pragma once

#include <vector>

#include "rls_nearest.hpp"
#include "rlshaders_amd_nearest_group.h"

namespace rlsb {

// The found planes of a group query: a NearestFound, the instance plane and, with NearestFound::Last, last_instance beside last.
class NearestGroupFound {
public:
    NearestGroupFound(const Device &d, int64_t rays, unsigned planes = NearestFound::All, int64_t ids = -1)
        : found_(d, rays, planes, ids), bufs_(d)
    {
        const int64_t n = rays > 0 ? rays : 1;
        instance_ = bufs_.alloc<uint32_t>(n);
        if (planes & NearestFound::Last) {
            ids_ = ids < 0 ? n : ids > 0 ? ids : 1;
            last_instance_ = bufs_.alloc<uint32_t>(ids_);
        }
    }
    NearestGroupFound(const NearestGroupFound &) = delete;
    NearestGroupFound &operator=(const NearestGroupFound &) = delete;

    // every ray skips nothing again (copies from the host: it synchronises)
    void resetLast(const Device &d)
    {
        found_.resetLast(d);
        if (!last_instance_) return;
        const std::vector<uint32_t> none((size_t)ids_, RLS_NEAREST_NO_INSTANCE);
        check(rls_copy_to_device(d.ctx(), last_instance_, none.data(), sizeof(uint32_t) * none.size()));
    }
    NearestFound &found() { return found_; }
    const NearestFound &found() const { return found_; }
    const uint32_t *instance() const { return instance_; }
    rls_nearest_group_found c() const { return rls_nearest_group_found{found_.c(), instance_, last_instance_}; }

private:
    NearestFound found_;
    detail::DeviceBuffers bufs_;
    uint32_t *instance_ = nullptr, *last_instance_ = nullptr;
    int64_t ids_ = 0;
};

// A group: the one owner of its rls_nearest_group.  It borrows the instances' scenes, which must outlive it (declare the group
// after the scenes).
class NearestGroup {
public:
    NearestGroup(const Device &d, const std::vector<rls_nearest_instance> &instances, int leafSize = 0) : dev_(&d)
    {
        check(rls_nearest_group_create(d.ctx(), instances.data(), (int64_t)instances.size(), leafSize, &g_));
    }
    ~NearestGroup() { rls_nearest_group_destroy(g_); }
    NearestGroup(const NearestGroup &) = delete;
    NearestGroup &operator=(const NearestGroup &) = delete;

    rls_nearest_group_info info() const
    {
        rls_nearest_group_info i{};
        check(rls_nearest_group_get_info(g_, &i));
        return i;
    }
    // toObject, toWorld: device float [instances * 12] each, or both NULL (the matrices stay, the world boxes are taken again from
    // the scenes as they are on the device then); parked: device, one value, or NULL
    void update(const float *toObject = nullptr, const float *toWorld = nullptr, int64_t *parked = nullptr)
    {
        const rls_nearest_group_moves m{toObject, toWorld, parked};
        check(rls_nearest_group_update(dev_->ctx(), g_, &m));
    }
    // the nearest hit of every ray / of every entry of a walk's list (bound: an upper bound on its count, < 0: its capacity)
    void hits(const rls_nearest_rays &rays, const NearestGroupFound &found) const
    {
        const rls_nearest_group_found f = found.c();
        check(rls_nearest_group_hits(dev_->ctx(), g_, &rays, &f));
    }
    void hits(const rls_walk_rays &list, int64_t bound, const NearestGroupFound &found) const
    {
        const rls_nearest_group_found f = found.c();
        check(rls_nearest_group_walk_hits(dev_->ctx(), g_, &list, bound, &f));
    }
    // the top tree as it is now, on the host (it synchronises): boxes [top_nodes * 6], links [top_nodes * 2], order [instances],
    // world [instances * 6], parked [instances]
    void readTree(std::vector<float> &boxes, std::vector<uint32_t> &links, std::vector<uint32_t> &order, std::vector<float> &world,
                  std::vector<uint8_t> &parked) const
    {
        const rls_nearest_group_info i = info();
        boxes.assign((size_t)(6 * i.top_nodes), 0.0f);
        links.assign((size_t)(2 * i.top_nodes), 0u);
        order.assign((size_t)i.instances, 0u);
        world.assign((size_t)(6 * i.instances), 0.0f);
        parked.assign((size_t)i.instances, 0);
        check(rls_nearest_group_read_tree(dev_->ctx(), g_, boxes.data(), links.data(), order.data(), world.data(), parked.data()));
    }
    const rls_nearest_group *c() const { return g_; }

private:
    const Device *dev_;
    rls_nearest_group *g_ = nullptr;
};

} // namespace rlsb
