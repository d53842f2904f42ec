// rls_nearest_rebuild.hpp -- C++14 host-side mirror of the device rebuild of a nearest-hit scene's tree
// (include/rlshaders_amd_nearest_rebuild.h, librls_nearest_rebuild.so).  Header-only, in the style of rls_nearest.hpp, whose
// NearestScene it rebuilds.
//
// A mesh that deforms far from the pose its tree was built for, its vertices left on the device by the deformer:
//     rlsb::NearestScene scene(dev, mesh);                  // the tree is built on the host, once
//     rlsb::NearestRebuild rebuild(dev, scene);             // the links are read and the working set allocated, once
//     every so often:  rebuild.update(deformedVertices);    // device float [nv * 3]; no synchronisation, no allocation
//                      scene.hits(...);                     // every query on the same stream sees the new tree
// After an update the scene holds the tree a fresh NearestScene on the moved vertices holds: a query returns its bytes at its cost.
#pragma once

#include <vector>

#include "rls_nearest.hpp"
#include "rlshaders_amd_nearest_rebuild.h"

namespace rlsb {

// The rebuild of a scene: the one owner of its rls_nearest_rebuild.  It borrows the scene, which must outlive it (declare the
// rebuild after the scene).
class NearestRebuild {
public:
    NearestRebuild(const Device &d, NearestScene &scene) : dev_(&d), scene_(&scene)
    {
        check(rls_nearest_rebuild_create(d.ctx(), const_cast<rls_nearest_scene *>(scene.c()), &r_));
    }
    ~NearestRebuild() { rls_nearest_rebuild_destroy(r_); }
    NearestRebuild(const NearestRebuild &) = delete;
    NearestRebuild &operator=(const NearestRebuild &) = delete;

    rls_nearest_rebuild_info info() const
    {
        rls_nearest_rebuild_info i{};
        check(rls_nearest_rebuild_get_info(r_, &i));
        return i;
    }
    // vertices, normals: device float [nv * 3] (normals NULL: the scene's stay); parked: device, one value, or NULL
    void update(const float *vertices, const float *normals = nullptr, int64_t *parked = nullptr)
    {
        rls_nearest_rebuild_mesh m{};
        m.nv = info().nv; m.vertices = vertices; m.normals = normals; m.parked = parked;
        check(rls_nearest_rebuild_update(dev_->ctx(), r_, &m));
    }
    // the tree as it is now, on the host (it synchronises): boxes [nodes * 6], links [nodes * 2], prims [nt]
    void readTree(std::vector<float> &boxes, std::vector<uint32_t> &links, std::vector<uint32_t> &prims) const
    {
        const rls_nearest_rebuild_info i = info();
        boxes.assign((size_t)(6 * i.nodes), 0.0f);
        links.assign((size_t)(2 * i.nodes), 0u);
        prims.assign((size_t)i.nt, 0u);
        check(rls_nearest_rebuild_read_tree(dev_->ctx(), r_, boxes.data(), links.data(), prims.data()));
    }
    NearestScene &scene() const { return *scene_; }
    const rls_nearest_rebuild *c() const { return r_; }

private:
    const Device *dev_;
    NearestScene *scene_;
    rls_nearest_rebuild *r_ = nullptr;
};

} // namespace rlsb
