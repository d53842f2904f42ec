// rls_nearest_refit.hpp -- C++14 host-side mirror of the refit of a nearest-hit scene (include/rlshaders_amd_nearest_refit.h,
// librls_nearest_refit.so).  Header-only, in the style of rls_nearest.hpp, whose NearestScene it moves.
//
// A mesh that deforms every frame, its vertices left on the device by the deformer:
//     rlsb::NearestScene scene(dev, mesh);                  // the tree is built on the host, once
//     rlsb::NearestRefit refit(dev, scene);                 // the tree's levels are read, once
//     per frame:  refit.update(deformedVertices);           // device float [nv * 3]; no synchronisation
//                 scene.hits(...);                          // every query on the same stream sees the moved mesh
// Every query after an update returns, bit for bit, what a fresh NearestScene on the moved vertices returns.
#pragma once

#include <vector>

#include "rls_nearest.hpp"
#include "rlshaders_amd_nearest_refit.h"

namespace rlsb {

// The refit of a scene: the one owner of its rls_nearest_refit.  It borrows the scene, which must outlive it (declare the
// refit after the scene).
class NearestRefit {
public:
    NearestRefit(const Device &d, NearestScene &scene) : dev_(&d), scene_(&scene)
    {
        check(rls_nearest_refit_create(d.ctx(), const_cast<rls_nearest_scene *>(scene.c()), &r_));
    }
    ~NearestRefit() { rls_nearest_refit_destroy(r_); }
    NearestRefit(const NearestRefit &) = delete;
    NearestRefit &operator=(const NearestRefit &) = delete;

    rls_nearest_refit_info info() const
    {
        rls_nearest_refit_info i{};
        check(rls_nearest_refit_get_info(r_, &i));
        return i;
    }
    // vertices, normals: device float [nv * 3] (normals NULL: the scene's stay); parked: device, one value, or NULL
    void update(const float *vertices, const float *normals = nullptr, int64_t *parked = nullptr)
    {
        rls_nearest_refit_mesh m{};
        m.nv = info().nv; m.vertices = vertices; m.normals = normals; m.parked = parked;
        check(rls_nearest_refit_update(dev_->ctx(), r_, &m));
    }
    // the tree as it is now, on the host (it synchronises): boxes [nodes * 6], links [nodes * 2], prims [nt]
    void readTree(std::vector<float> &boxes, std::vector<uint32_t> &links, std::vector<uint32_t> &prims) const
    {
        const rls_nearest_refit_info i = info();
        boxes.assign((size_t)(6 * i.nodes), 0.0f);
        links.assign((size_t)(2 * i.nodes), 0u);
        prims.assign((size_t)i.nt, 0u);
        check(rls_nearest_refit_read_tree(dev_->ctx(), r_, boxes.data(), links.data(), prims.data()));
    }
    NearestScene &scene() const { return *scene_; }
    const rls_nearest_refit *c() const { return r_; }

private:
    const Device *dev_;
    NearestScene *scene_;
    rls_nearest_refit *r_ = nullptr;
};

} // namespace rlsb
