// nearest_ownership.cpp -- rlsb::NearestScene and rlsb::NearestFound (host/rls_nearest.hpp) give back what they allocated, also
// when one of their allocations fails (tests/test_nearest_host_ownership.py).  Stand-alone over ownership_harness.hpp, like
// shadow_walk_ownership.cpp; rls_nearest_scene_create / _destroy are defined here over new and delete, counted and failed with
// the device blocks and, like them, given back the way they were made.
#include "rls_nearest.hpp"
#include "ownership_harness.hpp"

struct rls_nearest_scene { int unused; };

extern "C" {

rls_status rls_nearest_scene_create(rls_context *, const rls_nearest_mesh *, rls_nearest_scene **out)
{
    *out = nullptr;
    if (own::fails()) return RLS_ERR_OUT_OF_MEMORY;
    *out = new rls_nearest_scene();
    own::made(*out, [](void *s) { delete static_cast<rls_nearest_scene *>(s); });
    return RLS_OK;
}
rls_status rls_nearest_scene_destroy(rls_nearest_scene *s)
{
    if (!s) return RLS_OK;
    own::gone(s, "rls_nearest_scene_destroy of a scene");
    delete s;
    return RLS_OK;
}
rls_status rls_nearest_scene_get_info(const rls_nearest_scene *, rls_nearest_scene_info *) { return RLS_OK; }
rls_status rls_nearest_hits(rls_context *, const rls_nearest_scene *, const rls_nearest_rays *, const rls_nearest_found *) { return RLS_OK; }
rls_status rls_nearest_walk_hits(rls_context *, const rls_nearest_scene *, const rls_walk_rays *, int64_t, const rls_nearest_found *) { return RLS_OK; }
rls_status rls_copy_to_device(rls_context *, void *, const void *, size_t) { return RLS_OK; }

} // extern "C"

int main()
{
    using namespace rlsb;
    const Device dev;
    const rls_nearest_mesh mesh = {};
    own::Cases cases;
    cases.push_back({"NearestScene", [&dev, &mesh] { NearestScene s(dev, mesh); }});
    for (int64_t rays : {20, 0}) {
        cases.push_back({"NearestFound all rays " + std::to_string(rays), [&dev, rays] { NearestFound f(dev, rays); }});
        cases.push_back({"NearestFound walk rays " + std::to_string(rays), [&dev, rays] { NearestFound f(dev, rays, NearestFound::ForWalk, 40); }});
        cases.push_back({"NearestFound shadow rays " + std::to_string(rays), [&dev, rays] { NearestFound f(dev, rays, NearestFound::ForShadowWalk); }});
        cases.push_back({"NearestFound bare rays " + std::to_string(rays), [&dev, rays] { NearestFound f(dev, rays, 0u); }});
    }
    cases.push_back({"scene and found", [&dev, &mesh] { NearestScene s(dev, mesh); NearestFound f(dev, 8, NearestFound::ForRouting); }});
    return own::run(cases);
}
