// nearest_refit_ownership.cpp -- rlsb::NearestRefit (host/rls_nearest_refit.hpp) gives back the refit it made, also when its
// creation fails, and beside the scene it borrows and a NearestFound (tests/test_nearest_refit_host_ownership.py).  Stand-alone
// over ownership_harness.hpp, like nearest_ownership.cpp; rls_nearest_refit_create / _destroy and the scene's are defined here
// over new and delete, counted and failed with the device blocks and, like them, given back the way they were made.
#include "rls_nearest_refit.hpp"
#include "ownership_harness.hpp"

struct rls_nearest_scene { int unused; };
struct rls_nearest_refit { int unused; };

namespace {
bool g_counted = true;           // false around the scene that a lone refit borrows: made and given back outside the cases
}

extern "C" {

rls_status rls_nearest_scene_create(rls_context *, const rls_nearest_mesh *, rls_nearest_scene **out)
{
    *out = nullptr;
    if (g_counted && own::fails()) return RLS_ERR_OUT_OF_MEMORY;
    *out = new rls_nearest_scene();
    if (g_counted) own::made(*out, [](void *s) { delete static_cast<rls_nearest_scene *>(s); });
    return RLS_OK;
}
rls_status rls_nearest_scene_destroy(rls_nearest_scene *s)
{
    if (!s) return RLS_OK;
    if (g_counted) own::gone(s, "rls_nearest_scene_destroy of a scene");
    delete s;
    return RLS_OK;
}
rls_status rls_nearest_scene_get_info(const rls_nearest_scene *, rls_nearest_scene_info *) { return RLS_OK; }
rls_status rls_nearest_hits(rls_context *, const rls_nearest_scene *, const rls_nearest_rays *, const rls_nearest_found *) { return RLS_OK; }
rls_status rls_nearest_walk_hits(rls_context *, const rls_nearest_scene *, const rls_walk_rays *, int64_t, const rls_nearest_found *) { return RLS_OK; }
rls_status rls_copy_to_device(rls_context *, void *, const void *, size_t) { return RLS_OK; }

rls_status rls_nearest_refit_create(rls_context *, rls_nearest_scene *, rls_nearest_refit **out)
{
    *out = nullptr;
    if (own::fails()) return RLS_ERR_OUT_OF_MEMORY;
    *out = new rls_nearest_refit();
    own::made(*out, [](void *r) { delete static_cast<rls_nearest_refit *>(r); });
    return RLS_OK;
}
rls_status rls_nearest_refit_destroy(rls_nearest_refit *r)
{
    if (!r) return RLS_OK;
    own::gone(r, "rls_nearest_refit_destroy of a refit");
    delete r;
    return RLS_OK;
}
rls_status rls_nearest_refit_get_info(const rls_nearest_refit *, rls_nearest_refit_info *) { return RLS_OK; }
rls_status rls_nearest_refit_update(rls_context *, rls_nearest_refit *, const rls_nearest_refit_mesh *) { return RLS_OK; }
rls_status rls_nearest_refit_read_tree(rls_context *, const rls_nearest_refit *, float *, uint32_t *, uint32_t *) { return RLS_OK; }

} // extern "C"

int main()
{
    using namespace rlsb;
    const Device dev;
    const rls_nearest_mesh mesh = {};
    g_counted = false;
    NearestScene *borrowed = new NearestScene(dev, mesh);
    g_counted = true;
    own::Cases cases;
    cases.push_back({"NearestRefit", [&dev, borrowed] { NearestRefit r(dev, *borrowed); }});
    cases.push_back({"NearestRefit used", [&dev, borrowed] {
        NearestRefit r(dev, *borrowed);
        std::vector<float> boxes;
        std::vector<uint32_t> links, prims;
        r.update(nullptr);
        r.readTree(boxes, links, prims);
    }});
    cases.push_back({"scene and refit", [&dev, &mesh] { NearestScene s(dev, mesh); NearestRefit r(dev, s); }});
    cases.push_back({"scene, refit and found", [&dev, &mesh] {
        NearestScene s(dev, mesh);
        NearestRefit r(dev, s);
        NearestFound f(dev, 8, NearestFound::ForRouting);
    }});
    cases.push_back({"two refits of one scene", [&dev, &mesh] { NearestScene s(dev, mesh); NearestRefit a(dev, s), b(dev, s); }});
    const int status = own::run(cases);
    g_counted = false;
    delete borrowed;
    return status;
}
