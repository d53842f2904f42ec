// nearest_ownership.cpp -- rlsb::NearestScene and rlsb::NearestFound (host/rls_nearest.hpp) give back what they allocated, also
// when one of their allocations fails (tests/test_nearest_host_ownership.py).  Stand-alone like shadow_walk_ownership.cpp: it
// links no library and needs no GPU; the few C-ABI functions the classes and rlsb::Device call are defined here --
// rls_device_alloc / rls_device_free over malloc and rls_nearest_scene_create / _destroy over new, counting the live blocks and
// failing the k-th call.
//
// Per argument set one line: name, N (the allocations of an unhindered construction), the blocks live after its destruction,
// and over k = 1..N with the k-th allocation failing: the k that left blocks live, the k at which no rlsb::Error was thrown.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <set>
#include <string>
#include <vector>

#include "rls_nearest.hpp"

struct rls_nearest_scene { int unused; };

namespace {
std::set<void *> g_live;
int g_calls = 0, g_fail_at = 0;
} // namespace

extern "C" {

rls_status rls_device_alloc(rls_context *, size_t bytes, void **out)
{
    if (++g_calls == g_fail_at) return RLS_ERR_OUT_OF_MEMORY;
    *out = malloc(bytes > 0 ? bytes : 1);
    g_live.insert(*out);
    return RLS_OK;
}
rls_status rls_device_free(rls_context *, void *p)
{
    if (g_live.erase(p) != 1) { fprintf(stderr, "rls_device_free of a block that is not live\n"); abort(); }
    free(p);
    return RLS_OK;
}
rls_status rls_nearest_scene_create(rls_context *, const rls_nearest_mesh *, rls_nearest_scene **out)
{
    *out = nullptr;
    if (++g_calls == g_fail_at) return RLS_ERR_OUT_OF_MEMORY;
    *out = new rls_nearest_scene();
    g_live.insert(*out);
    return RLS_OK;
}
rls_status rls_nearest_scene_destroy(rls_nearest_scene *s)
{
    if (!s) return RLS_OK;
    if (g_live.erase(s) != 1) { fprintf(stderr, "rls_nearest_scene_destroy of a scene that is not live\n"); abort(); }
    delete s;
    return RLS_OK;
}
rls_status rls_nearest_scene_get_info(const rls_nearest_scene *, rls_nearest_scene_info *) { return RLS_OK; }
rls_status rls_nearest_hits(rls_context *, const rls_nearest_scene *, const rls_nearest_rays *, const rls_nearest_found *) { return RLS_OK; }
rls_status rls_nearest_walk_hits(rls_context *, const rls_nearest_scene *, const rls_walk_rays *, int64_t, const rls_nearest_found *) { return RLS_OK; }
rls_status rls_copy_to_device(rls_context *, void *, const void *, size_t) { return RLS_OK; }
const char *rls_last_error(void) { return "allocation failed (the test's)"; }
const char *rls_status_string(rls_status) { return "status"; }
rls_status rls_context_create(int, rls_context **out) { static int ctx; *out = (rls_context *)&ctx; return RLS_OK; }
void rls_context_destroy(rls_context *) {}
const char *rls_libm_flavour(void) { return "none"; }
rls_status rls_host_libm_matches(int *mismatches) { *mismatches = 0; return RLS_OK; }

} // extern "C"

int main()
{
    using namespace rlsb;
    const Device dev;
    const rls_nearest_mesh mesh = {};
    std::vector<std::pair<std::string, std::function<void()>>> cases;
    cases.push_back({"NearestScene", [&dev, &mesh] { NearestScene s(dev, mesh); }});
    for (int64_t rays : {20, 0}) {
        cases.push_back({"NearestFound all rays " + std::to_string(rays), [&dev, rays] { NearestFound f(dev, rays); }});
        cases.push_back({"NearestFound walk rays " + std::to_string(rays), [&dev, rays] { NearestFound f(dev, rays, NearestFound::ForWalk, 40); }});
        cases.push_back({"NearestFound shadow rays " + std::to_string(rays), [&dev, rays] { NearestFound f(dev, rays, NearestFound::ForShadowWalk); }});
        cases.push_back({"NearestFound bare rays " + std::to_string(rays), [&dev, rays] { NearestFound f(dev, rays, 0u); }});
    }
    cases.push_back({"scene and found", [&dev, &mesh] { NearestScene s(dev, mesh); NearestFound f(dev, 8, NearestFound::ForRouting); }});
    for (const auto &c : cases) {
        g_calls = 0; g_fail_at = 0;
        c.second();
        const int N = g_calls;
        const size_t live = g_live.size();
        std::string leaked, silent;
        for (int k = 1; k <= N; k++) {
            g_live.clear();
            g_calls = 0; g_fail_at = k;
            try {
                c.second();
                silent += (silent.empty() ? "" : ",") + std::to_string(k);
            } catch (const Error &) {
            }
            if (!g_live.empty()) leaked += (leaked.empty() ? "" : ",") + std::to_string(k);
        }
        g_live.clear();
        printf("%s\t%d\t%zu\t%s\t%s\n", c.first.c_str(), N, live, leaked.c_str(), silent.c_str());
    }
    return 0;
}
