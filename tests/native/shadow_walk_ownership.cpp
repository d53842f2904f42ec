// shadow_walk_ownership.cpp -- rlsb::ShadowWalk (host/rls_shadow_walk.hpp) gives back what it allocated, also when one of its
// allocations fails (tests/test_shadow_walk_host_ownership.py).  Stand-alone like walk_ownership.cpp: it links no library and needs
// no GPU; the few C-ABI functions the class and rlsb::Device call are defined here -- rls_device_alloc / rls_device_free over
// malloc, counting the live blocks and failing the k-th call, the scratch size, the error strings.
//
// Per argument set one line: name, N (the allocations of an unhindered construction), the blocks live after its destruction,
// and over k = 1..N with the k-th allocation failing: the k that left blocks live, the k at which no rlsb::Error was thrown.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <set>
#include <string>
#include <vector>

#include "rls_shadow_walk.hpp"

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
rls_status rls_shadow_walk_scratch_bytes(int64_t, size_t *bytes) { *bytes = 256; return RLS_OK; }
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
    std::vector<std::pair<std::string, std::function<void()>>> cases;
    for (int64_t rays : {20, 0})
        cases.push_back({"ShadowWalk rays " + std::to_string(rays), [&dev, rays] { ShadowWalk w(dev, rays); }});
    for (const auto &c : cases) {
        g_calls = 0; g_fail_at = 0;
        c.second();
        const int N = g_calls;
        const size_t live = g_live.size();
        std::string leaked, silent;
        for (int k = 1; k <= N; k++) {
            for (void *p : g_live) free(p);                      // (what an earlier k left behind is not this k's)
            g_live.clear();
            g_calls = 0; g_fail_at = k;
            try {
                c.second();
                silent += (silent.empty() ? "" : ",") + std::to_string(k);
            } catch (const Error &) {
            }
            if (!g_live.empty()) leaked += (leaked.empty() ? "" : ",") + std::to_string(k);
        }
        for (void *p : g_live) free(p);
        g_live.clear();
        printf("%s\t%d\t%zu\t%s\t%s\n", c.first.c_str(), N, live, leaked.c_str(), silent.c_str());
    }
    return 0;
}
