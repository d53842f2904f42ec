// trace_queue_ownership.cpp -- every buffer-owning class of host/rls_trace.hpp gives back what it allocated, also when one of
// its allocations fails (tests/test_trace_host_ownership.py).  Stand-alone: it links neither library and needs no GPU; the few
// C-ABI functions the constructors call are defined here -- rls_device_alloc / rls_device_free over malloc, counting the live
// blocks and failing the k-th call, the three scratch sizes, the error strings, and what rlsb::Device needs.
//
// Per class and argument set one line: name, N (the allocations of an unhindered construction), the blocks live after its
// destruction, and over k = 1..N with the k-th allocation failing: the k that left blocks live, the k at which no rlsb::Error
// was thrown.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <set>
#include <string>
#include <vector>

#include "rls_trace.hpp"

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
rls_status rls_trace_scratch_bytes(int64_t, int, size_t *bytes) { *bytes = 256; return RLS_OK; }
rls_status rls_trace_shadow_scratch_bytes(int64_t, int, int, size_t *bytes) { *bytes = 256; return RLS_OK; }
rls_status rls_trace_sss_hits_scratch_bytes(int64_t, int, int, int64_t, int, int, size_t *bytes) { *bytes = 256; return RLS_OK; }
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
    const int64_t n = 5;
    const int spp_n = 2, max_hits = 3;
    const int64_t cap = max_hits * n * spp_n * spp_n;
    std::vector<std::pair<std::string, std::function<void()>>> cases;
    const char *kinds[] = {"Glossy", "Refract", "DisneyDiffuse", "DisneyGlossy", "NodeDiffuse"};
    for (int k = 0; k < 5; k++)
        cases.push_back({std::string("RayQueue ") + kinds[k], [&dev, n, spp_n, k] { RayQueue q(dev, n, spp_n, (RayQueue::Kind)k); }});
    cases.push_back({"ProbeQueue", [&] { ProbeQueue q(dev, n, spp_n); }});
    for (int lights : {2, 0})
        for (bool diffuse : {true, false})
            cases.push_back({"HitQueues lights " + std::to_string(lights) + " diffuse " + std::to_string(diffuse),
                             [&dev, n, spp_n, max_hits, cap, lights, diffuse] { HitQueues q(dev, n, spp_n, max_hits, cap, lights, 2, diffuse); }});
    const char *nodes[] = {"Ggx", "Disney", "Skin", "SkinScatter"};
    for (int k = 0; k < 4; k++)
        cases.push_back({std::string("ShadowQueue ") + nodes[k], [&dev, n, spp_n, k] { ShadowQueue q(dev, n, 2, spp_n, (ShadowQueue::Node)k); }});
    cases.push_back({"ShadowHits Direct", [&] { ShadowHits h(dev, n, max_hits, ShadowHits::Direct); }});
    cases.push_back({"ShadowHits Indexed", [&] { ShadowHits h(dev, n, max_hits, ShadowHits::Indexed); }});
    for (int lights : {2, 0}) {
        const std::string l = " lights " + std::to_string(lights);
        cases.push_back({"GgxNodeQueues" + l, [&dev, n, spp_n, lights] { GgxNodeQueues q(dev, n, lights, spp_n); }});
        cases.push_back({"DisneyNodeQueues" + l, [&dev, n, spp_n, lights] { DisneyNodeQueues q(dev, n, lights, spp_n); }});
        cases.push_back({"SkinNodeQueues" + l, [&dev, n, spp_n, lights] { SkinNodeQueues q(dev, n, lights, spp_n); }});
        cases.push_back({"SkinBounceQueues" + l, [&dev, n, spp_n, lights] { SkinBounceQueues q(dev, n, lights, spp_n); }});
    }

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
