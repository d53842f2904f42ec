// trace_queue_ownership.cpp -- every buffer-owning class of host/rls_trace.hpp gives back what it allocated, also when one of
// its allocations fails (tests/test_trace_host_ownership.py).  Stand-alone over ownership_harness.hpp, which states the counting
// allocator, the loop and the row per class and argument set; beside its stubs the constructors call the three scratch sizes.
#include "rls_trace.hpp"
#include "ownership_harness.hpp"

extern "C" {
rls_status rls_trace_scratch_bytes(int64_t, int, size_t *bytes) { *bytes = 256; return RLS_OK; }
rls_status rls_trace_shadow_scratch_bytes(int64_t, int, int, size_t *bytes) { *bytes = 256; return RLS_OK; }
rls_status rls_trace_sss_hits_scratch_bytes(int64_t, int, int, int64_t, int, int, size_t *bytes) { *bytes = 256; return RLS_OK; }
} // extern "C"

int main()
{
    using namespace rlsb;
    const Device dev;
    const int64_t n = 5;
    const int spp_n = 2, max_hits = 3;
    const int64_t cap = max_hits * n * spp_n * spp_n;
    own::Cases cases;
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
    return own::run(cases);
}
