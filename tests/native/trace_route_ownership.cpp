// trace_route_ownership.cpp -- rlsb::HitRoutes (host/rls_trace.hpp) gives back what it allocated, also when one of its
// allocations fails (tests/test_trace_route_ownership.py).  Stand-alone over ownership_harness.hpp, after the pattern of
// trace_queue_ownership.cpp; beside the harness's stubs the constructor calls the scratch size and a copy.
#include "rls_trace.hpp"
#include "ownership_harness.hpp"

extern "C" {
rls_status rls_trace_route_scratch_bytes(int64_t, int, size_t *bytes) { *bytes = 256; return RLS_OK; }
rls_status rls_copy_to_host(rls_context *, void *, const void *, size_t) { return RLS_OK; }
} // extern "C"

int main()
{
    using namespace rlsb;
    const Device dev;
    own::Cases cases;
    for (int64_t rays : {5, 0})
        for (bool slot : {false, true})
            cases.push_back({"HitRoutes rays " + std::to_string(rays) + " slot " + std::to_string(slot),
                             [&dev, rays, slot] { HitRoutes r(dev, rays, 3, slot); }});
    return own::run(cases);
}
