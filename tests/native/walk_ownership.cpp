// walk_ownership.cpp -- rlsb::ProbeWalk (host/rls_walk.hpp) gives back what it allocated, also when one of its allocations fails
// (tests/test_walk_host_ownership.py).  Stand-alone over ownership_harness.hpp, which states the counting allocator, the loop
// and the row per case; beside them the class calls only the scratch size.
#include "rls_walk.hpp"
#include "ownership_harness.hpp"

extern "C" rls_status rls_walk_scratch_bytes(int64_t, size_t *bytes) { *bytes = 256; return RLS_OK; }

int main()
{
    using namespace rlsb;
    const Device dev;
    own::Cases cases;
    for (int64_t rays : {20, 0})
        for (int max_hits : {12, 1})
            cases.push_back({"ProbeWalk rays " + std::to_string(rays) + " max_hits " + std::to_string(max_hits),
                             [&dev, rays, max_hits] { ProbeWalk w(dev, rays, max_hits); }});
    return own::run(cases);
}
