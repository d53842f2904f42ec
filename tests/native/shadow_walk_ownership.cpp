// shadow_walk_ownership.cpp -- rlsb::ShadowWalk (host/rls_shadow_walk.hpp) gives back what it allocated, also when one of its
// allocations fails (tests/test_shadow_walk_host_ownership.py).  Stand-alone over ownership_harness.hpp, like
// walk_ownership.cpp; beside the harness's stubs the class calls only its own scratch size, and nothing of the probe walk's
// library.
#include "rls_shadow_walk.hpp"
#include "ownership_harness.hpp"

extern "C" rls_status rls_shadow_walk_scratch_bytes(int64_t, size_t *bytes) { *bytes = 256; return RLS_OK; }

int main()
{
    using namespace rlsb;
    const Device dev;
    own::Cases cases;
    for (int64_t rays : {20, 0})
        cases.push_back({"ShadowWalk rays " + std::to_string(rays), [&dev, rays] { ShadowWalk w(dev, rays); }});
    return own::run(cases);
}
