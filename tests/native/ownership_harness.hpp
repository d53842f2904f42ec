// ownership_harness.hpp -- what the stand-alone *_ownership.cpp programs share (tests/ownership_util.py builds and runs them): a
// program includes the host header under test, then this one, defines the C-ABI functions only its classes call, and hands
// run() its cases.  It links no library and needs no GPU: rls_device_alloc / rls_device_free are defined here over malloc,
// counting the live blocks and failing the k-th call, with the error strings and what rlsb::Device needs.
//
// Per case one line: name, N (the allocations of an unhindered construction), the blocks live after its destruction, and over
// k = 1..N with the k-th allocation failing: the k that left blocks live, the k at which no rlsb::Error was thrown.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "rls_trace.hpp"

namespace own {
namespace {
std::map<void *, void (*)(void *)> g_live;                       // every live block and what gives it back
int g_calls = 0, g_fail_at = 0;
} // namespace

// an allocating stub begins with `if (own::fails()) return RLS_ERR_OUT_OF_MEMORY;` and ends with made(); a releasing one
// begins with gone()
inline bool fails() { return ++g_calls == g_fail_at; }
inline void made(void *p, void (*release)(void *)) { g_live[p] = release; }
inline void gone(void *p, const char *what)
{
    if (g_live.erase(p) != 1) { fprintf(stderr, "%s that is not live\n", what); abort(); }
}
inline void release_leftovers()                                  // (what an earlier k left behind is not this k's)
{
    for (const auto &b : g_live) b.second(b.first);
    g_live.clear();
}

using Cases = std::vector<std::pair<std::string, std::function<void()>>>;

inline int run(const Cases &cases)
{
    for (const auto &c : cases) {
        g_calls = 0; g_fail_at = 0;
        c.second();
        const int N = g_calls;
        const size_t live = g_live.size();
        std::string leaked, silent;
        for (int k = 1; k <= N; k++) {
            release_leftovers();
            g_calls = 0; g_fail_at = k;
            try {
                c.second();
                silent += (silent.empty() ? "" : ",") + std::to_string(k);
            } catch (const rlsb::Error &) {
            }
            if (!g_live.empty()) leaked += (leaked.empty() ? "" : ",") + std::to_string(k);
        }
        release_leftovers();
        printf("%s\t%d\t%zu\t%s\t%s\n", c.first.c_str(), N, live, leaked.c_str(), silent.c_str());
    }
    return 0;
}
} // namespace own

extern "C" {

rls_status rls_device_alloc(rls_context *, size_t bytes, void **out)
{
    if (own::fails()) return RLS_ERR_OUT_OF_MEMORY;
    *out = malloc(bytes > 0 ? bytes : 1);
    own::made(*out, free);
    return RLS_OK;
}
rls_status rls_device_free(rls_context *, void *p)
{
    own::gone(p, "rls_device_free of a block");
    free(p);
    return RLS_OK;
}
const char *rls_last_error(void) { return "allocation failed (the test's)"; }
const char *rls_status_string(rls_status) { return "status"; }
rls_status rls_context_create(int, rls_context **out) { static int ctx; *out = (rls_context *)&ctx; return RLS_OK; }
void rls_context_destroy(rls_context *) {}
const char *rls_libm_flavour(void) { return "none"; }
rls_status rls_host_libm_matches(int *mismatches) { *mismatches = 0; return RLS_OK; }

} // extern "C"
