"""CPU: rlsb::HitRoutes (host/rls_trace.hpp) gives back every device allocation, also when one of them fails.

tests/native/trace_route_ownership.cpp is built as an integrator builds against the header (g++ -std=c++14 -Wall) but links
neither library (tests/test_trace_host_ownership.py): it constructs HitRoutes with and without slot, for 5 rays and for none:
once unhindered -- N allocations (offsets, order, the scratch; slot one more), none live after destruction -- and once per k in
1..N with the k-th allocation failing -- an rlsb::Error, none live."""
from ownership_util import (rows_of, test_a_failing_allocation_throws_and_leaves_nothing_live,  # noqa: F401
                            test_nothing_is_live_after_destruction)

rows =rows_of("trace_route_ownership", sanitize=False)


def test_the_allocations_of_every_form(rows):
    assert set(rows) == {f"HitRoutes rays {r} slot {s}" for r in (5, 0) for s in (0, 1)}
    for r in (5, 0):
        assert rows[f"HitRoutes rays {r} slot 0"]["n"] == 3 and rows[f"HitRoutes rays {r} slot 1"]["n"] == 4
