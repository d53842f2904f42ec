"""CPU: rlsb::ProbeWalk (host/rls_walk.hpp) is the single owner of its device buffers: it gives back every allocation, also when
one of them fails.

tests/native/walk_ownership.cpp is built as an integrator builds against the header (g++ -std=c++14 -Wall, here with the address
and undefined-behaviour sanitizers: a stand-alone host program) but links no library: with ownership_harness.hpp it defines
rls_device_alloc / rls_device_free over malloc, counting live blocks and failing the k-th call.  It constructs the walk with and
without rays and at two max_hits: once unhindered -- N allocations, none live after destruction -- and once per k in 1..N with
the k-th allocation failing -- an rlsb::Error, none live."""
import re

from ownership_util import (HOST, rows_of, test_a_failing_allocation_throws_and_leaves_nothing_live,  # noqa: F401
                            test_nothing_is_live_after_destruction)

HEADER = HOST / "rls_walk.hpp"

rows = rows_of("walk_ownership", sanitize=True)


def test_the_walk_is_constructed_in_every_form(rows):
    assert set(rows) == {f"ProbeWalk rays {r} max_hits {m}" for r in (20, 0) for m in (12, 1)}
    # two lists of 10 buffers (count, ray, origin[3], dir[3], maxdist, trials), the hits' count and 6 planes, the scratch
    assert {r["n"] for r in rows.values()} == {2 * 10 + 7 + 1}


def test_one_owner_in_the_header():
    """every allocation of the class goes through its one DeviceBuffers member; the header frees and allocates nothing by itself,
    and the class cannot be copied"""
    text = HEADER.read_text()
    assert not re.search(r"\brls_device_(alloc|free)\b", text)
    assert text.count("detail::DeviceBuffers bufs_;") == 1
    assert "ProbeWalk(const ProbeWalk &) = delete;" in text and "ProbeWalk &operator=(const ProbeWalk &) = delete;" in text
