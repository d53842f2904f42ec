"""CPU: rlsb::NearestScene and rlsb::NearestFound (host/rls_nearest.hpp) are the single owners of what they hold: they give back
every allocation, also when one of them fails.

tests/native/nearest_ownership.cpp is built as an integrator builds against the header (g++ -std=c++14 -Wall, here with the
address and undefined-behaviour sanitizers: a stand-alone host program) but links no library: with ownership_harness.hpp it
defines rls_device_alloc / rls_device_free and the scene's create / destroy over the heap, counting live blocks and failing
the k-th call.  Every form is constructed once unhindered -- N allocations, none live after destruction -- and once per k in
1..N with the k-th failing -- an rlsb::Error, none live (what a k leaves live is reported in its row, then given back the way
it was made: free for a block, delete for a scene)."""
import re

from ownership_util import (HOST, rows_of, test_a_failing_allocation_throws_and_leaves_nothing_live,  # noqa: F401
                            test_nothing_is_live_after_destruction)

HEADER = HOST / "rls_nearest.hpp"

rows = rows_of("nearest_ownership", sanitize=True)


def test_every_form_is_constructed(rows):
    want = {"NearestScene": 1, "scene and found": 1 + 2 + 5 * 3 + 1 + 1}
    for r in (20, 0):
        # hit, t; five vectors of three planes; prim, surface, u, v; bin; last
        want[f"NearestFound all rays {r}"] = 2 + 15 + 4 + 1 + 1
        want[f"NearestFound walk rays {r}"] = 2 + 9 + 1 + 1
        want[f"NearestFound shadow rays {r}"] = 2 + 3 + 1 + 1
        want[f"NearestFound bare rays {r}"] = 2
    assert {k: v["n"] for k, v in rows.items()} == want


def test_one_owner_in_the_header():
    """the found planes go through the class's one DeviceBuffers member, the scene through its one pointer; the header frees and
    allocates nothing by itself, and neither class can be copied"""
    text = HEADER.read_text()
    assert not re.search(r"\brls_device_(alloc|free)\b", text)
    assert text.count("detail::DeviceBuffers bufs_;") == 1 and text.count("rls_nearest_scene_destroy(") == 1
    for cls in ("NearestScene", "NearestFound"):
        assert f"{cls}(const {cls} &) = delete;" in text and f"{cls} &operator=(const {cls} &) = delete;" in text
