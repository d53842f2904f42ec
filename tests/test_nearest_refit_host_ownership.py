"""CPU: rlsb::NearestRefit (host/rls_nearest_refit.hpp) is the single owner of its rls_nearest_refit: it gives it back, also when
its creation fails, and beside the scene it borrows and a NearestFound none of the three leaves anything live.

tests/native/nearest_refit_ownership.cpp is built as an integrator builds against the header (g++ -std=c++14 -Wall, here with the
address and undefined-behaviour sanitizers: a stand-alone host program) but links no library: with ownership_harness.hpp it
defines rls_device_alloc / rls_device_free, the scene's and the refit's create / destroy over the heap, counting live blocks and
failing the k-th call.  Every form is constructed once unhindered -- N allocations, none live after destruction -- and once per k
in 1..N with the k-th failing -- an rlsb::Error, none live (what a k leaves live is reported in its row, then given back the
way it was made)."""
import re

from ownership_util import (HOST, rows_of, test_a_failing_allocation_throws_and_leaves_nothing_live,  # noqa: F401
                            test_nothing_is_live_after_destruction)

HEADER = HOST / "rls_nearest_refit.hpp"

rows = rows_of("nearest_refit_ownership", sanitize=True)


def test_every_form_is_constructed(rows):
    """a refit is one allocation (the scene a lone one borrows is made outside the case); update and readTree allocate nothing
    that is counted; the found of test_nearest_host_ownership.py's "scene and found": hit, t, five vectors of three planes,
    prim, surface"""
    found = 2 + 5 * 3 + 1 + 1
    want = {"NearestRefit": 1, "NearestRefit used": 1, "scene and refit": 2, "scene, refit and found": 2 + found,
            "two refits of one scene": 3}
    assert {k: v["n"] for k, v in rows.items()} == want


def test_one_owner_in_the_header():
    """the refit goes through the class's one pointer; the header frees and allocates nothing on the device by itself, and the
    class cannot be copied"""
    text = HEADER.read_text()
    assert not re.search(r"\brls_device_(alloc|free)\b", text)
    assert text.count("rls_nearest_refit_destroy(") == 1 and text.count("rls_nearest_refit_create(") == 1
    assert "NearestRefit(const NearestRefit &) = delete;" in text and "NearestRefit &operator=(const NearestRefit &) = delete;" in text
