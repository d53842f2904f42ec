"""CPU: the buffer-owning classes of host/rls_trace.hpp give back every device allocation, also when one of them fails.

tests/native/trace_queue_ownership.cpp is built as an integrator builds against the header (g++ -std=c++14 -Wall) but links
neither library: with ownership_harness.hpp it defines rls_device_alloc / rls_device_free over malloc, counting live blocks and
failing the k-th call.  It constructs RayQueue of every kind, ProbeQueue, HitQueues with and without lights and diffuse,
ShadowQueue of every node, ShadowHits in both forms and the four node queue sets with and without lights (n = 5, spp_n = 2,
2 lights, max_hits 3): once unhindered -- N allocations, none live after destruction -- and once per k in 1..N with the k-th
allocation failing -- an rlsb::Error, none live."""
from ownership_util import (ROOT, rows_of, test_a_failing_allocation_throws_and_leaves_nothing_live,  # noqa: F401
                            test_nothing_is_live_after_destruction)

rows = rows_of("trace_queue_ownership", sanitize=False)


def test_the_counting_allocator_is_written_once():
    """in ownership_harness.hpp, for this program and the five after its pattern"""
    programs = sorted((ROOT / "tests" / "native").glob("*_ownership.cpp"))
    assert len(programs) == 6
    for p in programs:
        assert "rls_device_alloc" not in p.read_text() and '#include "ownership_harness.hpp"' in p.read_text(), p.name


def test_every_owning_class_is_constructed(rows):
    want = {f"RayQueue {k}" for k in ("Glossy", "Refract", "DisneyDiffuse", "DisneyGlossy", "NodeDiffuse")}
    want |= {"ProbeQueue", "ShadowHits Direct", "ShadowHits Indexed"}
    want |= {f"HitQueues lights {l} diffuse {d}" for l in (2, 0) for d in (1, 0)}
    want |= {f"ShadowQueue {k}" for k in ("Ggx", "Disney", "Skin", "SkinScatter")}
    want |= {f"{q} lights {l}" for q in ("GgxNodeQueues", "DisneyNodeQueues", "SkinNodeQueues", "SkinBounceQueues") for l in (2, 0)}
    assert set(rows) == want
    assert all(r["n"] >= 2 for r in rows.values()), rows
    # a set is the sum of its parts (SkinNodeQueues: its three scalars are one allocation more)
    for l, shadows in ((2, 1), (0, 0)):
        ray = rows["RayQueue Glossy"]["n"]
        assert rows[f"GgxNodeQueues lights {l}"]["n"] == shadows * rows["ShadowQueue Ggx"]["n"] + ray + rows["RayQueue Refract"]["n"] + \
            rows["RayQueue NodeDiffuse"]["n"]
        assert rows[f"DisneyNodeQueues lights {l}"]["n"] == shadows * rows["ShadowQueue Disney"]["n"] + \
            rows["RayQueue DisneyDiffuse"]["n"] + rows["RayQueue DisneyGlossy"]["n"]
        skin = 2 * shadows * rows["ShadowQueue Skin"]["n"] + 2 * ray + rows["ProbeQueue"]["n"] + 1
        assert rows[f"SkinNodeQueues lights {l}"]["n"] == skin
        assert rows[f"SkinBounceQueues lights {l}"]["n"] == skin + shadows * rows["ShadowQueue SkinScatter"]["n"]
