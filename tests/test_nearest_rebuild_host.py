"""CPU: the rebuild of librls_nearest_rebuild.so -- rlshaders_amd/csrc_nearest/rls_nearest_rebuild.hpp compiled for the host with
-ffp-contract=off by tests/native/nearest_rebuild_host_check.cpp, over the product's builder.  For each mesh pair (A, B): the tree
is built on A, its shape and levels are read from its links, and the level algorithm -- three lists sorted by a stable radix
sort, the axis from the list ends, a stable partition a level, the leaves' ids sorted -- moves it to B.  The result is held to
nearest_build on B: first, meta (the axis bits included) and the order of the triangle ids exactly, the boxes by value, the
records bit for bit; a rebuild back to A gives the tree built on A; a tree of another shape is refused.

nt in {0, 1, leaf, leaf + 1, 2 leaf + 1, 11, 1000, 4099} x leaf in {1, 3, 4, 8}, on five meshes: random; every triangle the same
(every key ties: the order is the ids'); a flat grid in z = 0 with zeros of both signs and negative coordinates; coordinates
near +-3e38 (a centroid sum of +-inf, an extent of NaN); a soup scaled by 2^-128 (every coordinate, centroid sum and extent is
denormal: the tree still splits along all three axes).  And vertices with NaN and infinities: the parked triangles stand at the
origin.  The same stand-alone program runs once more under the address and undefined-behaviour sanitizers; nothing is loaded
into Python."""
import numpy as np
import pytest

from nearest_rebuild_util import LEAVES, PAIRS, build, hostile_pair, parked_of, run_check, sizes, write_pair


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("rebuild_host")
    return d, build(d), build(d, sanitize=True)


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("name", list(PAIRS))
def test_rebuild_on_the_host_is_the_builders_tree(programs, name, leaf):
    d, plain, san = programs
    for nt in sizes(leaf):
        A, B, tri = PAIRS[name](nt)
        assert tri.shape[0] == nt and np.isfinite(B).all()
        path = write_pair(d / f"{name}_{nt}.bin", A, B, tri)
        for exe in (plain, san) if nt <= 1000 else (plain,):
            r = run_check(exe, path, leaf)
            assert (r["nt"], r["leaf"], r["parked"]) == (nt, leaf, 0), r
            assert r["nodes"] == (0 if nt == 0 else 1 if nt <= leaf else r["nodes"]) and sum(r["axes"]) == (r["nodes"] - 1) // 2 * (nt > 0)
        if name == "flat" and nt >= 1000:
            assert r["axes"][2] == 0 and r["axes"][0] and r["axes"][1], r      # no extent in z: never the longest
        if name == "identical" and nt > leaf:
            assert r["axes"] == [r["nodes"] // 2, 0, 0], r                      # every extent is zero: axis 0 everywhere
        if name == "subnormal" and nt >= 1000:
            assert all(r["axes"]), r                                            # a flushed key or extent: the identical mesh's axes


@pytest.mark.parametrize("leaf", LEAVES)
def test_non_finite_vertices_park_triangles_at_the_origin(programs, leaf):
    d, plain, san = programs
    for nt, exe in ((11, san), (1000, san), (4099, plain)):
        A, B, tri = hostile_pair(nt)
        parked = int(parked_of(B, tri).sum())
        assert 0 < parked < nt
        r = run_check(exe, write_pair(d / f"hostile_{nt}.bin", A, B, tri), leaf)
        assert (r["nt"], r["leaf"], r["parked"]) == (nt, leaf, parked), r
