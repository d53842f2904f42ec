"""CPU: the refit of librls_nearest_refit.so -- rlshaders_amd/csrc_nearest/rls_nearest_refit.hpp compiled for the host with
-ffp-contract=off by tests/native/nearest_refit_host_check.cpp, over the product's builder and traversal.  For each mesh pair
(A, B): the tree is built on A and refit to B; every node box == the exact union below it, first, meta and the order of the
triangle ids are unchanged, the traversal == the program's brute force on B bit for bit in (hit, t, prim), and a refit back to A
restores every box and record by value.  The same stand-alone program runs once more under the address and undefined-behaviour
sanitizers, on fewer rays; nothing is loaded into Python.

The program's tree mode gives the tree a scene holds without a device: the trees both launch plans of the device's update are
run on (nearest_refit_util.PLAN_TREES) have the level sizes they were chosen for, and on them the frontier-a-level forms of the
levels and of the union that the deep GPU test needs (levels_fast, union_fast) equal the node-by-node ones."""
import numpy as np
import pytest

import nearest_util as U
from nearest_util import F
from nearest_refit_util import (PLAN_GRIDS, PLAN_TREES, build, jittered, levels_fast, levels_np, profile_np, run_pair, run_tree,
                                 squashed, stacked, union_fast, union_np, write_pair)

RAYS = 100_000


def _jittered():
    m = U.icosphere(2)
    return m.V, jittered(m, 3), m.tri


def _permuted():
    """the vertex positions dealt to other vertices: every triangle is somewhere else, the tree's splits mean nothing"""
    m = U.icosphere(2)
    return m.V, m.V[np.random.default_rng(5).permutation(m.V.shape[0])], m.tri


def _collapsed():
    m = U.icosphere(2)
    return m.V, np.tile(np.array([[0.25, -0.5, 0.125]], F), (m.V.shape[0], 1)), m.tri


def _flattened():
    return U.quad_grid(33).V, U.quad_grid(33, flat=True).V, U.quad_grid(33).tri


def _huge():
    m = U.huge_soup()
    return U.soup(1025).V, m.V, m.tri


def _non_finite():
    m = U.icosphere(2)
    B = jittered(m, 7)
    rng = np.random.default_rng(9)
    bad = rng.permutation(B.shape[0])[:B.shape[0] // 4]
    B[bad, rng.integers(0, 3, bad.size)] = np.array([np.nan, np.inf, -np.inf], F)[rng.integers(0, 3, bad.size)]
    return m.V, B, m.tri


# name -> (the pair, rays, the least share of rays that must hit, the parked triangles expected: None = count them here)
PAIRS = dict(jittered=(_jittered, RAYS, 0.3), permuted=(_permuted, 4_000, 0.0), collapsed=(_collapsed, RAYS, 0.0),
             flattened=(_flattened, RAYS, 0.3), huge=(_huge, RAYS, 0.05), non_finite=(_non_finite, RAYS, 0.1),
             stacked=(stacked, 4_000, 0.3))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("refit_host")
    return d, build(d), build(d, sanitize=True)


@pytest.mark.parametrize("name", list(PAIRS))
def test_refit_on_the_host(programs, name):
    d, plain, san = programs
    make, rays, share = PAIRS[name]
    A, B, tri = make()
    parked = int((~np.isfinite(B[tri.astype(np.int64)]).all(axis=(1, 2))).sum())
    path = write_pair(d / f"{name}.bin", A, B, tri)
    for exe, n, leaves in ((plain, rays, (1, 4, 8)), (san, max(rays // 10, 2000), (1, 4))):
        for leaf in leaves:
            r = run_pair(exe, path, n, leaf)
            print(name, "sanitized" if exe is san else "plain", r)
            assert r["nt"] == tri.shape[0] and r["leaf"] == leaf and r["rays"] == n and r["differ"] == 0
            assert r["parked"] == parked
            assert r["hits"] >= share * n, r
    if name == "non_finite":
        assert tri.shape[0] // 4 < parked < tri.shape[0]             # a quarter of the vertices: most triangles, not all
    if name == "collapsed":
        assert r["hits"] == 0


@pytest.mark.parametrize("nt,leaf", [(nt, 1) for nt in PLAN_TREES] + [(0, leaf) for leaf in PLAN_GRIDS])
def test_plan_trees_and_the_frontier_union(programs, nt, leaf):
    """nt = 0: U.quad_grid(33)"""
    d, plain, _ = programs
    a = U.soup(nt) if nt else U.quad_grid(33)
    B = squashed(a, 3)
    boxes, links, prims = run_tree(plain, write_pair(d / f"plan{nt}_{leaf}.bin", a.V, B, a.tri), leaf)
    assert profile_np(links) == (PLAN_TREES[nt] if nt else PLAN_GRIDS[leaf])
    assert (leaf != 1 or links.shape[0] == 2 * a.nt - 1) and sorted(prims) == list(range(a.nt))
    assert np.array_equal(levels_fast(links), levels_np(links))
    assert np.array_equal(boxes, union_np(boxes, links, prims, a.V, a.tri))              # the builder's boxes are that union
    want = union_np(boxes, links, prims, B, a.tri)
    assert np.array_equal(union_fast(boxes, links, prims, B, a.tri), want) and not np.array_equal(want, boxes)
    # a quarter of the vertices non-finite: the parked triangles' origin enters both forms alike
    B[::4, 1] = np.nan
    assert np.array_equal(union_fast(boxes, links, prims, B, a.tri), union_np(boxes, links, prims, B, a.tri))
