"""CPU: the two-level traversal of librls_nearest_group.so -- rlshaders_amd/csrc_nearest/rls_nearest_group.hpp compiled for the host
with -ffp-contract=off by tests/native/nearest_group_host_check.cpp, over the product's builder.  For each group the program holds
the traversal to its brute force over every instance and triangle bit for bit (differ == 0), at top leaf sizes 1 and 4 and scene
leaf sizes 1 and 8, and this file holds that brute force to group_np (tests/nearest_group_util.py) bit for bit in (hit, instance,
prim, t): the C++ restatement and the numpy one are the same function.  The groups: general placements; coincident instances (the
smaller j wins every tie); a skip pair; parked instances (a NaN matrix, an inf matrix, an empty scene); a singular to_object;
hostile rays (NaN / inf / zero / -0 components, NaN reach, reach 0) in every stream.  The program also checks the top builder
(deterministic, the depth bound, every instance in one leaf) and that the update's union restated on the host gives the
builder's boxes by value (a zero's sign may differ: rls_nearest_refit.hpp) -- at 1, 2, 3, 5 and 2^16 instances too -- and it prints
the top tree's level sizes, from which the update's launch plans of test_gpu_nearest_group_update_edges.py are pinned here.  The same
program runs once more under the address and undefined-behaviour sanitizers, on fewer rays; nothing is loaded into Python.

At 2^16 one-triangle instances on a line (top leaf 1: 17 levels) no ray holds more than 16 top entries and the ray along the
line towards +x holds exactly 16 = depth - 1: instance 0 has the smallest centroid, lies in the left (larger) half of every
split, and a ray of positive direction goes left first, holding the right sibling of every level."""
import numpy as np
import pytest

import nearest_group_host_util as H
import nearest_group_util as G
import nearest_util as U
from nearest_group_util import group_rays, line_rays, skips
from nearest_util import F, NO_PRIM


def check(exe, path, insts, o, d, m, skip, leaves=((1, 1), (4, 8), (1, 8), (4, 1))):
    want = G.group_np(insts, o, d, m, skip)
    for top_leaf, scene_leaf in leaves:
        r = H.run(exe, path, o, d, m, skip, top_leaf, scene_leaf)
        assert r.differ == 0 and r.instances == len(insts) and r.parked == sum(i.parked for i in insts)
        hit = want.hit != 0
        assert np.array_equal(r.hit, hit)
        assert np.array_equal(r.instance[hit], want.instance[hit]) and np.array_equal(r.prim[hit], want.prim[hit])
        assert np.array_equal(r.t[hit].view(np.uint32), want.t[hit].view(np.uint32))
        assert np.array_equal(r.tree_instance, r.instance) and np.array_equal(r.tree_prim, r.prim)
    return want, r


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("group_host")
    return d, H.build(d), H.build(d, sanitize=True)


def _general(n, mesh=None):
    return G.general_instances(U.icosphere(2) if mesh is None else mesh, n, seed=n)


def _two_meshes():
    a, b = U.icosphere(1), U.quad_grid(9)
    x, y = G.general_instances(a, 4, seed=3), G.general_instances(b, 4, seed=4)
    return [v for pair in zip(x, y) for v in pair]


def _parked():
    mesh = U.icosphere(1)
    live = G.general_instances(mesh, 4, seed=12)
    nanA, infB = live[0].A.copy(), live[1].B.copy()
    nanA[2, 1], infB[1, 3] = np.nan, -np.inf
    flatA = live[2].A.copy()
    flatA[1, :3] = 0                                                 # singular: rank 2, every d' has d'_y = 0
    return [live[0], G.Inst(mesh, live[0].B, nanA), live[1], G.Inst(mesh, infB, live[1].A), G.Inst(U.empty_mesh(), live[2].B),
            live[2], G.Inst(mesh, live[2].B, flatA, base=9), live[3]]


GROUPS = {"one": lambda: _general(1), "two": lambda: _general(2), "three": lambda: _general(3), "five": lambda: _general(5),
          "sixty_four": lambda: _general(64, U.icosphere(1)), "two_meshes": _two_meshes, "coincident": G.coincident, "parked": _parked}


@pytest.mark.parametrize("name", list(GROUPS))
def test_two_level_traversal_on_the_host(programs, name):
    d, plain, san = programs
    insts = GROUPS[name]()
    path = H.write_group(d / f"{name}.bin", insts)
    o, d_, m = group_rays(insts, 1500, seed=len(name))
    first, _ = check(plain, path, insts, o, d_, m, None)
    assert (first.hit != 0).sum() > 300
    skip = skips(np.random.default_rng(2), first)
    second, r = check(plain, path, insts, o, d_, m, skip)
    assert r.max_top <= max(r.depth - 1, 0)
    took = (skip[0] == first.instance) & (skip[1] != NO_PRIM) & (first.hit != 0)
    assert took.sum() > 50 and not np.any(took & (second.hit != 0) & (second.instance == first.instance) & (second.prim == first.prim))
    other = (skip[1] != NO_PRIM) & (skip[0] != first.instance)       # the same prim id under another instance id: not skipped
    assert other.sum() > 5 and np.array_equal(second.prim[other], first.prim[other]) and np.array_equal(second.instance[other], first.instance[other])
    if name == "coincident":                                         # instances 2 and 5 are instance 0 again, 4 is 1 again
        hit = first.hit != 0
        assert not np.isin(first.instance[hit], (2, 4, 5)).any() and np.isin(second.instance[second.hit != 0], (2, 4)).any()
    if name == "parked":
        assert not np.isin(first.instance[first.hit != 0], (1, 3, 4)).any() and [i.parked for i in insts] == [False, True, False, True, True, False, False, False]
    # the sanitized program: fewer rays, two leaf pairs
    n = 300
    keep = np.r_[0:n, o.shape[1] - 64:o.shape[1]]
    check(san, path, insts, o[:, keep], d_[:, keep], m[keep], (skip[0][keep], skip[1][keep]), leaves=((1, 1), (4, 8)))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 5])
def test_small_top_trees(programs, n):
    d, plain, _ = programs
    insts = G.line_instances(n)
    path = H.write_group(d / f"line{n}.bin", insts)
    o, d_ = np.array([[-1.0], [0.0], [-0.25]], F), np.array([[1.0], [0.0], [0.0]], F)
    for leaf in (1, 2, 4):
        r = H.run(plain, path, o, d_, top_leaf=leaf, scene_leaf=1)
        assert r.differ == 0 and r.hits == (1 if n else 0)
        assert r.depth <= (int(np.ceil(np.log2(max(n / leaf, 1)))) + 1 if n else 0)
        if n:
            assert r.instance[0] == 0 and r.prim[0] == 0 and r.t[0] == 1.0


@pytest.mark.parametrize("n,leaf", [k for k in G.PLANS if k[0] < G.MAX_INSTANCES])
def test_the_update_plans_of_the_edge_cases(programs, n, leaf):
    """the level sizes the update's launch plan is made from, for the instance counts of test_gpu_nearest_group_update_edges.py:
    a change of the builder that changes a plan fails here, without a GPU.  The parked pattern's instances are parked by the
    program's group_record as by the numpy statement."""
    d, plain, _ = programs
    A, B = G.line_moves(n, "shift")
    which = G.parked_pattern(n)
    insts = G.placed(G.line_triangle(), *G.park(A, B, which))
    o, d_, m = G.line_stream(0.0, 0.75 * n, K=64)
    for new in (G.line_instances(n), insts):
        r = H.run(plain, H.write_group(d / f"plan{n}.bin", new), o, d_, m, top_leaf=leaf, scene_leaf=1)
        assert r.differ == 0 and r.parked == sum(i.parked for i in new)
        if new is not insts:
            assert r.levels == G.PLANS[n, leaf] and len(r.levels) == r.depth and sum(r.levels) == r.top_nodes
    assert sum(i.parked for i in insts) == which.size and np.array_equal(np.flatnonzero([i.parked for i in insts]), which)
    wide, folded = G.update_plan(G.PLANS[n, leaf])
    assert (wide, folded) == {1: (1, 0), 2: (0, 2), 256: (0, 9), 257: (0, 10), 384: (0, 10), 385: (1, 9), 600: (2, 9), 1500: (1, 9)}[n]


def test_the_deepest_top_tree_fills_the_top_stack(programs):
    d, plain, san = programs
    n = G.MAX_INSTANCES
    path = H.write_group(d / "line65536.bin", G.line_instances(n))
    o, dd, want = line_rays(n)
    for exe in (plain, san):
        r = H.run(exe, path, o, dd, top_leaf=1, scene_leaf=1)
        assert r.differ == 0 and r.depth == 17 and r.top_nodes == 2 * n - 1 and r.levels == G.PLANS[n, 1]
        assert r.max_top == G.GROUP_STACK and r.ray_max_top[0] == r.depth - 1 and (r.ray_max_top <= G.GROUP_STACK).all()
        assert np.array_equal(r.instance, want)
        assert r.t[0] == 1.0 and r.prim[0] == 0
