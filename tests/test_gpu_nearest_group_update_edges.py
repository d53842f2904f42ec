"""-m gpu: rls_nearest_group_update (librls_nearest_group.so) at every launch plan.  The update writes the records
(group_records_kernel), then one group_level_kernel per level that is not part of the top of the tree, then ONE workgroup
(group_top_kernel) over the levels from the root down of at most 256 nodes each.  Groups of one-triangle instances on a line
(the cost is the instance count), moved by new matrices for every instance:

    n      leaf  levels (root first)             launches of a level   folded   parked
    1      1     1                               1 (the root alone)    0        0
    2      1     1 2                             0                     2        0
    256    1     1 .. 256                        0                     9        0
    257    1     1 .. 256, 2                     0                     10       0       (one leaf more: still all folded)
    384    1     1 .. 256, 256                   0                     10       32      (the last all-folded plan)
    385    1     1 .. 256, 258                   1                     9        33      (a level grows by two: the first wide one)
    600    1     1 .. 256, 512, 176              2                     9        76      (two tiles beside a narrow deepest level)
    1500   4     1 .. 256, 512                   1                     9        192
    65536  1     1 .. 256, 512 .. 65536          8                     9        8160

Each case reads the level sizes from read_tree()'s links and asserts the plan it claims (nearest_group_util.PLANS, pinned on the
CPU by test_nearest_group_host.py), then, exactly: the world boxes equal world_box over the new placements and the fresh
group's; every top node's box is the union of what is below it; the parked flags and the parked count (a tensor pre-filled with
a sentinel) equal the inputs'; about 512 rays return, in every plane, the bytes of a fresh group over the new placements, and
group_np (2^16: the host program's brute force).  From 384 instances on about one instance in seven is parked -- a NaN in A, an
inf in B, a finite B whose box overflows -- so that some workgroups park none, some in all four waves, some in one wave, and the
last partial tile some.  Also: the line reversed and every placement shrunk onto one point (the old tree is then as bad as it
can be); update(None, None) after a member scene's refit at 600, and after a member scene's REBUILD (600 placements of the
icosphere, twisted and carried out of its old box: records permuted and axes rewritten under the group), twice more with no
query between; two updates in a row without a query between."""
import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_group_host_util as H
import nearest_group_util as G
import nearest_util as U
from nearest_refit_util import twisted
from nearest_util import F
from test_gpu_nearest import _dev, _host
from test_gpu_nearest_group import DeviceGroup, all_bytes, check_found, query

pytestmark = pytest.mark.gpu
SENTINEL = -0x5A5A5A5A5A5A5A5B


@pytest.fixture(scope="module")
def ctx():
    from rlshaders_amd import nearest_group, nearest_rebuild, nearest_refit
    nearest_group.load(), nearest_refit.load(), nearest_rebuild.load()          # (a missing library is an error, not a build)
    c = R.Context(0)
    yield c
    c.close()


def new_placements(n, kind, park=True):
    A, B = G.line_moves(n, kind)
    which = G.parked_pattern(n) if park else np.zeros(0, np.int64)
    return G.placed(G.line_triangle(), *G.park(A, B, which)), which


def stream_for(n, kind):
    lo, hi = {"shift": (0.0, 0.75 * n), "reverse": (0.0, float(n)), "point": (2.0, 4.0)}[kind]
    return G.line_stream(lo, hi, seed=n % 1000 + len(kind))


def check_plan(group, n, leaf):
    links = group.read_tree()[1]
    sizes = G.level_sizes(links)
    assert sizes == G.PLANS[n, leaf], sizes
    wide, folded = G.update_plan(sizes)
    assert wide + folded == group.info()["top_depth"]
    return wide, folded


def check_tree(group, new, fresh, parked, which):
    """the read tree after an update to the placements `new`, exactly"""
    boxes, links, order, world, flags = group.read_tree()
    want = np.stack([np.concatenate([i.wlo, i.whi]) for i in new])
    assert np.array_equal(world, want)
    assert np.array_equal(world, fresh.read_tree()[3])
    assert np.array_equal(np.flatnonzero(flags), which) and int(parked.item()) == which.size
    assert np.array_equal(np.sort(order), np.arange(len(new)))
    first, count = links[:, 0].astype(np.int64), links[:, 1].astype(np.int64) & 0xFF
    inner = np.flatnonzero(count == 0)
    below = boxes[first[inner][:, None] + np.arange(2)]              # [inner, 2, 6]: every top node's box is the union of what is below it
    assert np.array_equal(boxes[inner], np.concatenate([below[:, :, :3].min(axis=1), below[:, :, 3:].max(axis=1)], axis=1))
    for k in np.unique(count[count > 0]):
        leaves = np.flatnonzero(count == k)
        below = world[order[first[leaves][:, None] + np.arange(k)]]
        assert np.array_equal(boxes[leaves], np.concatenate([below[:, :, :3].min(axis=1), below[:, :, 3:].max(axis=1)], axis=1)), k
    assert inner.size + (count > 0).sum() == links.shape[0]


def sentinel():
    return torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")


def update_and_check(ctx, g, n, kind, park=True, rays=None, reference="numpy", host=None):
    """one update of the DeviceGroup g to line_moves(n, kind), held to a fresh group and to the statement"""
    new, which = new_placements(n, kind, park)
    A, B = G.matrices(new)
    parked = sentinel()
    g.group.update(_dev(A), _dev(B), parked=parked)
    o, d, m = stream_for(n, kind) if rays is None else rays
    f, _, _ = query(ctx, g.group, o, d, m)
    fresh = DeviceGroup(ctx, new, leaf=g.group.leaf_size, scene_leaf=1)
    try:
        check_tree(g.group, new, fresh.group, parked, which)
        for x, y in zip(all_bytes(f), all_bytes(query(ctx, fresh.group, o, d, m)[0])):
            assert np.array_equal(x, y)
    finally:
        fresh.close()
    if reference == "numpy":
        h = G.group_np(new, o, d, m)
        hits = (h.hit != 0).mean()
        check_found(f, h, d.shape[1], (n, kind))
    else:
        exe, directory = host
        r = H.run(exe, H.write_group(directory / f"moved{n}{kind}.bin", new), o, d, m, top_leaf=1, scene_leaf=1)
        assert r.differ == 0 and r.parked == which.size
        hit = _host(f.hit) != 0
        hits = hit.mean()
        assert np.array_equal(hit, r.hit)
        assert np.array_equal(_host(f.instance).view(np.uint32)[hit], r.instance[hit])
        assert np.array_equal(_host(f.prim).view(np.uint32)[hit], r.prim[hit])
        assert np.array_equal(_host(f.t).view(np.uint32)[hit], r.t.view(np.uint32)[hit])
    assert 0.2 < hits < 0.98, hits
    return new, which


CASES = [(1, 1, 1, 0, 0), (2, 1, 0, 2, 0), (256, 1, 0, 9, 0), (257, 1, 0, 10, 0), (384, 1, 0, 10, 32), (385, 1, 1, 9, 33),
         (600, 1, 2, 9, 76), (1500, 4, 1, 9, 192)]


@pytest.mark.parametrize("n,leaf,wide,folded,parks", CASES)
def test_every_launch_plan(ctx, n, leaf, wide, folded, parks):
    g = DeviceGroup(ctx, G.line_instances(n), leaf=leaf, scene_leaf=1)
    try:
        assert check_plan(g.group, n, leaf) == (wide, folded)
        _, which = update_and_check(ctx, g, n, "shift", park=parks > 0)
        assert which.size == parks
        assert g.group.info()["updates"] == 1
    finally:
        g.close()


def test_the_parked_pattern_reaches_every_kind_of_workgroup():
    """what the counts of the table stand for: per tile of 256 instances, tiles that park none, tiles that park in all four
    waves, tiles that park in one wave alone, and a last partial tile that parks some -- and all three ways of parking"""
    for n in (600, G.MAX_INSTANCES):
        which = G.parked_pattern(n)
        per_wave = np.bincount(which // 64, minlength=-(-n // 64))
        per_wave = np.concatenate([per_wave, np.zeros(-per_wave.size % 4, np.int64)]).reshape(-1, 4)
        waves = (per_wave > 0).sum(axis=1)
        assert (waves == 0).any() and (waves == 4).any() and (6.0 < n / which.size < 8.5)
        if n == 600:
            assert list(waves) == [0, 4, 1] and per_wave[2].sum() == 12 and which.size == 76
        else:
            assert (waves == 1).any() and which.size == 8160
        A, B = G.park(*G.line_moves(n, "shift"), which)
        nan, inf = np.isnan(A).any(axis=(1, 2)), np.isinf(B).any(axis=(1, 2))
        big = np.isfinite(A).all(axis=(1, 2)) & np.isfinite(B).all(axis=(1, 2)) & (np.abs(B).max(axis=(1, 2)) > 1e38)
        assert min(nan.sum(), inf.sum(), big.sum()) >= which.size // 3 and nan.sum() + inf.sum() + big.sum() == which.size


@pytest.mark.parametrize("kind", ["reverse", "point"])
def test_instances_moved_against_the_tree(ctx, kind):
    """the tree was built over the line: reversed, every inner node's two boxes overlap as much as they can; shrunk onto one
    point, every box of the tree is the same box and every hit a tie of all live instances, which instance 0 wins"""
    n = 600
    g = DeviceGroup(ctx, G.line_instances(n), leaf=1, scene_leaf=1)
    try:
        assert check_plan(g.group, n, 1) == (2, 9)
        new, which = update_and_check(ctx, g, n, kind)
        assert which.size == 76
        if kind == "point":
            o, d, m = stream_for(n, kind)
            f, _, _ = query(ctx, g.group, o, d, m)
            hit = _host(f.hit) != 0
            assert hit.sum() > 100 and (_host(f.instance)[hit] == 0).all()
    finally:
        g.close()


def test_the_matrices_stay_after_a_refit_of_the_member_scene(ctx):
    from rlshaders_amd import nearest_refit
    n = 600
    old = G.line_instances(n)
    mesh = old[0].mesh
    g = DeviceGroup(ctx, old, leaf=1, scene_leaf=1)
    try:
        assert check_plan(g.group, n, 1) == (2, 9)
        refit = nearest_refit.Refit(g.scenes[id(mesh)])
        V = (mesh.V * F([1.0, 1.5, 0.75]) + F([0.25, 0.125, -0.25])).astype(F)      # outside the old box in x and y
        refit.update(_dev(V))
        parked = sentinel()
        g.group.update(None, None, parked=parked)
        moved = U.Mesh(V, mesh.tri, surface=mesh.surface)
        new = G.placed(moved, *G.matrices(old), bases=[i.base for i in old])
        o, d, m = G.line_stream(0.0, float(n), seed=9)
        f, _, _ = query(ctx, g.group, o, d, m)
        fresh = DeviceGroup(ctx, new, leaf=1, scene_leaf=1)
        try:
            check_tree(g.group, new, fresh.group, parked, np.zeros(0, np.int64))
            for x, y in zip(all_bytes(f), all_bytes(query(ctx, fresh.group, o, d, m)[0])):
                assert np.array_equal(x, y)
        finally:
            fresh.close()
        h = G.group_np(new, o, d, m)
        assert 0.2 < (h.hit != 0).mean() < 0.98 and not np.array_equal(h.t, G.group_np(old, o, d, m).t)
        check_found(f, h, d.shape[1], "refit")
        refit.close()
    finally:
        g.close()


def test_the_matrices_stay_after_a_rebuild_of_the_member_scene(ctx):
    """the rebuild's twin of the test above, on a mesh whose tree a move can change: 600 placements of the 80-triangle icosphere
    along the line.  The member scene is rebuilt for the mesh twisted by 2 rad and carried outside its old root box -- the
    records under the group are permuted and split axes rewritten, which no refit does -- then update(None, None)"""
    from rlshaders_amd import nearest_rebuild
    n = 600
    line = G.line_instances(n)
    mesh = U.icosphere(1)
    old = G.placed(mesh, *G.matrices(line), bases=[i.base for i in line])
    g = DeviceGroup(ctx, old, leaf=1, scene_leaf=1)
    try:
        assert check_plan(g.group, n, 1) == (2, 9)
        rb = nearest_rebuild.Rebuild(g.scenes[id(mesh)])
        _, links0, prims0 = rb.read_tree()
        V = (twisted(mesh.V, 2.0).astype(np.float64) + np.array([3.0, 0.5, 0.0])).astype(F)
        lo0, hi0 = G.mesh_box(mesh)
        assert V[:, 0].min() > hi0[0] + 1.0                           # well outside the old root box
        rb.update(_dev(V))
        _, links, prims = rb.read_tree()
        assert np.array_equal(np.sort(prims), np.arange(mesh.nt)) and links.shape == links0.shape
        assert not np.array_equal(prims, prims0) or not np.array_equal(links, links0)       # another order or other axes: no refit's tree
        parked = sentinel()
        g.group.update(None, None, parked=parked)
        moved = U.Mesh(V, mesh.tri, surface=mesh.surface, normals=mesh.normals)
        new = G.placed(moved, *G.matrices(old), bases=[i.base for i in old])
        o, d, m = G.line_stream(0.0, float(n), seed=9)
        h, still = G.group_np(new, o, d, m), G.group_np(old, o, d, m)
        assert 0.2 < (h.hit != 0).mean() < 0.98 and not np.array_equal(h.hit, still.hit)
        fresh = DeviceGroup(ctx, new, leaf=1, scene_leaf=1)
        try:
            want = all_bytes(query(ctx, fresh.group, o, d, m)[0])

            def check():
                f, _, _ = query(ctx, g.group, o, d, m)
                check_tree(g.group, new, fresh.group, parked, np.zeros(0, np.int64))
                for x, y in zip(all_bytes(f), want):
                    assert np.array_equal(x, y)
                check_found(f, h, d.shape[1], "rebuild")
                assert not np.array_equal(_host(f.hit), still.hit)
                return g.group.read_tree()

            once = check()
            # twice more with no query between the two: nothing changes
            parked.fill_(SENTINEL)
            g.group.update(None, None)
            g.group.update(None, None, parked=parked)
            for x, y in zip(check(), once):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
            assert g.group.info()["updates"] == 3
        finally:
            fresh.close()
        rb.close()
    finally:
        g.close()


def test_two_updates_in_a_row(ctx):
    """no query and no read between them: the second update's launches follow the first's on the stream"""
    n = 600
    g = DeviceGroup(ctx, G.line_instances(n), leaf=1, scene_leaf=1)
    try:
        first, _ = new_placements(n, "point", park=False)
        A, B = G.matrices(first)
        parked = sentinel()
        g.group.update(_dev(A), _dev(B), parked=parked)
        update_and_check(ctx, g, n, "shift")
        assert g.group.info()["updates"] == 2
    finally:
        g.close()


# ---- 2^16 instances: 17 levels, the eight deepest launched one by one -----------------------------------------------------------------
@pytest.fixture(scope="module")
def deepest(ctx):
    g = DeviceGroup(ctx, G.line_instances(G.MAX_INSTANCES), leaf=1, scene_leaf=1)
    yield g
    g.close()


def test_the_deepest_plan(ctx, deepest, tmp_path):
    n = G.MAX_INSTANCES
    assert check_plan(deepest.group, n, 1) == (8, 9)
    _, which = update_and_check(ctx, deepest, n, "shift", reference="host", host=(H.build(tmp_path), tmp_path))
    assert which.size == 8160
