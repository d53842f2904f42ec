"""-m gpu: rls_nearest_rebuild_update (librls_nearest_rebuild.so, rlshaders_amd/nearest_rebuild.py) rebuilds a scene's tree for a
moved mesh on the device, and the scene then holds the tree a FRESH nearest.Scene on the moved vertices holds -- the reference
throughout, its tree read through a nearest_refit.Refit(fresh).read_tree(): links (the split axes included) and the triangle ids
in leaf order exactly, the boxes by value.

The shapes of the CPU check (nt in {0, 1, leaf, leaf + 1, 2 leaf + 1, 11, 1000, 4099} x leaf in {1, 3, 4, 8} on the random, the
identical, the flat, the huge and the subnormal mesh -- five meshes; on the last the device's key add and extent subtract must
keep denormals, or every key ties); nt about the sort's and the scan's tile of 256 elements (255, 256, 257, 769: the three
lists are one array of 3 nt positions, so the scan's tiles end at other places than the sort's, which are a list's own) and a
deep tree, nt = 65 539 at leaf 1 (17 rounds, a scan whose tile sums take more than one run of the single workgroup).  Queries of
both entry points after a 2 rad twist, `last` set before the rebuild; the traversal's cost; hostile vertices; the interplay with
a refit made before; a graph replayed over changing vertices and a second stream; trees whose root is a leaf."""
import json
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_util as U
from nearest_util import F, NO_PRIM
from nearest_rebuild_util import LEAVES, PAIRS, TILE, flat_grid, hostile_pair, parked_of, same_tree, sizes
from nearest_refit_util import COUNT_MASK, twisted, without
from test_gpu_nearest import SCALAR, VEC, _bytes, _dev, _host, _ids
from trace_abi_util import ROOT

pytestmark = pytest.mark.gpu

NAMES = ("hit", "t") + VEC + SCALAR


@pytest.fixture(scope="module")
def ctx():
    from rlshaders_amd import nearest, nearest_rebuild, nearest_refit
    nearest.load(), nearest_refit.load(), nearest_rebuild.load()     # (a missing library is an error, not a build)
    c = R.Context(0)
    yield c
    c.close()


def scene_on(ctx, V, tri, leaf=0, surface=None, normals=None):
    from rlshaders_amd import nearest
    return nearest.Scene(ctx, V, tri, surface=surface, normals=normals, leaf_size=leaf)


def fresh_tree(ctx, V, tri, leaf):
    """the reference: the tree of a fresh scene on V, read through a refit of it that is never updated"""
    from rlshaders_amd import nearest_refit
    fresh = scene_on(ctx, V, tri, leaf)
    reader = nearest_refit.Refit(fresh)
    tree = reader.read_tree()
    reader.close(), fresh.close()
    return tree


def rebuilt_tree(ctx, A, B, tri, leaf, parked=None):
    """a scene made on A, rebuilt to B -> (its tree, the scene's info before and after, the rebuild's info)"""
    from rlshaders_amd import nearest_rebuild
    scene = scene_on(ctx, A, tri, leaf)
    before = (scene.nv, scene.nt, scene.nodes, scene.depth)
    rb = nearest_rebuild.Rebuild(scene)
    rb.update(_dev(B), parked=parked)
    tree, info = rb.read_tree(), rb.info()
    assert before == (info["nv"], info["nt"], info["nodes"], info["levels"]) and info["updates"] == 1
    assert (info["device_bytes"] > 0) == (len(tri) > 0)
    rb.close(), scene.close()
    return tree


# ---- the tree --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("name", list(PAIRS))
def test_the_rebuilt_tree_is_a_fresh_scenes(ctx, name, leaf):
    for nt in sizes(leaf):
        A, B, tri = PAIRS[name](nt)
        got, want = rebuilt_tree(ctx, A, B, tri, leaf), fresh_tree(ctx, B, tri, leaf)
        assert same_tree(got, want) is None, (name, leaf, nt, same_tree(got, want))
        if nt > leaf:
            # a rebuild that does nothing cannot pass: the tree on A is another one
            assert same_tree(fresh_tree(ctx, A, tri, leaf), want) is not None, (name, leaf, nt)


@pytest.mark.parametrize("leaf", [1, 4])
@pytest.mark.parametrize("nt", [TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_sizes_at_the_tile_edges(ctx, nt, leaf):
    for name in ("random", "flat", "subnormal"):
        A, B, tri = PAIRS[name](nt)
        got, want = rebuilt_tree(ctx, A, B, tri, leaf), fresh_tree(ctx, B, tri, leaf)
        assert same_tree(got, want) is None, (name, leaf, nt, same_tree(got, want))


def test_a_deep_tree(ctx):
    nt = 65_539
    A, B, tri = PAIRS["random"](nt)
    got, want = rebuilt_tree(ctx, A, B, tri, 1), fresh_tree(ctx, B, tri, 1)
    assert want[1].shape[0] == 2 * nt - 1 and 3 * nt > TILE * TILE          # the scan's tile sums: more than one run
    assert same_tree(got, want) is None, same_tree(got, want)


@pytest.mark.parametrize("nt,leaf", [(0, 4), (1, 1), (1, 4), (3, 4), (4, 4), (8, 8)])
def test_a_root_that_is_a_leaf(ctx, nt, leaf):
    """an empty scene, one triangle, nt <= leaf: an update is accepted, the one node stays a leaf and holds the ids ascending"""
    from rlshaders_amd import nearest_rebuild
    A, B, tri = PAIRS["random"](nt)
    scene = scene_on(ctx, A, tri, leaf)
    rb = nearest_rebuild.Rebuild(scene)
    _, links0, prims0 = rb.read_tree()
    parked = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    rb.update(_dev(B), parked=parked)
    boxes, links, prims = rb.read_tree()
    assert int(parked.item()) == 0 and rb.info()["updates"] == 1 and rb.info()["levels"] == (1 if nt else 0)
    assert np.array_equal(links, links0) and np.array_equal(prims, np.arange(nt, dtype=np.uint32))
    assert links.shape[0] == (1 if nt else 0) and (nt == 0 or (links[0, 1] & COUNT_MASK) == nt)
    assert same_tree((boxes, links, prims), fresh_tree(ctx, B, tri, leaf)) is None
    rb.close(), scene.close()


# ---- queries ---------------------------------------------------------------------------------------------------------------------------
def twist_meshes():
    sphere = U.icosphere(3)
    grid = flat_grid(2178)
    grid = U.Mesh(grid.V, grid.tri, surface=grid.surface, normals=np.tile(np.array([[0, 0, 1]], F), (grid.V.shape[0], 1)))
    return dict(sphere=sphere, grid=grid)


def stream(mesh, B, seed, n_grid=16, n_loose=256):
    """a coherent grid of parallel rays over the mesh's extent, and incoherent rays aimed at the moved triangles"""
    rng = np.random.default_rng(seed)
    lo, hi = B.min(axis=0) - 0.1, B.max(axis=0) + 0.1
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], n_grid), np.linspace(lo[1], hi[1], n_grid))
    og = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, hi[2] + 1.0)]).astype(F)
    dg = np.tile(np.array([[0.02], [0.01], [-1.0]], F), (1, gx.size))
    ol, dl = U.rays_at_targets(rng, U.interior_targets(rng, U.Mesh(B, mesh.tri), n_loose, margin=0.0), spread=2.0)
    return np.concatenate([og, ol], 1), np.concatenate([dg, dl], 1)


def both_entry_points(ctx, scene, o, d, last0):
    """rls_nearest_hits and rls_nearest_walk_hits over the same rays, `last` read and written -> every found plane's bytes"""
    from rlshaders_amd import nearest
    n = d.shape[1]
    out = []
    zeros = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")      # (a miss leaves its planes as they are)
    last = _ids(last0)
    f = scene.hits(nearest.Rays(_dev(o), _dev(d)), last=last, found=nearest.Found(ctx, n, alloc=zeros))
    torch.cuda.synchronize()
    out += _bytes(f, NAMES) + [_host(last)]
    last = _ids(last0)
    lst = SimpleNamespace(count=torch.tensor([n], dtype=torch.int64, device="cuda"), ray=_ids(np.arange(n)), origin=_dev(o), dir=_dev(d),
                          maxdist=_dev(np.full(n, np.inf, F)), trials=torch.zeros(n, dtype=torch.uint8, device="cuda"))
    g = scene.hits(lst, active=n, last=last, found=nearest.Found(ctx, n, alloc=zeros))
    torch.cuda.synchronize()
    out += _bytes(g, NAMES) + [_host(last)]
    return out


@pytest.mark.parametrize("leaf", [1, 4])
@pytest.mark.parametrize("name", ["sphere", "grid"])
def test_queries_after_a_twist_are_a_fresh_scenes_bytes(ctx, name, leaf):
    from rlshaders_amd import nearest, nearest_rebuild
    mesh = twist_meshes()[name]
    B = twisted(mesh.V, 2.0)
    o, d = stream(mesh, B, 5)
    n = d.shape[1]
    scene = scene_on(ctx, mesh.V, mesh.tri, leaf, mesh.surface, mesh.normals)
    fresh = scene_on(ctx, B, mesh.tri, leaf, mesh.surface, mesh.normals)
    rb = nearest_rebuild.Rebuild(scene)
    # `last` is set BEFORE the rebuild: what every ray hits on the untouched scene
    last = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    first = scene.hits(nearest.Rays(_dev(o), _dev(d)), last=last)
    torch.cuda.synchronize()
    last0 = _host(last).view(np.uint32).copy()
    assert (_host(first.hit) != 0).mean() > 0.3 and (last0 != NO_PRIM).sum() > n // 4
    rb.update(_dev(B))
    got, want = both_entry_points(ctx, scene, o, d, last0), both_entry_points(ctx, fresh, o, d, last0)
    for k, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(x, y), (name, leaf, k)
    hit = got[0] != 0
    assert hit.mean() > 0.3 and not (got[NAMES.index("prim")].view(np.uint32)[hit] == last0[hit]).any()      # `last` survived
    rb.close(), scene.close(), fresh.close()


# ---- the cost --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree_stats(tmp_path_factory):
    """tests/native/nearest_tree_stats.cpp: the traversal's own source counting on a tree as read from a device"""
    d = tmp_path_factory.mktemp("tree_stats")
    exe = d / "nearest_tree_stats"
    p = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-ffp-contract=off", "-O2", str(ROOT / "tests" / "native" / "nearest_tree_stats.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def run(tree, V, tri, o, d):
        boxes, links, prims = tree
        M = d.shape[1]
        rec = np.empty((M, 8), np.uint32)
        rec[:, 0:3], rec[:, 3:6] = np.ascontiguousarray(o.T, F).view(np.uint32), np.ascontiguousarray(d.T, F).view(np.uint32)
        rec[:, 6], rec[:, 7] = np.full(M, np.inf, F).view(np.uint32), NO_PRIM
        path = tmp_path_factory.mktemp("rays") / "in.bin"
        with open(path, "wb") as f:
            f.write(np.array([V.shape[0], tri.shape[0], links.shape[0], M], np.int64).tobytes())
            f.write(np.ascontiguousarray(V, F).tobytes() + np.ascontiguousarray(tri, np.uint32).tobytes())
            f.write(np.ascontiguousarray(links, np.uint32).tobytes() + np.ascontiguousarray(prims, np.uint32).tobytes())
            f.write(np.ascontiguousarray(boxes, F).tobytes() + rec.tobytes())
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return json.loads(r.stdout)
    return run


@pytest.mark.parametrize("name", ["sphere", "grid"])
def test_the_cost_is_a_fresh_scenes_and_below_the_refits(ctx, tree_stats, name):
    """nodes and triangles a ray on the rebuilt tree == on the fresh tree == what nearest.host_stats counts on the builder's own
    tree, exactly; and fewer than on the tree that was only refit -- that tree comes from nearest_refit alone"""
    from rlshaders_amd import nearest, nearest_rebuild, nearest_refit
    mesh = twist_meshes()[name]
    B = twisted(mesh.V, 2.0)
    o, d = stream(mesh, B, 7)
    leaf = 4
    s1, s2 = scene_on(ctx, mesh.V, mesh.tri, leaf), scene_on(ctx, mesh.V, mesh.tri, leaf)
    refit, rb = nearest_refit.Refit(s1), nearest_rebuild.Rebuild(s2)
    refit.update(_dev(B))
    rb.update(_dev(B))
    c_refit = tree_stats(refit.read_tree(), B, mesh.tri, o, d)
    c_rebuilt = tree_stats(rb.read_tree(), B, mesh.tri, o, d)
    c_fresh = tree_stats(fresh_tree(ctx, B, mesh.tri, leaf), B, mesh.tri, o, d)
    own = nearest.host_stats(B, mesh.tri, o, d, leaf_size=leaf)
    print(name, "refit", c_refit, "rebuilt", c_rebuilt, "fresh", c_fresh)
    assert c_rebuilt == c_fresh
    assert (c_fresh["nodes"], c_fresh["triangles"], c_fresh["hits"], c_fresh["max_stack"]) == \
        (own["nodes"], own["triangles"], own["hits"], own["max_stack"])
    assert c_refit["results"] == c_fresh["results"] and c_refit["hits"] == c_fresh["hits"] > d.shape[1] // 4
    assert c_rebuilt["nodes"] < c_refit["nodes"] and c_rebuilt["triangles"] < c_refit["triangles"]
    refit.close(), rb.close(), s1.close(), s2.close()


# ---- hostile vertices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [1, 4])
def test_hostile_vertices_park_triangles(ctx, leaf):
    """NaN and infinities in a quarter of the vertices: *parked is exact, the tree is the builder's on the mesh whose parked
    triangles stand at the origin, no query hits a parked triangle, and an update with clean vertices gives the fresh tree"""
    from rlshaders_amd import nearest_rebuild
    nt = 1000
    A, B, tri = hostile_pair(nt)
    gone = parked_of(B, tri)
    a = U.soup(nt, seed=5)
    rest = without(U.Mesh(A, tri, surface=a.surface), B, gone)
    scene = scene_on(ctx, A, tri, leaf, a.surface)
    rb = nearest_rebuild.Rebuild(scene)
    parked = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert rb.update(_dev(B), parked=parked) is parked
    assert int(parked.item()) == int(gone.sum()) and 0 < gone.sum() < nt
    got = rb.read_tree()
    want = fresh_tree(ctx, rest.V, rest.tri, leaf)
    assert np.isfinite(got[0]).all() and same_tree(got, want) is None, same_tree(got, want)
    rng = np.random.default_rng(3)
    clean = np.where(np.isfinite(B), B, F(0))
    o1, d1 = U.rays_at_targets(rng, U.interior_targets(rng, U.Mesh(clean, tri[gone]), 128, margin=0.05), spread=2.0)
    o2, d2 = U.rays_at_targets(rng, U.interior_targets(rng, U.Mesh(clean, tri[~gone]), 128, margin=0.0), spread=2.0)
    o3, d3 = U.rays_at_targets(rng, np.zeros((32, 3)), spread=2.0)
    o, d = np.concatenate([o1, o2, o3], 1), np.concatenate([d1, d2, d3], 1)
    fresh = scene_on(ctx, rest.V, rest.tri, leaf, rest.surface)
    none = np.full(d.shape[1], NO_PRIM, np.uint32)
    x, y = both_entry_points(ctx, scene, o, d, none), both_entry_points(ctx, fresh, o, d, none)
    for k, (p, q) in enumerate(zip(x, y)):
        assert np.array_equal(p, q), (leaf, k)
    hit = x[0] != 0
    assert hit.mean() > 0.3 and not np.isin(x[NAMES.index("prim")].view(np.uint32)[hit], np.flatnonzero(gone)).any()
    rb.update(_dev(A), parked=parked)
    assert int(parked.item()) == 0 and same_tree(rb.read_tree(), fresh_tree(ctx, A, tri, leaf)) is None
    rb.close(), scene.close(), fresh.close()


# ---- interplay -------------------------------------------------------------------------------------------------------------------------
def test_a_refit_made_before_a_rebuild_updates_after_it(ctx):
    from rlshaders_amd import nearest_rebuild, nearest_refit
    mesh = twist_meshes()["sphere"]
    B, Cv = twisted(mesh.V, 2.0), twisted(mesh.V, 2.3)
    leaf = 4
    scene = scene_on(ctx, mesh.V, mesh.tri, leaf, mesh.surface, mesh.normals)
    refit = nearest_refit.Refit(scene)                               # made BEFORE the rebuild: its level lists come from the links alone
    rb = nearest_rebuild.Rebuild(scene)
    original = rb.read_tree()
    rb.update(_dev(B))
    once = rb.read_tree()
    rb.update(_dev(B))                                               # twice in a row: the same tree
    assert same_tree(rb.read_tree(), once) is None and np.array_equal(rb.read_tree()[0].view(np.uint32), once[0].view(np.uint32))
    refit.update(_dev(Cv))                                           # the rebuilt tree's links and order, C's boxes
    boxes, links, prims = refit.read_tree()
    assert np.array_equal(links, once[1]) and np.array_equal(prims, once[2])
    # the boxes a fresh scene on C holds for THIS order: the union below every node, which is what that scene's builder folds
    from nearest_refit_util import union_np
    assert np.array_equal(boxes, union_np(boxes, links, prims, Cv, mesh.tri))
    o, d = stream(mesh, Cv, 9)
    none = np.full(d.shape[1], NO_PRIM, np.uint32)
    fresh = scene_on(ctx, Cv, mesh.tri, leaf, mesh.surface, mesh.normals)
    for k, (x, y) in enumerate(zip(both_entry_points(ctx, scene, o, d, none), both_entry_points(ctx, fresh, o, d, none))):
        assert np.array_equal(x, y), k
    rb.update(_dev(mesh.V))                                          # back: the original tree
    assert same_tree(rb.read_tree(), original) is None
    assert rb.info()["updates"] == 3 and refit.info()["updates"] == 1
    refit.close(), rb.close(), scene.close(), fresh.close()


# ---- a graph, a second stream ----------------------------------------------------------------------------------------------------------
def test_update_in_a_graph_and_on_a_second_stream(ctx):
    """update recorded once and replayed over a vertex buffer whose contents change: each frame's fresh tree; the update run
    on a second stream's context gives the same bytes"""
    from rlshaders_amd import nearest_rebuild
    nt, leaf = 4099, 4
    A, B, tri = PAIRS["random"](nt)
    Cv = twisted(B, 2.0)
    scene = scene_on(ctx, A, tri, leaf)
    side = torch.cuda.Stream()
    gctx = R.Context(0)
    gctx.use_stream(side)
    try:
        rb = nearest_rebuild.Rebuild(scene)
        verts = _dev(A)
        parked = torch.zeros(1, dtype=torch.int64, device="cuda")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rb.update(verts, parked=parked, ctx=gctx)
        torch.cuda.synchronize()
        for V in (B, Cv, B):
            verts.copy_(_dev(V))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert same_tree(rb.read_tree(), fresh_tree(ctx, V, tri, leaf)) is None
        assert int(parked.item()) == 0 and rb.info()["updates"] == 1          # a replay is not a call
        replayed = rb.read_tree()
        rb.update(_dev(Cv), ctx=gctx)                                # the second stream's context, no graph
        on_side = rb.read_tree(ctx=gctx)
        rb.update(_dev(B), ctx=gctx)
        on_side_b = rb.read_tree(ctx=gctx)
        assert same_tree(on_side, fresh_tree(ctx, Cv, tri, leaf)) is None
        for x, y in zip(on_side_b, replayed):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        del graph
        rb.close()
    finally:
        gctx.close()
        scene.close()
