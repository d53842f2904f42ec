"""-m gpu: rls_nearest_refit_update (librls_nearest_refit.so, rlshaders_amd/nearest_refit.py) moves a scene to a new mesh, and
every query afterwards equals the numpy statement (tests/nearest_util.py, nearest_np) on the moved mesh AND a fresh nearest.Scene
on the moved vertices, bit for bit in every found plane (hit, t, P, N, Ns, T, wo, prim, surface, u, v, bin); an update back
restores the untouched scene's bytes.  Moved meshes at three leaf sizes; trees of one node, of two levels of leaves, of a level
list that crosses a workgroup; the read tree against a numpy bottom-up union; parked triangles; normals replaced, kept and
refused; `last` across an update; both walks on the refit scene; an update and a query recorded into one graph and replayed
after the vertex buffer changed."""
import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_util as U
from nearest_util import F, NO_PRIM
from nearest_refit_util import COUNT_MASK, jittered, moved, squashed, union_np, without
from test_gpu_nearest import SCALAR, VEC, _bytes, _dev, _host, _ids, check_found, query

pytestmark = pytest.mark.gpu

BINS = np.array([3, 0, 7, 1, 2], np.uint8)
NAMES = ("hit", "t") + VEC + SCALAR + ("bin",)


@pytest.fixture(scope="module")
def ctx():
    from rlshaders_amd import nearest, nearest_refit
    nearest.load(), nearest_refit.load()                             # (a missing library is an error, not a build)
    c = R.Context(0)
    yield c
    c.close()


def device_scene(ctx, mesh, leaf=0, V=None):
    from rlshaders_amd import nearest
    return nearest.Scene(ctx, mesh.V if V is None else V, mesh.tri, surface=mesh.surface, normals=mesh.normals, leaf_size=leaf)


def rays_for(mesh_a, mesh_b, M, seed):
    """rays aimed at points of B's triangles and of A's, from about them, and the hostile rays"""
    rng = np.random.default_rng(seed)
    k = M * 2 // 3
    ob, db = U.rays_at_targets(rng, U.interior_targets(rng, mesh_b, k, margin=0.0), spread=2.0)
    oa, da = U.rays_at_targets(rng, U.interior_targets(rng, mesh_a, M - k, margin=0.0), spread=2.0)
    ho, hd, hm, hs = U.hostile_rays(mesh_b, seed=seed)
    o, d = np.concatenate([ob, oa, ho], 1), np.concatenate([db, da, hd], 1)
    m = np.concatenate([np.full(M, np.inf, F), hm])
    skip = np.concatenate([np.full(M, NO_PRIM, np.uint32), hs])
    return o, d, m, skip


def found_bytes(ctx, scene, o, d, m, skip):
    f, last, _ = query(ctx, scene, o, d, m, skip, bin_table=BINS)
    return f, _bytes(f, NAMES) + [_host(last)]


def same(a, b, what):
    for name, x, y in zip(NAMES + ("last",), a, b):
        assert np.array_equal(x, y), (what, name)


# ---- moved meshes ----------------------------------------------------------------------------------------------------------------------
MESHES = dict(icosphere=lambda: U.icosphere(3), grid=lambda: U.quad_grid(33), soup=lambda: U.soup(1025))
_cache = {}


def pair_of(name):
    """(A, B, the rays, the statement on A, the statement on B), computed once"""
    if name not in _cache:
        a = MESHES[name]()
        b = moved(a, squashed(a, 11))
        o, d, m, skip = rays_for(a, b, 448, 17)
        _cache[name] = (a, b, (o, d, m, skip), U.nearest_np(a, o, d, m, skip), U.nearest_np(b, o, d, m, skip))
    return _cache[name]


@pytest.mark.parametrize("leaf", [1, 4, 8])
@pytest.mark.parametrize("name", list(MESHES))
def test_moved_meshes(ctx, name, leaf):
    from rlshaders_amd import nearest_refit
    a, b, rays, ha, hb = pair_of(name)
    assert a.nt == {"icosphere": 1280, "grid": 2178, "soup": 1025}[name]
    n = rays[1].shape[1]
    # an update that does nothing cannot pass: the rays hit on B, and what they hit is not what they hit on A
    assert hb.hit.mean() >= 0.25, hb.hit.mean()
    differ = (ha.hit != hb.hit) | ((hb.hit != 0) & ((ha.prim != hb.prim) | (ha.t.view(np.uint32) != hb.t.view(np.uint32))))
    assert differ.mean() >= 0.25, differ.mean()
    scene = device_scene(ctx, a, leaf)
    refit = nearest_refit.Refit(scene)
    assert (refit.nv, refit.nt, refit.nodes, refit.levels) == (scene.nv, scene.nt, scene.nodes, scene.depth)
    f0, before = found_bytes(ctx, scene, *rays)
    check_found(f0, ha, n, (name, leaf, "the untouched scene"), bin_table=BINS)
    refit.update(_dev(b.V))
    f1, after = found_bytes(ctx, scene, *rays)
    check_found(f1, hb, n, (name, leaf, "refit to B"), bin_table=BINS)
    fresh = device_scene(ctx, b, leaf)
    _, rebuilt = found_bytes(ctx, fresh, *rays)
    same(after, rebuilt, (name, leaf, "a fresh scene on B"))
    refit.update(_dev(a.V))
    _, back = found_bytes(ctx, scene, *rays)
    same(back, before, (name, leaf, "back on A"))
    assert refit.info()["updates"] == 2
    refit.close(), fresh.close(), scene.close()


# ---- small trees -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt,leaf", [(0, 4), (1, 4), (1, 1), (5, 4), (9, 8), (2, 1), (5, 1), (6, 1), (7, 1), (9, 1), (257, 1), (600, 1)])
def test_small_trees(ctx, nt, leaf):
    """nt = 0 and 1: the root is a leaf (or absent); nt = leaf + 1: one split; nt = 5, 6, 7, 9 at leaf 1: leaves on two levels;
    nt = 257 at leaf 1: levels of 1, 2, 4 .. 256 and 2 nodes, none above one workgroup's 256, so the whole tree is the folded
    top and the single-workgroup launch meets a full level of 256 lanes with a level of 2 below it (the per-level kernel at
    such levels: test_gpu_nearest_refit_edges.py, test_both_launch_plans); nt = 600 at leaf 1: a level list of more than one
    workgroup's nodes"""
    from rlshaders_amd import nearest_refit
    s = U.soup(max(nt, 1), seed=100 + nt)
    a = U.Mesh(s.V, s.tri[:nt], surface=s.surface[:nt], normals=s.normals)
    b = moved(a, squashed(a, 3))
    scene = device_scene(ctx, a, leaf)
    refit = nearest_refit.Refit(scene)
    info = refit.info()
    assert info["levels"] == scene.depth and info["nodes"] == scene.nodes and (info["device_bytes"] > 0) == (nt > 0)
    boxes0, links0, prims0 = refit.read_tree()
    if nt:
        leaves = (links0[:, 1] & COUNT_MASK) != 0
        assert (links0[leaves, 1] & COUNT_MASK).sum() == nt and sorted(prims0) == list(range(nt))
    if nt in (5, 6, 7, 9) and leaf == 1:
        # leaves on two levels: a leaf node that is a child of the root's grandchildren's level and one a level deeper
        depth_of = {0: 1}
        for n in range(links0.shape[0]):
            if not links0[n, 1] & COUNT_MASK:
                depth_of[int(links0[n, 0])] = depth_of[int(links0[n, 0]) + 1] = depth_of[n] + 1
        assert len({depth_of[n] for n in np.flatnonzero(leaves)}) == 2
    if nt >= 257:
        assert refit.levels >= 10 and links0.shape[0] == 2 * nt - 1
    if nt:
        o, d, m, skip = rays_for(a, b, 96, nt)
    else:
        o, d = U.random_rays(np.random.default_rng(1), 64)
        m, skip = np.full(64, np.inf, F), np.full(64, NO_PRIM, np.uint32)
    parked = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    refit.update(_dev(b.V), parked=parked)
    f, _, _ = query(ctx, scene, o, d, m, skip)
    check_found(f, U.nearest_np(b, o, d, m, skip), d.shape[1], ("small", nt, leaf))
    assert int(parked.item()) == 0
    boxes, links, prims = refit.read_tree()
    assert np.array_equal(links, links0) and np.array_equal(prims, prims0)
    assert np.array_equal(boxes, union_np(boxes, links, prims, b.V, b.tri))
    refit.update(_dev(a.V))
    boxes, _, _ = refit.read_tree()
    assert np.array_equal(boxes, boxes0)
    refit.close(), scene.close()


# ---- shape and contracts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [1, 4])
def test_read_tree_is_the_bottom_up_union(ctx, leaf):
    from rlshaders_amd import nearest_refit
    a, b, _, _, _ = pair_of("grid")
    scene = device_scene(ctx, a, leaf)
    refit = nearest_refit.Refit(scene)
    boxes0, links0, prims0 = refit.read_tree()
    assert boxes0.shape == (scene.nodes, 6) and links0.shape == (scene.nodes, 2) and prims0.shape == (a.nt,)
    assert np.array_equal(boxes0, union_np(boxes0, links0, prims0, a.V, a.tri))          # the builder's boxes are that union too
    refit.update(_dev(b.V))
    boxes, links, prims = refit.read_tree()
    assert np.array_equal(links, links0) and np.array_equal(prims, prims0)
    assert np.array_equal(boxes, union_np(boxes, links, prims, b.V, b.tri)) and not np.array_equal(boxes, boxes0)
    refit.close(), scene.close()


def test_parked_triangles(ctx):
    """a NaN, a +inf and a -inf vertex: the triangles that use them are parked -- counted exactly, never hit -- and every
    ray sees the mesh without them"""
    from rlshaders_amd import nearest_refit
    a = U.icosphere(3)
    V = jittered(a, 5, 0.02)
    V[7, 1], V[100, 0], V[333, 2] = np.nan, np.inf, -np.inf
    gone = np.isin(a.tri, (7, 100, 333)).any(axis=1)
    assert 12 <= gone.sum() <= 18
    rest = without(a, V, gone)
    rng = np.random.default_rng(2)
    # aimed at where the parked triangles stood, at the others, and through the origin, where they stand now
    at = U.Mesh(jittered(a, 5, 0.02), a.tri[gone])
    o1, d1 = U.rays_at_targets(rng, U.interior_targets(rng, at, 200, margin=0.05), spread=2.0)
    o2, d2 = U.rays_at_targets(rng, U.interior_targets(rng, rest, 200, margin=0.0), spread=2.0)
    o3, d3 = U.rays_at_targets(rng, np.zeros((48, 3)), spread=2.0)
    o, d = np.concatenate([o1, o2, o3], 1), np.concatenate([d1, d2, d3], 1)
    h = U.nearest_np(rest, o, d)
    assert not np.isin(h.prim[h.hit != 0], np.flatnonzero(gone)).any() and h.hit.mean() > 0.5
    for leaf in (1, 4):
        scene = device_scene(ctx, a, leaf)
        refit = nearest_refit.Refit(scene)
        parked = torch.zeros(1, dtype=torch.int64, device="cuda")
        assert refit.update(_dev(V), parked=parked) is parked
        f, _, _ = query(ctx, scene, o, d)
        check_found(f, h, d.shape[1], ("parked", leaf))
        assert int(parked.item()) == int(gone.sum())
        boxes, links, prims = refit.read_tree()
        assert np.isfinite(boxes).all() and np.array_equal(boxes, union_np(boxes, links, prims, V, a.tri))
        refit.update(_dev(a.V), parked=parked)
        assert int(parked.item()) == 0
        refit.close(), scene.close()


def test_normals_replaced_kept_and_refused(ctx):
    from rlshaders_amd import nearest_refit
    a = U.icosphere(2)
    B = squashed(a, 4)
    rng = np.random.default_rng(8)
    other = rng.normal(size=a.normals.shape).astype(F)
    o, d, m, skip = rays_for(a, moved(a, B), 192, 6)
    scene = device_scene(ctx, a)
    refit = nearest_refit.Refit(scene)
    assert refit.info()["has_normals"]
    refit.update(_dev(B))                                            # kept
    f, _, _ = query(ctx, scene, o, d, m, skip)
    kept = U.nearest_np(moved(a, B), o, d, m, skip)
    check_found(f, kept, d.shape[1], "normals kept")
    refit.update(_dev(B), normals=_dev(other))                       # replaced
    f, _, _ = query(ctx, scene, o, d, m, skip)
    replaced = U.nearest_np(U.Mesh(B, a.tri, surface=a.surface, normals=other), o, d, m, skip)
    check_found(f, replaced, d.shape[1], "normals replaced")
    sel = replaced.hit != 0
    assert sel.sum() > 50 and (replaced.Ns[:, sel].view(np.uint32) != kept.Ns[:, sel].view(np.uint32)).any()
    refit.update(B, normals=a.normals)                               # host arrays are uploaded
    f, _, _ = query(ctx, scene, o, d, m, skip)
    check_found(f, kept, d.shape[1], "normals put back from the host")
    refit.close(), scene.close()
    bare = nearest_refit.Refit(device_scene(ctx, U.Mesh(a.V, a.tri)))
    assert not bare.info()["has_normals"]
    with pytest.raises(Exception, match="rls_nearest_refit_update: mesh.normals is set but the scene was made without normals"):
        bare.update(_dev(B), normals=_dev(other))
    with pytest.raises(ValueError, match="vertices"):
        bare.update(_dev(B[:-1]))
    assert bare.info()["updates"] == 0
    scene2 = bare.scene
    bare.close(), bare.close(), scene2.close()


def test_last_carried_across_an_update(ctx):
    """a ray standing on the triangle it hit before the update does not meet it again after it: triangle ids do not change"""
    from rlshaders_amd import nearest, nearest_refit
    a = U.icosphere(2)
    B = jittered(a, 9, 0.03)
    rng = np.random.default_rng(12)
    n = 256
    o, d = U.rays_at_targets(rng, U.interior_targets(rng, a, n), spread=2.0)
    scene = device_scene(ctx, a)
    refit = nearest_refit.Refit(scene)
    last = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    f1 = scene.hits(nearest.Rays(_dev(o), _dev(d)), last=last)
    h1 = U.nearest_np(a, o, d)
    assert h1.hit.all() and np.array_equal(_host(last).view(np.uint32), h1.prim)
    # the next segment starts ON the hit and goes on; on the moved mesh the old triangle is still about there
    o2 = h1.P.copy()
    refit.update(_dev(B))
    f2 = scene.hits(nearest.Rays(_dev(o2), _dev(d)), last=last)
    torch.cuda.synchronize()
    h2 = U.nearest_np(moved(a, B), o2, d, skip=h1.prim)
    free = U.nearest_np(moved(a, B), o2, d)
    assert ((free.hit != 0) & (free.prim == h1.prim)).sum() > 10      # without `last` many would hit where they stand
    assert np.array_equal(_host(f2.hit), h2.hit) and not ((h2.hit != 0) & (h2.prim == h1.prim)).any()
    sel = h2.hit != 0
    assert np.array_equal(_host(f2.prim).view(np.uint32)[sel], h2.prim[sel])
    assert np.array_equal(_host(f2.t).view(np.uint32)[sel], h2.t.view(np.uint32)[sel])
    assert np.array_equal(_host(last).view(np.uint32), np.where(sel, h2.prim, h1.prim))
    del f1
    refit.close(), scene.close()


# ---- composition -----------------------------------------------------------------------------------------------------------------------
def test_both_walks_on_the_refit_scene(ctx):
    from rlshaders_amd import nearest, nearest_refit, shadow_walk, trace, walk
    from test_walk_statement import SEED, setting
    walk.load(), shadow_walk.load()
    n, spp_n = 40, 2
    case, _ = setting("sphere", n)
    P = case["P"]
    s = R.SssSampler(ctx, _dev(case["N"]), _dev(case["T"]), _dev(case["albedo"]), _dev(case["dist"]), has_dPdu=True)
    q = trace.sss_probe_rays(s, _dev(P), spp_n, SEED)
    maxdist = _host(q.maxdist)
    centre = P.astype(np.float64).mean(axis=1)
    reach = float(np.median(maxdist[maxdist > 0]))
    radius = float(np.linalg.norm(P.astype(np.float64).T - centre, axis=1).max()) + 0.25 * reach
    b = U.icosphere(2, radius=radius, center=centre)
    a = U.icosphere(2, radius=3.0 * radius, center=centre + 1.0)     # the scene starts far off and is refit about the points
    scene, fresh = device_scene(ctx, a), device_scene(ctx, b)
    refit = nearest_refit.Refit(scene)
    refit.update(_dev(b.V))
    w, wf = walk.run(q, _dev(P), nearest.tracer(scene)), walk.run(q, _dev(P), nearest.tracer(fresh))
    assert w.active == 0 and int(w.hit_count.sum()) > n
    assert torch.equal(w.hit_count, wf.hit_count)
    live = np.arange(w.max_hits)[:, None] < _host(w.hit_count)[None, :]
    for x, y in ((w.hit_P, wf.hit_P), (w.hit_N, wf.hit_N)):
        assert np.array_equal(_host(x)[:, live].view(np.uint32), _host(y)[:, live].view(np.uint32))
    refit.close(), scene.close(), fresh.close()


@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_shadow_walk_on_the_refit_scene(ctx, gpu, oracle, node):
    """light-loop shadow rays under two tinted quads and an opaque sphere (tests/test_gpu_nearest_walks.py's scene), the scene
    made with everything somewhere else and refit there"""
    from rlshaders_amd import nearest, nearest_refit, shadow_walk, trace
    from test_gpu_nearest_walks import shadow_mesh
    from test_gpu_shadow_walk import SEED as LSEED, SPP_N, batch, surface_table
    trace.load(), shadow_walk.load()
    bt, lights = batch(trace, gpu, oracle, node)
    q = bt.emit(lights, SPP_N, LSEED)
    table = surface_table(trace, gpu)
    b = shadow_mesh()
    a = moved(b, squashed(b, 21) + F(0.7))
    scene, fresh = device_scene(gpu, a), device_scene(gpu, b)
    refit = nearest_refit.Refit(scene)
    refit.update(_dev(b.V), ctx=gpu)
    w = shadow_walk.run(q, bt.P, nearest.tracer(scene, opacity=table), max_steps=12)
    wf = shadow_walk.run(q, bt.P, nearest.tracer(fresh, opacity=table), max_steps=12)
    got, want = _host(w.visibility)[:, :q.count], _host(wf.visibility)[:, :q.count]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    black = (got.view(np.uint32) == 0).all(axis=0)
    assert black.any() and (got[:, ~black] > 0).all() and (got < 1).any()
    for x, y in zip(q.resolve(w.visibility), q.resolve(wf.visibility)):
        assert np.array_equal(_host(x).view(np.uint32), _host(y).view(np.uint32))
    refit.close(), scene.close(), fresh.close()


def test_update_and_query_in_one_graph(ctx):
    """update + hits recorded once; replayed after the vertex buffer's contents changed, the results follow the buffer"""
    from rlshaders_amd import nearest, nearest_refit
    a, b, (o, d, m, skip), _, _ = pair_of("icosphere")
    n = 256
    o, d, m = o[:, :n], d[:, :n], m[:n]
    scene = device_scene(ctx, a)
    side = torch.cuda.Stream()
    gctx = R.Context(0)
    gctx.use_stream(side)
    try:
        refit = nearest_refit.Refit(scene)
        verts = _dev(a.V)
        parked = torch.zeros(1, dtype=torch.int64, device="cuda")
        rays = nearest.Rays(_dev(o), _dev(d), _dev(m))
        f = nearest.Found(gctx, n)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            refit.update(verts, parked=parked, ctx=gctx)
            scene.hits(rays, found=f, ctx=gctx)
        torch.cuda.synchronize()
        for V, h in ((b.V, U.nearest_np(b, o, d, m)), (a.V, U.nearest_np(a, o, d, m)), (b.V, None)):
            verts.copy_(_dev(V))
            f.hit.fill_(9)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            if h is not None:
                hit = _host(f.hit)
                assert np.array_equal(hit, h.hit)
                sel = hit != 0
                for name in ("t",) + VEC + SCALAR:
                    got, want = _host(getattr(f, name)), getattr(h, name)
                    assert np.array_equal(np.ascontiguousarray(got[..., sel]).view(np.uint32),
                                          np.ascontiguousarray(want[..., sel]).view(np.uint32)), name
        assert int(parked.item()) == 0 and refit.info()["updates"] == 1      # a replay is not a call
        del graph
        refit.close()
    finally:
        gctx.close()
        scene.close()
