"""-m gpu: rls_nearest_any_hits / rls_nearest_any_walk_hits / rls_nearest_any_opaque (librls_nearest_any.so,
rlshaders_amd/nearest_any.py) equal the numpy statement (tests/nearest_any_util.py, any_np) bit for bit in every plane -- on the
empty scene, the icosphere, the quad grid, the soup and the rules' mesh with its rule streams and the hostile rays; at ray counts
about the tile; for every leaf size; without a flag table, with every flag set and with mixed flags under surfaces past the
table; with a device count below the rays, 0 and negative; with via; with a permuted ray plane indexing visibility, reach and
last; with base absent, given and aliasing visibility; at t == m and at reaches of 0, negative and NaN; on the deep grid with
its stack-filling stream (the expected states from the host-check program's brute force); on a scene moved by the refit and one
rebuilt on the device; recorded into a graph and replayed after the device count changed.  Every plane lives inside a
sentinel-filled buffer: entries at and past the count, and ids no entry names, are untouched, and `last` is never written."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_any_util as A
import nearest_util as U
from nearest_any_util import BLOCKED, CLEAR, VEILED, any_np
from nearest_util import F, NO_PRIM
from test_gpu_nearest import SENTINEL, Guarded, _dev, _host, _ids, mesh_of, mixed_rays

pytestmark = pytest.mark.gpu

COUNTS = [1, 255, 256, 257, 1000]
SENT32 = np.uint32(0xA5A5A5A5)
TABLES = {"none": None, "all": np.ones(4, np.uint8), "mixed": np.array([1, 0, 0, 1], np.uint8)}
SPECIAL = np.array([1.0, -0.0, 0.0, np.inf, -np.inf, np.nan, 0.25, -3.0, 1e-45, 0.5], F)


@pytest.fixture(scope="module")
def ctx():
    from rlshaders_amd import nearest_any
    nearest_any.load()                                               # (a missing library is an error, not a build)
    c = R.Context(0)
    yield c
    c.close()


def grid6():
    """the quad grid with surfaces 0 .. 5: two past a table of 4"""
    if "grid6" not in _cache:
        _cache["grid6"] = U.quad_grid(33, surfaces=6)
    return _cache["grid6"]


_cache = {}


def any_scene(ctx, name, leaf=0):
    """a scene of this module's context (test_gpu_nearest.scene_of caches scenes of a context that module closes)"""
    from rlshaders_amd import nearest
    key = ("scene", name, leaf)
    if key not in _cache:
        m = any_mesh(name)
        _cache[key] = nearest.Scene(ctx, m.V, m.tri, surface=m.surface, normals=m.normals, leaf_size=leaf)
    return _cache[key]


def any_mesh(name):
    return grid6() if name == "grid6" else mesh_of(name)


def bits(t):
    a = _host(t)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def run(ctx, scene, mesh, o, d, m=None, skip=None, flags=None, base=None, alias=False, rays=None, count=None, via=None, table=None,
        ids=None, width=None, planes=True, listed=None, active=None, use_ctx=None):
    """One guarded query and its check against any_np.  skip: the `last` plane by ray id, of `width` entries; ids: the ray plane;
    base: float32 [3, width]; alias: base IS the visibility tensor.  listed: the query goes through rls_nearest_any_walk_hits
    over a list of the rays (count required).  -> the statement's result over the traced entries, and the state tensor."""
    from rlshaders_amd import nearest, nearest_any
    n = d.shape[1] if rays is None else rays
    width = n if width is None else width
    alloc = Guarded()
    state = alloc((max(n, 1),), torch.uint8)
    vis = alloc((3, width), torch.float32) if planes else None
    reach = alloc((width,), torch.float32) if planes else None
    last = None
    if skip is not None:
        last = alloc((width,), torch.int32)
        last.copy_(_ids(skip))
    base_t = None
    if base is not None:
        if alias:
            vis.copy_(_dev(base))
            base_t = vis
        else:
            base_t = alloc((3, width), torch.float32)
            base_t.copy_(_dev(base))
    vis0 = None if vis is None else bits(vis).copy()
    cnt = None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda")
    fl = None if flags is None else _dev(flags)
    if listed:
        lst = SimpleNamespace(count=cnt, ray=_ids(ids), origin=_dev(o), dir=_dev(d), maxdist=_dev(m),
                              trials=torch.zeros(n, dtype=torch.uint8, device="cuda"))
        nearest_any.hits(scene, lst, active=active, opaque=fl, base=base_t, last=last, state=state,
                         visibility=vis if planes else False, reach=reach if planes else False, ctx=ctx if use_ctx is None else use_ctx)
        bound = n if active is None else active
    else:
        r = nearest.Rays(_dev(o if table is None else table), _dev(d), None if m is None else _dev(m),
                         via=None if via is None else _ids(via), ray=None if ids is None else _ids(ids), count=cnt, rays=n)
        nearest_any.hits(scene, r, opaque=fl, base=base_t, last=last, state=state, visibility=vis if planes else False,
                         reach=reach if planes else False, ctx=ctx if use_ctx is None else use_ctx)
        bound = n
    torch.cuda.synchronize()
    alloc.check()
    traced = bound if count is None else min(bound, max(count, 0))
    ray = np.arange(traced, dtype=np.int64) if ids is None else np.asarray(ids[:traced]).astype(np.int64)
    per_entry = None if skip is None else np.asarray(skip)[ray]
    want = any_np(mesh, o[:, :traced], d[:, :traced], None if m is None else m[:traced], per_entry, flags=flags,
                  base=None if base is None else base, ray=ray, ids=width)
    check(state, vis, reach, last, want, traced, vis0, skip)
    return want, state


def check(state, vis, reach, last, want, traced, vis0, skip):
    got = _host(state)
    assert np.array_equal(got[:traced], want.state), np.flatnonzero(got[:traced] != want.state)[:8]
    assert (got[traced:] == SENTINEL).all()                          # at and past the count
    if vis is not None:
        exp = vis0.copy()                                            # ids no traced entry names keep what they held
        exp[:, want.written] = A.bits(want.visibility)[:, want.written]
        assert np.array_equal(bits(vis), exp), np.argwhere(bits(vis) != exp)[:4]
        exp = np.full(want.reach.shape, SENT32)
        exp[want.written] = A.bits(want.reach)[want.written]
        assert np.array_equal(bits(reach), exp)
    if last is not None:
        assert np.array_equal(_host(last).view(np.uint32), np.asarray(skip).astype(np.uint32))     # read, never written


def base_of(rng, width):
    return SPECIAL[rng.integers(0, SPECIAL.size, (3, width))]


@pytest.fixture(scope="module")
def sphere_stream():
    return mixed_rays(mesh_of("icosphere"), COUNTS[-1], 21)


@pytest.mark.parametrize("n", COUNTS)
def test_ray_counts(ctx, sphere_stream, n):
    o, d, m, skip = sphere_stream
    want, _ = run(ctx, any_scene(ctx, "icosphere"), mesh_of("icosphere"), o[:, :n], d[:, :n], m[:n], skip[:n],
                  base=base_of(np.random.default_rng(n), n))
    if n == COUNTS[-1]:
        assert 0.3 < (want.state == BLOCKED).mean() < 0.95 and (want.state == CLEAR).sum() > 50


@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("name", ["empty", "icosphere", "grid6", "soup", "rules"])
def test_scenes_tables_hostile_rays_and_via(ctx, name, table):
    mesh = any_mesh(name)
    flags = TABLES[table]
    o, d, m, skip = mixed_rays(mesh, 300, 5)
    ho, hd, hm, hs = U.hostile_rays(mesh)
    o, d, m, skip = np.concatenate([o, ho], 1), np.concatenate([d, hd], 1), np.concatenate([m, hm]), np.concatenate([skip, hs])
    n = d.shape[1]
    scene = any_scene(ctx, name)
    want, _ = run(ctx, scene, mesh, o, d, m, skip, flags=flags)
    if mesh.nt:
        assert (want.state != CLEAR).sum() > 10
    if table == "mixed" and name in ("grid6", "soup"):
        # (the soup's surfaces run to 299 and nearly all read the table's last entry: its veiled rays are too few to ask for)
        assert (want.state == BLOCKED).any() and ((want.state == VEILED).any() or name == "soup")
        assert (mesh.surface >= 4).any()                             # surfaces past the table: they read its last entry
    if table != "mixed":
        assert not (want.state == VEILED).any()
    # via: the origins in a table of another order; no maxdist: +inf; no planes but state
    rng = np.random.default_rng(9)
    perm = rng.permutation(n)
    origins = np.empty_like(o)
    origins[:, perm] = o
    run(ctx, scene, mesh, o, d, None, skip, flags=flags, via=perm, table=origins, planes=False)


@pytest.mark.parametrize("name", sorted(U.rule_streams()))
def test_rule_streams(ctx, name):
    o, d, m, skip = U.rule_streams()[name]
    mesh = mesh_of("rules")
    for leaf in (1, 4):
        for flags in (None, np.array([1, 0, 0, 0], np.uint8), np.array([0, 0, 1, 0, 1, 1, 1, 1, 1, 0], np.uint8)):
            run(ctx, any_scene(ctx, "rules", leaf), mesh, o, d, m, skip, flags=flags)


def test_a_triangle_at_exactly_the_reach_and_hostile_reaches(ctx):
    mesh = mesh_of("icosphere")
    rng = np.random.default_rng(31)
    o, d = U.rays_at_targets(rng, U.interior_targets(rng, mesh, 256), spread=2.0)
    h = U.nearest_np(mesh, o, d)
    assert h.hit.all()
    scene = any_scene(ctx, "icosphere")
    at, _ = run(ctx, scene, mesh, o, d, h.t)                         # t == m: a candidate
    assert (at.state == BLOCKED).all()
    below, _ = run(ctx, scene, mesh, o, d, np.nextafter(h.t, F(0)))
    assert (below.state == CLEAR).all()
    for mm in (0.0, -0.0, -1.0, np.nan, -np.inf):
        none, _ = run(ctx, scene, mesh, o, d, np.full(256, mm, F), flags=np.array([0], np.uint8))
        assert (none.state == CLEAR).all()
    veiled, _ = run(ctx, scene, mesh, o, d, h.t, flags=np.array([0], np.uint8))
    assert (veiled.state == VEILED).all() and np.array_equal(A.bits(veiled.reach), A.bits(h.t))


@pytest.mark.parametrize("count", [-3, 0, 100, 256, 300, 301, 5000])
def test_device_count(ctx, sphere_stream, count):
    o, d, m, skip = sphere_stream
    n = 300
    run(ctx, any_scene(ctx, "icosphere"), mesh_of("icosphere"), o[:, :n], d[:, :n], m[:n], skip[:n], count=count,
        flags=TABLES["mixed"], base=base_of(np.random.default_rng(3), n))


@pytest.mark.parametrize("alias", [False, True])
def test_a_permuted_ray_plane_and_base_aliasing_visibility(ctx, alias):
    mesh = mesh_of("soup")
    o, d, m, _ = mixed_rays(mesh, 300, 13)
    rng = np.random.default_rng(17)
    ids = rng.permutation(400)[:300]                                 # ids past the entries, 100 of them unused
    last0 = rng.integers(0, mesh.nt, 400).astype(np.uint32)
    first = U.nearest_np(mesh, o, d, m)
    last0[ids] = np.where((first.hit != 0) & (rng.random(300) < 0.5), first.prim, last0[ids])
    last0[rng.random(400) < 0.3] = NO_PRIM
    flags = np.random.default_rng(2).integers(0, 2, 300).astype(np.uint8)
    want, _ = run(ctx, any_scene(ctx, "soup"), mesh, o, d, m, last0, flags=flags, base=base_of(rng, 400), alias=alias, ids=ids, width=400)
    plain = any_np(mesh, o, d, m, flags=flags)
    assert not np.array_equal(want.state, plain.state)               # the skips changed something
    assert (want.state == BLOCKED).sum() > 20 and (want.state == VEILED).sum() > 20


def test_leaf_sizes_give_the_same_bytes(ctx):
    mesh = mesh_of("soup")
    o, d, m, skip = mixed_rays(mesh, 600, 23)
    flags = np.random.default_rng(4).integers(0, 2, 300).astype(np.uint8)
    got = []
    for leaf in (1, 4, 8):
        scene = any_scene(ctx, "soup", leaf)
        assert scene.leaf_size == leaf
        _, state = run(ctx, scene, mesh, o, d, m, skip, flags=flags)
        got.append(_host(state).copy())
    assert all(np.array_equal(got[0], g) for g in got[1:])


def test_exact_and_fast_contexts_give_the_same_bytes(ctx, sphere_stream):
    o, d, m, skip = sphere_stream
    fast = R.Context(0)
    fast.set_math_mode(True)
    try:
        run(ctx, any_scene(ctx, "icosphere"), mesh_of("icosphere"), o, d, m, skip, use_ctx=fast)
    finally:
        fast.close()


def test_walk_list_entry_point(ctx, sphere_stream):
    """rls_nearest_any_walk_hits over a list as the walks hold it: state by entry, the other planes by the list's ray plane"""
    o, d, m, skip = sphere_stream
    cap, count = 300, 270
    rng = np.random.default_rng(29)
    ids = np.sort(rng.permutation(500)[:cap])                        # ascending queue rays, as a walk lists them
    last0 = np.full(500, NO_PRIM, np.uint32)
    last0[ids] = skip[:cap]
    mesh = mesh_of("icosphere")
    for active in (None, cap, 200):
        run(ctx, any_scene(ctx, "icosphere"), mesh, o[:, :cap], d[:, :cap], m[:cap], last0, flags=np.array([0, 1], np.uint8),
            base=base_of(rng, 500), alias=active is None, ids=ids, width=500, count=count, listed=True, active=active)


def test_opaque_flags_of_an_opacity_table(ctx):
    from rlshaders_amd import nearest_any
    one = F(1)
    rng = np.random.default_rng(6)
    t = rng.choice(np.array([1.0, 1.0, 1.0, 0.5, np.nan, np.inf, 0.0, -1.0, np.nextafter(one, F(0)), np.nextafter(one, F(2))], F), (3, 777))
    t[:, :3] = 1.0
    alloc = Guarded()
    out = alloc((777,), torch.uint8)
    flags = nearest_any.opaque_flags(ctx, _dev(t), out=out)
    torch.cuda.synchronize()
    alloc.check()
    want = A.flags_np(t)
    assert flags is out and np.array_equal(_host(flags), want) and 3 <= want.sum() < 200
    assert nearest_any.opaque_flags(ctx, torch.zeros(3, 0, device="cuda")).numel() == 0


def test_the_deep_grid_and_its_stack_filling_stream(ctx, tmp_path):
    """2^21 + 20 triangles, 23 levels at leaf 1: the corner rays fill the 22 stack entries a lane has use for.  The mesh is too
    large for any_np's loop: the expected states are the host-check program's brute force over the same statement."""
    import nearest_any_host_util as H
    from rlshaders_amd import nearest, nearest_any
    mesh = U.deep_grid()
    o, d, m, skip, info = U.deep_stream(mesh)
    flags = np.array([1, 1, 0, 1, 1, 0], np.uint8)                   # grid surface 2 and the extra triangles above translucent
    r = H.run(H.build(tmp_path), H.write_mesh(tmp_path / "deep.bin", mesh, flags), o, d, m, skip, leaf=1)
    assert r.depth == 23 and r.max_stack == 22 and (r.state == BLOCKED).sum() > 100 and (r.state == VEILED).sum() > 20
    n = d.shape[1]
    for leaf in (1, 8):
        scene = nearest.Scene(ctx, mesh.V, mesh.tri, surface=mesh.surface, leaf_size=leaf)
        alloc = Guarded()
        state, reach = alloc((n,), torch.uint8), alloc((n,), torch.float32)
        nearest_any.hits(scene, nearest.Rays(_dev(o), _dev(d), _dev(m)), opaque=_dev(flags), last=_ids(skip), state=state,
                         visibility=False, reach=reach)
        torch.cuda.synchronize()
        alloc.check()
        assert np.array_equal(_host(state), r.state), (leaf, np.flatnonzero(_host(state) != r.state)[:8])
        assert np.array_equal(bits(reach), A.bits(np.where(r.state == VEILED, m, F(0)).astype(F)))
        scene.close()


@pytest.mark.parametrize("how", ["refit", "rebuild"])
def test_a_moved_scene(ctx, how):
    """after a refit / a rebuild on the device the query returns any_np on the moved vertices"""
    from rlshaders_amd import nearest, nearest_rebuild, nearest_refit
    mesh = U.icosphere(2)
    rng = np.random.default_rng(37)
    scene = nearest.Scene(ctx, mesh.V, mesh.tri, surface=(np.arange(mesh.nt) % 6).astype(np.uint32), normals=mesh.normals)
    mover = (nearest_refit.Refit if how == "refit" else nearest_rebuild.Rebuild)(scene)
    V2 = (mesh.V * F([1.5, 0.7, 1.0]) + F([0.3, -0.2, 0.1]) + rng.uniform(-0.02, 0.02, mesh.V.shape)).astype(F)
    mover.update(_dev(V2))
    moved = U.Mesh(V2, mesh.tri, surface=(np.arange(mesh.nt) % 6).astype(np.uint32))
    o, d, m, skip = mixed_rays(moved, 600, 41)
    want, _ = run(ctx, scene, moved, o, d, m, skip, flags=TABLES["mixed"])
    still = any_np(U.Mesh(mesh.V, mesh.tri, surface=moved.surface), o, d, m, skip, flags=TABLES["mixed"])
    assert not np.array_equal(want.state, still.state)               # the move changed something
    assert (want.state == BLOCKED).any() and (want.state == VEILED).any()
    mover.close()
    scene.close()


def test_one_graph_replay_after_the_count_changed(ctx, sphere_stream):
    from rlshaders_amd import nearest, nearest_any
    o, d, m, skip = sphere_stream
    n = 300
    mesh, scene = mesh_of("icosphere"), any_scene(ctx, "icosphere")
    flags, base = np.array([0, 1], np.uint8), base_of(np.random.default_rng(8), n)
    side = torch.cuda.Stream()                                       # (the NULL stream cannot be captured)
    gctx = R.Context(0)
    gctx.use_stream(side)
    try:
        cnt = torch.tensor([n], dtype=torch.int64, device="cuda")
        rays = nearest.Rays(_dev(o[:, :n]), _dev(d[:, :n]), _dev(m[:n]), count=cnt)
        last, fl, base_t = _ids(skip[:n]), _dev(flags), _dev(base)
        alloc = Guarded()
        state, vis, reach = alloc((n,), torch.uint8), alloc((3, n), torch.float32), alloc((n,), torch.float32)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            nearest_any.hits(scene, rays, opaque=fl, base=base_t, last=last, state=state, visibility=vis, reach=reach, ctx=gctx)
        torch.cuda.synchronize()
        for count in (n, 133):
            for buf, _ in alloc.outer:
                buf.fill_(SENTINEL)
            cnt.fill_(count)
            vis0 = bits(vis).copy()
            graph.replay()
            torch.cuda.synchronize()
            alloc.check()
            want = any_np(mesh, o[:, :count], d[:, :count], m[:count], skip[:count], flags=flags, base=base, ids=n)
            check(state, vis, reach, last, want, count, vis0, skip[:n])
            direct, _ = run(ctx, scene, mesh, o[:, :n], d[:, :n], m[:n], skip[:n], flags=flags, base=base, count=count)
            assert np.array_equal(direct.state, want.state)
        del graph
    finally:
        gctx.close()


def test_refusals_on_the_device_path(ctx):
    from rlshaders_amd import nearest, nearest_any
    s = any_scene(ctx, "icosphere")
    z = torch.zeros(3, 8, device="cuda")
    with pytest.raises(ValueError, match="last: 7 entries for 8 rays"):
        nearest_any.hits(s, nearest.Rays(z, z), last=torch.full((7,), -1, dtype=torch.int32, device="cuda"))
    with pytest.raises(Exception, match="rls_nearest_any_hits: found.base or found.visibility is partly NULL"):
        f = nearest_any.NearestAnyFound_()
        f.state, f.visibility = z.data_ptr(), R._capi.Rgb(z.data_ptr(), None, z.data_ptr())
        R._capi.check(nearest_any.load().rls_nearest_any_hits(ctx.handle, s.handle, nearest.Rays(z, z).struct(), f))
