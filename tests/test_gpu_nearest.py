"""-m gpu: rls_nearest_hits / rls_nearest_walk_hits (librls_nearest.so, rlshaders_amd/nearest.py) equal the numpy statement
(tests/nearest_util.py, nearest_np) bit for bit in every written plane -- on an empty scene, a single triangle, the icosphere,
the quad grid and the 1025-triangle soup; at ray counts about the wavefront and the tile; on every hostile stream of the CPU test;
with via, maxdist, a device count, every optional plane absent and present, `last` through a permuted id plane; the same bytes for
every leaf size and under a FAST context; the bin plane as the numpy table lookup; one graph replay.  Every plane lives inside a
sentinel-filled buffer: entries past the count, and the planes of missed entries, are untouched."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_util as U
from nearest_util import F, NO_PRIM

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 512
VEC = ("P", "N", "Ns", "T", "wo")
SCALAR = ("prim", "surface", "u", "v")
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 3 * 256 + 5]


def _host(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ids(a):
    return _dev(np.asarray(a).astype(np.uint32).view(np.int32))


class Guarded:
    """an allocator: every tensor an inner view of a sentinel-filled buffer, itself sentinel-filled"""

    def __init__(self):
        self.outer = []

    def __call__(self, shape, dtype):
        size = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        inner = (size + 255) // 256 * 256
        buf = torch.full((GUARD + inner + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.outer.append((buf, size))
        return buf[GUARD:GUARD + size].view(dtype).view(shape)

    def check(self):
        for buf, size in self.outer:
            b = _host(buf)
            assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + size:] == SENTINEL).all(), size


@pytest.fixture(scope="module")
def ctx():
    from rlshaders_amd import nearest
    nearest.load()                                                   # (a missing library is an error, not a build)
    c = R.Context(0)
    yield c
    c.close()


MESHES = dict(empty=U.empty_mesh, single=U.single_triangle, icosphere=lambda: U.icosphere(2), grid=lambda: U.quad_grid(33),
              soup=lambda: U.soup(1025), rules=U.rules_mesh)
_cache = {}


def mesh_of(name):
    if name not in _cache:
        _cache[name] = MESHES[name]()
    return _cache[name]


def scene_of(ctx, name, leaf=0):
    from rlshaders_amd import nearest
    key = ("scene", name, leaf)
    if key not in _cache:
        m = mesh_of(name)
        _cache[key] = nearest.Scene(ctx, m.V, m.tri, surface=m.surface, normals=m.normals, leaf_size=leaf)
    return _cache[key]


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype.kind == "f":
        ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    else:
        ok = got.view(np.uint32) == want.view(np.uint32)
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:4].tolist(), got[~ok][:4], want[~ok][:4])


def untouched(t, cols, what):
    """the columns `cols` (a bool mask over the last axis) of tensor t hold the sentinel in every byte"""
    if t.numel() == 0:
        return
    b = _host(t.reshape(-1, t.shape[-1]).contiguous().view(torch.uint8)).reshape(-1, t.shape[-1], t.element_size())
    assert (b[:, cols] == SENTINEL).all(), what


def check_found(f, h, traced, what, bin_table=None, planes=VEC + SCALAR):
    """f: the device's Found over n entries of which `traced` were traced; h: the statement's Hits of (at least) those"""
    n = f.rays
    hit = _host(f.hit)
    assert np.array_equal(hit[:traced], h.hit[:traced]), (what, "hit", np.flatnonzero(hit[:traced] != h.hit[:traced])[:8])
    written = np.zeros(n, bool)
    written[:traced] = h.hit[:traced] != 0
    past = np.arange(n) >= traced
    untouched(f.hit, past, (what, "hit past the count"))
    for name in ("t",) + tuple(planes):
        t = getattr(f, name)
        want = getattr(h, name)
        got = _host(t)
        if name in ("prim", "surface"):
            got = got.view(np.uint32)
        same_bits(got[..., written], want[..., :n][..., written], (what, name))
        untouched(t, ~written, (what, name, "missed or past the count"))
    if bin_table is not None:
        want = np.where(h.hit[:traced] != 0, bin_table[np.minimum(h.surface[:traced].astype(np.int64), len(bin_table) - 1)], 255)
        assert np.array_equal(_host(f.bin)[:traced], want.astype(np.uint8)), (what, "bin")
        untouched(f.bin, past, (what, "bin past the count"))


def query(ctx, scene, o, d, m=None, skip=None, rays=None, count=None, via=None, table=None, planes=VEC + SCALAR, bin_table=None,
          ids=None, use_ctx=None):
    """one guarded query -> (Found, last or None, the allocator)"""
    from rlshaders_amd import nearest
    n = d.shape[1] if rays is None else rays
    alloc = Guarded()
    f = nearest.Found(ctx, n, planes=planes, bin=bin_table is not None, alloc=alloc)
    r = nearest.Rays(_dev(o if table is None else table), _dev(d), None if m is None else _dev(m),
                     via=None if via is None else _ids(via), ray=None if ids is None else _ids(ids),
                     count=None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda"), rays=n)
    last = None
    if skip is not None:
        last = alloc((len(skip),), torch.int32)
        last.copy_(_ids(skip))
    scene.hits(r, last=last, found=f, bin_of_surface=None if bin_table is None else _dev(bin_table), ctx=use_ctx)
    torch.cuda.synchronize()
    alloc.check()
    return f, last, alloc


def mixed_rays(mesh, M, seed):
    """random rays, half of them aimed at the mesh, with reaches about the scene's size and some skips"""
    rng = np.random.default_rng(seed)
    o, d = U.random_rays(rng, M)
    if mesh.nt:
        k = M // 2
        o[:, :k], d[:, :k] = U.rays_at_targets(rng, U.interior_targets(rng, mesh, k, margin=0.0), spread=2.0)
    m = rng.uniform(0.3, 3.0, M).astype(F)
    m[rng.random(M) < 0.3] = np.inf
    skip = np.full(M, NO_PRIM, np.uint32)
    if mesh.nt:
        first = U.nearest_np(mesh, o, d)
        pick = (rng.random(M) < 0.3) & (first.hit != 0)
        skip[pick] = first.prim[pick]
    return o, d, m, skip


def soup_stream():
    if "soup300" not in _cache:
        mesh = mesh_of("soup")
        o, d, m, skip = mixed_rays(mesh, 300, 13)
        _cache["soup300"] = (o, d, m, skip, U.nearest_np(mesh, o, d, m, skip))
    return _cache["soup300"]


@pytest.fixture(scope="module")
def sphere_stream():
    mesh = mesh_of("icosphere")
    o, d, m, skip = mixed_rays(mesh, COUNTS[-1], 21)
    return o, d, m, skip, U.nearest_np(mesh, o, d, m, skip)


@pytest.mark.parametrize("n", COUNTS)
def test_ray_counts(ctx, sphere_stream, n):
    o, d, m, skip, h = sphere_stream
    f, last, _ = query(ctx, scene_of(ctx, "icosphere"), o[:, :n], d[:, :n], m[:n], skip[:n])
    check_found(f, h, n, ("count", n))
    want = np.where(h.hit[:n] != 0, h.prim[:n], skip[:n])            # a hit writes prim, a miss leaves `last`
    assert np.array_equal(_host(last).view(np.uint32), want)
    if n == COUNTS[-1]:
        assert 0.3 < h.hit.mean() < 0.95 and (skip != NO_PRIM).sum() > 50


@pytest.mark.parametrize("name", ["empty", "single", "icosphere", "grid", "soup"])
def test_scenes_with_hostile_rays_via_and_no_maxdist(ctx, name):
    mesh = mesh_of(name)
    o, d, m, skip = mixed_rays(mesh, 300, 5)
    ho, hd, hm, hs = U.hostile_rays(mesh)
    o, d, m, skip = np.concatenate([o, ho], 1), np.concatenate([d, hd], 1), np.concatenate([m, hm]), np.concatenate([skip, hs])
    n = d.shape[1]
    scene = scene_of(ctx, name)
    assert scene.nt == mesh.nt and (scene.nodes == 0) == (mesh.nt == 0) and scene.depth - 1 <= U.STACK
    h = U.nearest_np(mesh, o, d, m, skip)
    f, _, _ = query(ctx, scene, o, d, m, skip)
    check_found(f, h, n, (name, "direct"))
    if mesh.nt:
        assert h.hit.any()
    # via: the origins in a table of another order, entry k starting at table[via[k]]; no maxdist: +inf
    rng = np.random.default_rng(9)
    perm = rng.permutation(n)
    table = np.empty_like(o)
    table[:, perm] = o
    h2 = U.nearest_np(mesh, o, d, None, skip)
    f2, _, _ = query(ctx, scene, o, d, None, skip, via=perm, table=table)
    check_found(f2, h2, n, (name, "via, no maxdist"))


@pytest.mark.parametrize("name", sorted(U.rule_streams()))
def test_rule_streams(ctx, name):
    o, d, m, skip = U.rule_streams()[name]
    mesh = mesh_of("rules")
    h = U.nearest_np(mesh, o, d, m, skip)
    for leaf in (1, 4):
        f, last, _ = query(ctx, scene_of(ctx, "rules", leaf), o, d, m, skip)
        check_found(f, h, d.shape[1], (name, leaf))
        assert np.array_equal(_host(last).view(np.uint32), np.where(h.hit != 0, h.prim, skip))


@pytest.mark.parametrize("count", [-3, 0, 100, 256, 300, 301, 5000])
def test_device_count(ctx, sphere_stream, count):
    o, d, m, skip, h = sphere_stream
    n = 300
    f, last, _ = query(ctx, scene_of(ctx, "icosphere"), o[:, :n], d[:, :n], m[:n], skip[:n], count=count)
    traced = min(n, max(count, 0))
    check_found(f, h, traced, ("device count", count))
    want = skip[:n].copy()
    want[:traced] = np.where(h.hit[:traced] != 0, h.prim[:traced], skip[:traced])
    assert np.array_equal(_host(last).view(np.uint32), want)


@pytest.mark.parametrize("planes", [(), ("P",), ("N",), ("Ns",), ("T",), ("wo",), ("prim",), ("surface",), ("u",), ("v",),
                                    ("P", "surface"), ("P", "N", "Ns", "surface")], ids=lambda p: "+".join(p) or "hit,t")
def test_optional_planes(ctx, planes):
    o, d, m, skip, h = soup_stream()
    f, last, _ = query(ctx, scene_of(ctx, "soup"), o, d, m, skip if len(planes) != 1 else None, planes=planes)
    if last is None:                                                 # `last` absent too: nothing is skipped
        h = _cache.setdefault("soup300 no skip", U.nearest_np(mesh_of("soup"), o, d, m))
    check_found(f, h, 300, planes, planes=planes)
    for name in VEC + SCALAR:
        assert (getattr(f, name) is None) == (name not in planes)


def test_last_through_a_permuted_id_plane(ctx, sphere_stream):
    o, d, m, skip, h0 = sphere_stream
    n = 300
    rng = np.random.default_rng(17)
    ids = rng.permutation(400)[:n]                                   # ids past the entries, 100 of them unused
    last0 = rng.integers(0, 320, 400).astype(np.uint32)
    last0[rng.random(400) < 0.5] = NO_PRIM
    h = U.nearest_np(mesh_of("icosphere"), o[:, :n], d[:, :n], m[:n], last0[ids])
    f, last, _ = query(ctx, scene_of(ctx, "icosphere"), o[:, :n], d[:, :n], m[:n], last0, ids=ids)
    check_found(f, h, n, "permuted ids")
    want = last0.copy()
    want[ids] = np.where(h.hit != 0, h.prim, last0[ids])
    assert np.array_equal(_host(last).view(np.uint32), want)
    assert not np.array_equal(h.hit, h0.hit[:n]) or not np.array_equal(h.prim, h0.prim[:n])   # the skips changed something


def _bytes(f, names=("hit", "t") + VEC + SCALAR):
    return [_host(getattr(f, k).contiguous().view(torch.uint8)) for k in names]


def test_leaf_sizes_give_the_same_bytes(ctx):
    mesh = mesh_of("soup")
    o, d, m, skip = mixed_rays(mesh, 600, 23)
    got = []
    for leaf in (1, 2, 4, 8):
        scene = scene_of(ctx, "soup", leaf)
        assert scene.leaf_size == leaf and scene.depth <= int(np.ceil(np.log2(1025 / leaf))) + 1
        f, last, _ = query(ctx, scene, o, d, m, skip)
        got.append(_bytes(f) + [_host(last)])
    assert len({scene_of(ctx, "soup", leaf).nodes for leaf in (1, 2, 4, 8)}) == 4
    for other in got[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(got[0], other))
    check_found(f, U.nearest_np(mesh, o, d, m, skip), 600, "leaf 8")


def test_exact_and_fast_contexts_give_the_same_bytes(ctx, sphere_stream):
    o, d, m, skip, h = sphere_stream
    fast = R.Context(0)
    fast.set_math_mode(True)
    try:
        scene = scene_of(ctx, "icosphere")
        a, la, _ = query(ctx, scene, o, d, m, skip)
        b, lb, _ = query(ctx, scene, o, d, m, skip, use_ctx=fast)
    finally:
        fast.close()
    assert all(np.array_equal(x, y) for x, y in zip(_bytes(a) + [_host(la)], _bytes(b) + [_host(lb)]))
    check_found(b, h, d.shape[1], "fast")
    from rlshaders_amd import build
    from rlshaders_amd.codeid import code_objects, fatbin
    assert len(code_objects(fatbin(build.NEAREST_LIB))) == 1         # mode-free: one code object


def test_bin_plane_is_the_table_lookup(ctx):
    o, d, m, skip, h = soup_stream()
    table =np.array([3, 0, 255, 1, 2, 0, 7], np.uint8)              # surfaces run to 299: most are past the table
    assert (h.surface[h.hit != 0] >= len(table)).sum() > 20 and (h.surface[h.hit != 0] < len(table)).sum() > 0
    f, _, _ = query(ctx, scene_of(ctx, "soup"), o, d, m, skip, bin_table=table, count=280)
    check_found(f, h, 280, "bins", bin_table=table)
    assert f.bins() is f.bin
    one = np.array([5], np.uint8)                                    # a table of one entry: every hit reads it
    g, _, _ = query(ctx, scene_of(ctx, "soup"), o, d, m, skip, bin_table=one, planes=())
    assert np.array_equal(_host(g.bin), np.where(h.hit != 0, 5, 255).astype(np.uint8))


def test_walk_list_entry_point(ctx, sphere_stream):
    """rls_nearest_walk_hits over a list as the walks hold it: its device count, its ray plane as the ids of `last`"""
    from rlshaders_amd import nearest
    o, d, m, skip, _ = sphere_stream
    cap, count = 300, 270
    rng = np.random.default_rng(29)
    ids = np.sort(rng.permutation(500)[:cap])                        # ascending queue rays, as a walk lists them
    last0 = np.full(500, NO_PRIM, np.uint32)
    last0[ids] = skip[:cap]
    lst = SimpleNamespace(count=torch.tensor([count], dtype=torch.int64, device="cuda"), ray=_ids(ids), origin=_dev(o[:, :cap]),
                          dir=_dev(d[:, :cap]), maxdist=_dev(m[:cap]), trials=torch.zeros(cap, dtype=torch.uint8, device="cuda"))
    h = U.nearest_np(mesh_of("icosphere"), o[:, :cap], d[:, :cap], m[:cap], skip[:cap])
    scene = scene_of(ctx, "icosphere")
    for active, traced in ((None, count), (cap, count), (200, 200)):
        alloc = Guarded()
        f = nearest.Found(ctx, cap if active is None else active, alloc=alloc)
        last = _ids(last0)
        scene.hits(lst, active=active, last=last, found=f)
        torch.cuda.synchronize()
        alloc.check()
        check_found(f, h, traced, ("list", active))
        want = last0.copy()
        want[ids[:traced]] = np.where(h.hit[:traced] != 0, h.prim[:traced], skip[:traced])
        assert np.array_equal(_host(last).view(np.uint32), want)
    wf = f.walk_found()
    assert wf.object is f.surface and wf.Ns is f.Ns
    sf = f.shadow_found(torch.zeros(3, 4, device="cuda"))
    assert sf.index is f.surface and sf.P is f.P


def test_one_graph_replay(ctx, sphere_stream):
    from rlshaders_amd import nearest
    o, d, m, skip, h = sphere_stream
    n = 300
    scene = scene_of(ctx, "icosphere")
    side = torch.cuda.Stream()                                       # (the NULL stream cannot be captured)
    gctx = R.Context(0)
    gctx.use_stream(side)
    try:
        rays = nearest.Rays(_dev(o[:, :n]), _dev(d[:, :n]), _dev(m[:n]))
        last = _ids(skip[:n])
        alloc = Guarded()
        f = nearest.Found(gctx, n, alloc=alloc)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            scene.hits(rays, last=last, found=f, ctx=gctx)
        torch.cuda.synchronize()
        for buf, _ in alloc.outer:
            buf.fill_(SENTINEL)
        last.copy_(_ids(skip[:n]))
        graph.replay()
        torch.cuda.synchronize()
        alloc.check()
        check_found(f, h, n, "replay")
        del graph
    finally:
        gctx.close()


def test_refusals_on_the_device_path(ctx):
    from rlshaders_amd import nearest
    mesh = mesh_of("single")
    with pytest.raises(Exception, match="index >= mesh.nv"):
        nearest.Scene(ctx, mesh.V, [(0, 1, 3)])
    with pytest.raises(Exception, match="NaN or an inf"):
        nearest.Scene(ctx, [(0, 0, 0), (1, 0, np.nan), (0, 1, 0)], mesh.tri)
    with pytest.raises(Exception, match="leaf_size"):
        nearest.Scene(ctx, mesh.V, mesh.tri, leaf_size=9)
    s = nearest.Scene(ctx, mesh.V, mesh.tri)
    assert (s.nt, s.nodes, s.depth, s.leaf_size) == (1, 1, 1, 4) and s.device_bytes > 0
    # `last` shorter than the rays whose ids are their indices: refused on the host, not written past on the device
    z = torch.zeros(3, 8, device="cuda")
    with pytest.raises(ValueError, match="last: 7 entries for 8 rays"):
        s.hits(nearest.Rays(z, z), last=torch.full((7,), -1, dtype=torch.int32, device="cuda"))
    s.close()
    s.close()
