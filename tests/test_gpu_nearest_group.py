"""-m gpu: rls_nearest_group_hits / rls_nearest_group_walk_hits / rls_nearest_group_update (librls_nearest_group.so,
rlshaders_amd/nearest_group.py) against the numpy statement (tests/nearest_group_util.py, group_np), bit for bit in every written
plane, every ray, no exclusions -- groups of 1, 2, 3, 5, 64 and 300 general placements of the 320-triangle icosphere (with vertex
normals) and of a quad grid (without), 4096 rays with reaches and hostile rays among them; via, a device count, ray ids with the
pair last / last_instance, bin; every plane alone and all together inside sentinel-filled buffers (planes not asked for and
missed entries untouched); the same bytes for top leaf sizes 1 and 4 and under a FAST context; a group of no instances and a
group of parked ones; the update (new matrices, a member scene's refit, a NaN matrix, one graph replay) equal to a fresh group."""
import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_group_util as G
import nearest_util as U
from nearest_group_util import group_rays, skips
from nearest_util import F, NO_PRIM
from test_gpu_nearest import Guarded, _dev, _host, _ids, same_bits, untouched

pytestmark = pytest.mark.gpu

VEC = ("P", "N", "Ns", "T", "wo")
SCALAR = ("prim", "surface", "u", "v", "instance")
RAYS = 4096


@pytest.fixture(scope="module")
def ctx():
    from rlshaders_amd import nearest_group
    nearest_group.load()                                             # (a missing library is an error, not a build)
    c = R.Context(0)
    yield c
    c.close()


_meshes = {}


def mesh_of(name):
    if name not in _meshes:
        _meshes[name] = U.icosphere(2) if name == "icosphere" else U.quad_grid(9)
    return _meshes[name]


class DeviceGroup:
    """the scenes (one per distinct mesh) and the nearest_group.Group of a list of nearest_group_util.Inst"""

    def __init__(self, ctx, insts, leaf=0, scene_leaf=0):
        from rlshaders_amd import nearest, nearest_group
        self.scenes = {}
        for i in insts:
            if id(i.mesh) not in self.scenes:
                m = i.mesh
                self.scenes[id(m)] = nearest.Scene(ctx, m.V, m.tri, surface=m.surface, normals=m.normals, leaf_size=scene_leaf)
        self.group = nearest_group.Group(ctx, [nearest_group.Instance(self.scenes[id(i.mesh)], i.B, surface_base=i.base, to_object=i.A)
                                               for i in insts], leaf_size=leaf)

    def close(self):
        self.group.close()
        for s in self.scenes.values():
            s.close()


def check_found(f, h, traced, what, bin_table=None, planes=VEC + SCALAR):
    n = f.rays
    hit = _host(f.hit)
    assert np.array_equal(hit[:traced], h.hit[:traced]), (what, "hit", np.flatnonzero(hit[:traced] != h.hit[:traced])[:8])
    written = np.zeros(n, bool)
    written[:traced] = h.hit[:traced] != 0
    past = np.arange(n) >= traced
    untouched(f.hit, past, (what, "hit past the count"))
    for name in ("t",) + tuple(planes):
        t, want = getattr(f, name), getattr(h, name)
        got = _host(t)
        if name in ("prim", "surface", "instance"):
            got = got.view(np.uint32)
        same_bits(got[..., written], want[..., :n][..., written], (what, name))
        untouched(t, ~written, (what, name, "missed or past the count"))
    if bin_table is not None:
        want = np.where(h.hit[:traced] != 0, bin_table[np.minimum(h.surface[:traced].astype(np.int64), len(bin_table) - 1)], 255)
        assert np.array_equal(_host(f.bin)[:traced], want.astype(np.uint8)), (what, "bin")
        untouched(f.bin, past, (what, "bin past the count"))


def query(ctx, group, o, d, m=None, skip=None, rays=None, count=None, via=None, table=None, planes=VEC + SCALAR, bin_table=None,
          ids=None, use_ctx=None):
    """one guarded query -> (Found, last, last_instance)"""
    from rlshaders_amd import nearest, nearest_group
    n = d.shape[1] if rays is None else rays
    alloc = Guarded()
    f = nearest_group.Found(ctx, n, planes=planes, bin=bin_table is not None, alloc=alloc)
    r = nearest.Rays(_dev(o if table is None else table), _dev(d), None if m is None else _dev(m),
                     via=None if via is None else _ids(via), ray=None if ids is None else _ids(ids),
                     count=None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda"), rays=n)
    last = last_instance = None
    if skip is not None:
        last_instance, last = alloc((len(skip[0]),), torch.int32), alloc((len(skip[1]),), torch.int32)
        last_instance.copy_(_ids(skip[0]))
        last.copy_(_ids(skip[1]))
    group.hits(r, last=last, last_instance=last_instance, found=f, bin_of_surface=None if bin_table is None else _dev(bin_table), ctx=use_ctx)
    torch.cuda.synchronize()
    alloc.check()
    return f, last, last_instance


def all_bytes(f, planes=VEC + SCALAR):
    return [_host(f.hit)] + [_host(getattr(f, k)) for k in ("t",) + tuple(planes)]


def stream_of(insts, seed):
    o, d, m = group_rays(insts, RAYS - 64, seed)
    first = G.group_np(insts, o, d, m)
    return o, d, m, skips(np.random.default_rng(seed + 1), first)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 300])
@pytest.mark.parametrize("name", ["icosphere", "grid"])
def test_device_equals_the_statement(ctx, name, n):
    insts = G.general_instances(mesh_of(name), n, seed=n + (7 if name == "grid" else 0))
    o, d, m, skip = stream_of(insts, n)
    h = G.group_np(insts, o, d, m, skip)
    assert 0.2 < (h.hit != 0).mean() < 0.98
    g = DeviceGroup(ctx, insts)
    try:
        info = g.group.info()
        assert info["instances"] == n and info["scenes"] == 1 and info["top_depth"] <= int(np.ceil(np.log2(max(n / 2, 1)))) + 1
        f, last, last_instance = query(ctx, g.group, o, d, m, skip)
        check_found(f, h, d.shape[1], (name, n))
        hit = h.hit != 0
        assert np.array_equal(_host(last).view(np.uint32), np.where(hit, h.prim, skip[1]))
        assert np.array_equal(_host(last_instance).view(np.uint32), np.where(hit, h.instance, skip[0]))
    finally:
        g.close()


@pytest.fixture(scope="module")
def five(ctx):
    a, b = mesh_of("icosphere"), mesh_of("grid")
    insts = [v for pair in zip(G.general_instances(a, 3, seed=31), G.general_instances(b, 3, seed=32)) for v in pair][:5]
    for k, i in enumerate(insts):
        i.base = 40 * k
    o, d, m, skip = stream_of(insts, 5)
    g = DeviceGroup(ctx, insts)
    yield insts, g, (o, d, m, skip), G.group_np(insts, o, d, m, skip)
    g.close()


def test_via_count_ids_and_bin(ctx, five):
    insts, g, (o, d, m, skip), _ = five
    M = d.shape[1]
    rng = np.random.default_rng(3)
    table = rng.uniform(-2, 2, (3, 97)).astype(F)                    # a queue's point plane: origins through via
    via = rng.integers(0, 97, M).astype(np.uint32)
    ids = rng.permutation(M + 40)[:M].astype(np.uint32)              # the pair is indexed by the ray's id
    sj, si = np.full(M + 40, G.NO_INSTANCE, np.uint32), np.full(M + 40, NO_PRIM, np.uint32)
    sj[ids], si[ids] = skip
    bins = rng.integers(0, 6, 150).astype(np.uint8)                  # fewer entries than based surface ids: the last one serves the rest
    count = M - 300
    h = G.group_np(insts, table[:, via], d, m, skip)
    f, last, last_instance = query(ctx, g.group, None, d, m, (sj, si), table=table, via=via, ids=ids, count=count, bin_table=bins)
    check_found(f, h, count, "via", bin_table=bins)
    hit = (h.hit != 0) & (np.arange(M) < count)
    assert (h.surface[hit] >= 150).any()
    wj, wi = sj.copy(), si.copy()
    wj[ids[hit]], wi[ids[hit]] = h.instance[hit], h.prim[hit]
    assert np.array_equal(_host(last).view(np.uint32), wi) and np.array_equal(_host(last_instance).view(np.uint32), wj)


@pytest.mark.parametrize("planes", [()] + [(k,) for k in VEC + SCALAR] + [("N", "T"), ("Ns", "instance", "u")])
def test_every_plane_alone(ctx, five, planes):
    insts, g, (o, d, m, skip), h = five
    f, _, _ = query(ctx, g.group, o, d, m, skip, planes=planes)
    check_found(f, h, d.shape[1], planes, planes=planes)
    for k in VEC + SCALAR:
        assert (getattr(f, k) is None) == (k not in planes)


def test_leaf_sizes_and_a_fast_context_give_the_same_bytes(ctx, five):
    insts, g, (o, d, m, skip), h = five
    want = all_bytes(query(ctx, g.group, o, d, m, skip)[0])
    for leaf, scene_leaf in ((1, 1), (4, 8), (3, 2)):
        other = DeviceGroup(ctx, insts, leaf=leaf, scene_leaf=scene_leaf)
        try:
            assert other.group.info()["leaf_size"] == leaf
            for x, y in zip(want, all_bytes(query(ctx, other.group, o, d, m, skip)[0])):
                assert np.array_equal(x, y), leaf
        finally:
            other.close()
    fast = R.Context(0)
    fast.set_math_mode(True)
    try:
        for x, y in zip(want, all_bytes(query(ctx, g.group, o, d, m, skip, use_ctx=fast)[0])):
            assert np.array_equal(x, y)
    finally:
        fast.close()


def test_walk_list_entry_point(ctx, five):
    """rls_nearest_group_walk_hits over a list in the shape of a walk's: count, ray, origin, dir, maxdist"""
    from types import SimpleNamespace
    from rlshaders_amd import nearest_group
    insts, g, (o, d, m, skip), _ = five
    M = d.shape[1]
    ids = np.random.default_rng(8).permutation(M).astype(np.uint32)
    lst = SimpleNamespace(count=torch.tensor([M - 100], dtype=torch.int64, device="cuda"), ray=_ids(ids), origin=_dev(o), dir=_dev(d),
                          maxdist=_dev(m))
    sj, si = np.empty(M, np.uint32), np.empty(M, np.uint32)
    sj[ids], si[ids] = skip
    alloc = Guarded()
    f = nearest_group.Found(ctx, M, alloc=alloc)
    last, last_instance = _ids(si), _ids(sj)
    g.group.hits(lst, active=M - 50, last=last, last_instance=last_instance, found=f)        # the device count is the smaller
    torch.cuda.synchronize()
    alloc.check()
    check_found(f, G.group_np(insts, o, d, m, skip), M - 100, "list")


def test_no_instances_and_parked_instances_miss_everywhere(ctx):
    mesh = mesh_of("icosphere")
    o, d = U.random_rays(np.random.default_rng(4), 1000)
    nanB, infA = G.IDENTITY.copy(), G.IDENTITY.copy()
    nanB[0, 0], infA[2, 3] = np.nan, np.inf
    for insts in ([], [G.Inst(mesh, nanB, G.IDENTITY), G.Inst(U.empty_mesh()), G.Inst(mesh, G.IDENTITY, infA)]):
        g = DeviceGroup(ctx, insts)
        try:
            f, _, _ = query(ctx, g.group, o, d)
            check_found(f, G.group_np(insts, o, d), 1000, len(insts))
            assert not _host(f.hit).any()
            if insts:
                boxes, links, order, world, parked = g.group.read_tree()
                assert parked.all() and not world.any() and not boxes.any() and sorted(order) == [0, 1, 2]
        finally:
            g.close()


# ---- the update ----------------------------------------------------------------------------------------------------------------------
def moved(insts, seed):
    """the same meshes and bases under new general placements"""
    new = G.general_instances(insts[0].mesh, len(insts), seed=seed)
    return [G.Inst(i.mesh, n.B, n.A, base=i.base) for i, n in zip(insts, new)]


def test_update_equals_a_fresh_group(ctx, five):
    insts, _, (o, d, m, skip), _ = five
    g = DeviceGroup(ctx, insts)
    try:
        for seed in (61, 62):
            new = moved(insts, seed)
            A, B = G.matrices(new)
            parked = torch.full((1,), -7, dtype=torch.int64, device="cuda")
            g.group.update(_dev(A), _dev(B), parked=parked)
            f, _, _ = query(ctx, g.group, o, d, m, skip)
            assert int(parked.item()) == 0
            check_found(f, G.group_np(new, o, d, m, skip), d.shape[1], ("update", seed))
            fresh = DeviceGroup(ctx, new)
            try:
                for x, y in zip(all_bytes(f), all_bytes(query(ctx, fresh.group, o, d, m, skip)[0])):
                    assert np.array_equal(x, y)
                # every top node's box is the union of what is below it; the world boxes are the fresh group's
                boxes, links, order, world, _ = g.group.read_tree()
                assert np.array_equal(world, fresh.group.read_tree()[3])
                assert np.array_equal(world, np.stack([np.concatenate([i.wlo, i.whi]) for i in new]))
                slot = np.argsort(order)
                for node in range(links.shape[0] - 1, -1, -1):
                    first, count = int(links[node, 0]), int(links[node, 1]) & 0xFF
                    below = world[order[first:first + count]] if count else boxes[first:first + 2]
                    assert np.array_equal(boxes[node], np.concatenate([below[:, :3].min(axis=0), below[:, 3:].max(axis=0)])), node
                assert sorted(slot) == list(range(len(insts)))
            finally:
                fresh.close()
        assert g.group.info()["updates"] == 2
        # a NaN written into one matrix parks exactly that instance
        A, B = G.matrices(new)
        A[3, 5] = np.nan
        parked = torch.zeros(1, dtype=torch.int64, device="cuda")
        g.group.update(_dev(A), _dev(B), parked=parked)
        f, _, _ = query(ctx, g.group, o, d, m, skip)
        assert int(parked.item()) == 1 and list(g.group.read_tree()[4]) == [0, 0, 0, 1, 0]
        nanA = new[3].A.copy()
        nanA[1, 1] = np.nan
        check_found(f, G.group_np(new[:3] + [G.Inst(new[3].mesh, new[3].B, nanA, base=new[3].base)] + new[4:], o, d, m, skip), d.shape[1], "nan")
    finally:
        g.close()


def test_update_after_a_refit_of_a_member_scene(ctx):
    from rlshaders_amd import nearest_refit
    mesh = mesh_of("icosphere")
    insts = G.general_instances(mesh, 4, seed=71)
    o, d, m, skip = stream_of(insts, 71)
    g = DeviceGroup(ctx, insts)
    try:
        scene = g.scenes[id(mesh)]
        refit = nearest_refit.Refit(scene)
        V = (mesh.V * F([1.5, 0.5, 1.25]) + F([0.25, 0.0, -0.5])).astype(F)         # well outside the old box
        refit.update(_dev(V))
        g.group.update(None, None)
        squashed = U.Mesh(V, mesh.tri, surface=mesh.surface, normals=mesh.normals)
        new = [G.Inst(squashed, i.B, i.A, base=i.base) for i in insts]
        f, _, _ = query(ctx, g.group, o, d, m, skip)
        h = G.group_np(new, o, d, m, skip)
        assert not np.array_equal(h.hit, G.group_np(insts, o, d, m, skip).hit)
        check_found(f, h, d.shape[1], "refit")
        assert np.array_equal(g.group.read_tree()[3], np.stack([np.concatenate([i.wlo, i.whi]) for i in new]))
        refit.close()
    finally:
        g.close()


def test_update_and_hits_in_one_graph(five):
    from rlshaders_amd import nearest, nearest_group
    insts, _, (o, d, m, skip), _ = five
    gctx = R.Context(0, use_torch_stream=False)                      # the context's own stream: the NULL stream cannot be captured
    g = DeviceGroup(gctx, insts)
    try:
        A, B = (_dev(x) for x in G.matrices(insts))
        parked = torch.zeros(1, dtype=torch.int64, device="cuda")
        rays = nearest.Rays(_dev(o), _dev(d), _dev(m))
        f = nearest_group.Found(gctx, d.shape[1])
        f.hit.fill_(7)
        torch.cuda.synchronize()
        with gctx.capture() as graph:
            g.group.update(A, B, parked=parked)
            g.group.hits(rays, found=f)
        torch.cuda.synchronize()
        assert (_host(f.hit) == 7).all()                             # recording runs nothing
        new = moved(insts, 81)
        nA, nB = G.matrices(new)
        nA[1, 0] = np.inf
        A.copy_(_dev(nA))                                            # in place: the graph reads the tensors as they are then
        B.copy_(_dev(nB))
        torch.cuda.synchronize()
        graph.launch()
        gctx.synchronize()
        infA = new[1].A.copy()
        infA[0, 0] = np.inf
        want = G.group_np([new[0], G.Inst(new[1].mesh, new[1].B, infA, base=new[1].base)] + new[2:], o, d, m)
        assert int(parked.item()) == 1
        check_found_plain(f, want)
        graph.close()
    finally:
        g.close()
        gctx.close()


def check_found_plain(f, h):
    """a Found of torch.empty planes: every written entry, no sentinels"""
    hit = h.hit != 0
    assert np.array_equal(_host(f.hit), h.hit)
    for name in ("t",) + VEC + SCALAR:
        got = _host(getattr(f, name))
        if name in ("prim", "surface", "instance"):
            got = got.view(np.uint32)
        same_bits(got[..., hit], getattr(h, name)[..., hit], name)
