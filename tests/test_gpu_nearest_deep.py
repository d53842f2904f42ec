"""-m gpu: nearest_kernel (librls_nearest.so) on trees as deep as its per-lane LDS stack is sized for.  Every other nearest test
runs meshes of at most 2 178 triangles -- 12 levels, stack words 0 .. 10; here

  - deep_grid (2^21 + 20 triangles, 23 levels at leaf_size 1) on the 577 rays of nearest_util.deep_stream: the corner ray alone
    in lane 0 of a wavefront of random rays, a wavefront of 64 corner rays, one that alternates corner and reversed rays, rays
    whose hit comes out of a sibling pushed at a high index -- 22 entries held, stack words 0 .. 21 written, the documented worst
    case.  Every plane of rls_nearest_hits (hit, t, prim, surface, u, v, P, N, Ns, T, wo, bin, `last`) = the brute force of
    tests/native/nearest_host_check.cpp over every triangle plus the numpy frame (nearest_util.hits_at), as bits, inside
    sentinel-filled buffers; a second query carrying `last` = the brute force with the first hit skipped (the rays from above
    go on from the extra triangles to the grid below);
  - deep_grid at leaf_size 8 and mid_soup (2^17 + 1 triangles) at leaf_size 1, 2, 4, 8: the same bytes, = the reference;
  - the deep stream on a context of one workgroup per CU and on a FAST context: the default context's bytes;
  - copies (4097 coincident triangles: a ray opens every node, the traversal's loop bound met with equality) and huge_soup
    (coordinates up to 3e38, subnormal triangles) = nearest_np in every plane, for every leaf size;
  - rls_nearest_walk_hits over a walk's list of the 577 rays = rls_nearest_hits; one graph replay of the deep query.
The references are made by the host program and numpy in module fixtures before any launch, the caps on the stream (at least
30 % hits, at least 65 rays that hold depth - 1 entries in the host run of the traversal source) are asserted with them.  A wrong
kernel cannot hang: the traversal's loop is bounded by node_count.

Wall time of this module on the MI355X machine: 6.7 s, 2.9 s of it the module's references (the host program's build of the
2^21-triangle tree and its two brute forces), no test above 1 s; test_gpu_nearest.py takes 4.0 s there."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_util as U
from nearest_util import NO_PRIM
from nearest_host_check_util import build, mixed_stream, run_file, write_mesh
from test_gpu_nearest import SENTINEL, Guarded, _bytes, _dev, _host, _ids, check_found, query

pytestmark = pytest.mark.gpu

LEAVES = (1, 2, 4, 8)
BINS = np.array([3, 0, 255, 1, 2, 0, 7], np.uint8)                   # the deep grid's surfaces: 0 .. 4, and 1000 .. past the table


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frame(mesh, o, d, m, skip, r):
    """the brute force's (prim, t) -> every plane; the t recomputed in numpy must be the program's"""
    h = U.hits_at(mesh, o, d, r.prim, m, skip)
    assert np.array_equal(h.hit != 0, r.hit) and np.array_equal(bits(h.t)[r.hit], bits(r.t)[r.hit])
    return h


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """meshes, streams and references, before any launch"""
    work = tmp_path_factory.mktemp("gpu_nearest_deep")
    exe = build(work)
    out = {}
    mesh = U.deep_grid()
    path = write_mesh(work / "deep_grid.bin", mesh)
    o, d, m, skip, info = U.deep_stream(mesh)
    r = run_file(exe, path, o, d, m, skip, leaf=1)
    # the caps, before anything is compared
    assert r.depth == 23 and r.hit.mean() >= 0.30, (r.depth, r.hit.mean())
    full = r.max_stack == r.depth - 1
    assert full.sum() >= 65 and r.max_stack.max() == 22 and full[0] and full[64:128].all() and full[128:192:2].all(), int(full.sum())
    assert np.array_equal(r.tree_prim, r.prim) and r.differ == 0
    assert np.array_equal(r.prim[info["vertical"]], info["vertical_prim"]) and np.array_equal(r.prim[info["above"]], info["above_prim"])
    last = np.where(r.hit, r.prim, skip).astype(np.uint32)
    r2 = run_file(exe, path, o, d, m, last)
    assert r2.hit[info["above"]].all() and (r2.prim[info["above"]] < (1 << 21)).all() and r2.hit.sum() >= 40
    out["deep_grid"] = SimpleNamespace(mesh=mesh, rays=(o, d, m, skip), info=info, h=frame(mesh, o, d, m, skip, r), last=last,
                                       h2=frame(mesh, o, d, m, last, r2), last2=np.where(r2.hit, r2.prim, last).astype(np.uint32))
    mesh = U.mid_soup()
    path = write_mesh(work / "mid_soup.bin", mesh)
    rays = mixed_stream(exe, path, mesh, 1024, 17)
    r = run_file(exe, path, *rays)
    assert 0.3 < r.hit.mean() < 0.98
    out["mid_soup"] = SimpleNamespace(mesh=mesh, rays=rays, h=frame(mesh, *rays, r), last=np.where(r.hit, r.prim, rays[3]).astype(np.uint32))
    for name, make in (("copies", lambda mesh: U.copies_rays(mesh.nt)), ("huge_soup", U.huge_rays)):
        mesh = U.DEEP_MESHES[name]()
        rays = make(mesh)
        h = U.nearest_np(mesh, *rays)
        assert h.hit.any() and not h.hit.all()
        out[name] = SimpleNamespace(mesh=mesh, rays=rays, h=h, last=np.where(h.hit != 0, h.prim, rays[3]).astype(np.uint32))
    return out


@pytest.fixture(scope="module")
def ctx(ref):
    from rlshaders_amd import nearest
    nearest.load()                                                   # (a missing library is an error, not a build)
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes(ctx, ref):
    """scene(name, leaf): uploaded once for the module"""
    from rlshaders_amd import nearest
    made = {}

    def scene(name, leaf):
        if (name, leaf) not in made:
            m = ref[name].mesh
            made[name, leaf] = nearest.Scene(ctx, m.V, m.tri, surface=m.surface, normals=m.normals, leaf_size=leaf)
        return made[name, leaf]

    yield scene
    for s in made.values():
        s.close()


def run_query(ctx, scene, case, skip=None, **kw):
    o, d, m, s = case.rays
    return query(ctx, scene, o, d, m, s if skip is None else skip, bin_table=BINS, **kw)


def all_bytes(f, last):
    return _bytes(f) + [_host(f.bin), _host(last)]


def check(f, last, h, want_last, what):
    check_found(f, h, f.rays, what, bin_table=BINS)
    assert np.array_equal(_host(last).view(np.uint32), want_last), (what, "last")


def test_deep_grid_at_leaf_1_every_plane_and_last_carried(ctx, scenes, ref):
    case = ref["deep_grid"]
    s = scenes("deep_grid", 1)
    assert s.depth == 23 and s.nt == (1 << 21) + 20 and s.depth - 1 <= U.STACK and s.nodes == 2 * s.nt - 1
    f, last, _ = run_query(ctx, s, case)
    check(f, last, case.h, case.last, "deep_grid leaf 1")
    assert (_host(f.prim).view(np.uint32)[case.info["above"]] == case.info["above_prim"]).all()
    g, last2, _ = run_query(ctx, s, case, skip=_host(last).view(np.uint32))
    check(g, last2, case.h2, case.last2, "deep_grid leaf 1, last carried")
    above = case.info["above"]
    assert _host(g.hit)[above].all() and (np.abs(_host(g.P)[2, above]) <= 1e-3).all() and (np.abs(_host(f.P)[2, above] - 1.0) <= 1e-6).all()


def test_deep_grid_at_leaf_8_gives_the_same_bytes(ctx, scenes, ref):
    case = ref["deep_grid"]
    s = scenes("deep_grid", 8)
    assert s.depth == 20 and s.leaf_size == 8
    a, la, _ = run_query(ctx, scenes("deep_grid", 1), case)
    b, lb, _ = run_query(ctx, s, case)
    assert all(np.array_equal(x, y) for x, y in zip(all_bytes(a, la), all_bytes(b, lb)))
    check(b, lb, case.h, case.last, "deep_grid leaf 8")


def test_mid_soup_every_leaf_size(ctx, scenes, ref):
    case = ref["mid_soup"]
    got = []
    for leaf in LEAVES:
        s = scenes("mid_soup", leaf)
        assert s.leaf_size == leaf and s.depth <= int(np.ceil(np.log2(s.nt / leaf))) + 1 and (leaf != 1 or s.depth == 19)
        f, last, _ = run_query(ctx, s, case)
        check(f, last, case.h, case.last, ("mid_soup", leaf))
        got.append(all_bytes(f, last))
    for other in got[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(got[0], other))


def test_capped_and_fast_contexts_give_the_default_bytes(ctx, scenes, ref):
    case = ref["deep_grid"]
    s = scenes("deep_grid", 1)
    a, la, _ = run_query(ctx, s, case)
    mp = pytest.MonkeyPatch()
    mp.setenv("RLS_BLOCKS_PER_CU", "1")                              # read at context creation: one workgroup per CU
    try:
        capped = R.Context(0)
    finally:
        mp.undo()
    fast = R.Context(0)
    fast.set_math_mode(True)
    try:
        for name, other in (("capped", capped), ("fast", fast)):
            b, lb, _ = run_query(ctx, s, case, use_ctx=other)
            assert all(np.array_equal(x, y) for x, y in zip(all_bytes(a, la), all_bytes(b, lb))), name
            check(b, lb, case.h, case.last, name)
    finally:
        capped.close()
        fast.close()


@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("name", ["copies", "huge_soup"])
def test_copies_and_huge_coordinates_are_the_statement(ctx, scenes, ref, name, leaf):
    """huge_soup holds subnormal vertices and rays: a device that flushed them where the statement does not would differ here"""
    case = ref[name]
    s = scenes(name, leaf)
    assert s.nt == case.mesh.nt and s.depth - 1 <= U.STACK
    if name == "copies":
        assert leaf == 2 or s.nodes == {1: 8193, 4: 2049, 8: 1025}[leaf]
    f, last, _ = run_query(ctx, s, case)
    check(f, last, case.h, case.last, (name, leaf))


def test_walk_list_entry_point_on_the_deep_grid(ctx, scenes, ref):
    from rlshaders_amd import nearest
    case = ref["deep_grid"]
    o, d, m, skip = case.rays
    n = d.shape[1]
    s = scenes("deep_grid", 1)
    a, la, _ = run_query(ctx, s, case)
    lst = SimpleNamespace(count=torch.tensor([n], dtype=torch.int64, device="cuda"), ray=_ids(np.arange(n)), origin=_dev(o),
                          dir=_dev(d), maxdist=_dev(m))
    alloc = Guarded()
    f = nearest.Found(ctx, n, bin=True, alloc=alloc)
    last = alloc((n,), torch.int32)
    last.copy_(_ids(skip))
    s.hits(lst, last=last, found=f, bin_of_surface=_dev(BINS))
    torch.cuda.synchronize()
    alloc.check()
    assert all(np.array_equal(x, y) for x, y in zip(all_bytes(a, la), all_bytes(f, last)))
    check(f, last, case.h, case.last, "walk list")


def test_one_graph_replay_of_the_deep_query(ctx, scenes, ref):
    from rlshaders_amd import nearest
    case = ref["deep_grid"]
    o, d, m, skip = case.rays
    n = d.shape[1]
    s = scenes("deep_grid", 1)
    side = torch.cuda.Stream()                                       # (the NULL stream cannot be captured)
    gctx = R.Context(0)
    gctx.use_stream(side)
    try:
        rays = nearest.Rays(_dev(o), _dev(d), _dev(m))
        table = _dev(BINS)
        alloc = Guarded()
        f = nearest.Found(gctx, n, bin=True, alloc=alloc)
        last = alloc((n,), torch.int32)
        last.copy_(_ids(skip))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            s.hits(rays, last=last, found=f, bin_of_surface=table, ctx=gctx)
        torch.cuda.synchronize()
        for buf, _ in alloc.outer:
            buf.fill_(SENTINEL)
        last.copy_(_ids(skip))
        graph.replay()
        torch.cuda.synchronize()
        alloc.check()
        check(f, last, case.h, case.last, "replay")
        del graph
    finally:
        gctx.close()
