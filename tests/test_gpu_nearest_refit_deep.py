"""-m gpu: the device's update on trees as deep as test_gpu_nearest_deep.py queries -- level lists of up to 2^20 nodes, int64 level
offsets past 2^16, 19 and 23 launches' worth of levels -- and the query on what such an update leaves: after a refit the sibling
boxes overlap wherever the mesh moved against the builder's splits, so a ray holds more stack entries and opens more nodes at
the same depth than on any tree the builder made.

  - mid_soup (2^17 + 1 triangles, 19 levels at leaf_size 1) moved by jittered(.., 0.15), at leaf 1 and leaf 8;
  - deep_grid (2^21 + 20 triangles, 23 levels at leaf_size 1) moved by twisted(.., 2.0), at leaf 1, and one further query on a
    context of one workgroup per CU gives the same bytes.
The read tree == the exact union on the moved mesh in every box (nearest_refit_util.union_fast, a frontier a level; == union_np
on small trees: test_nearest_refit_host.py), links and leaf order unchanged, and == the first read after the update back.
For each, on 1024 rays of nearest_host_check_util.mixed_stream over the moved mesh: after the update every plane of
rls_nearest_hits, bin and `last` = the brute force of tests/native/nearest_host_check.cpp over every triangle of the moved mesh
plus the numpy frame (nearest_util.hits_at), as bits, inside sentinel-filled buffers, = the bytes of a fresh scene on the moved
mesh; after the update back, the untouched scene's bytes.  The references are made by the host program and numpy in a module
fixture before any launch, with the cap on each stream (the brute force on the moved mesh hits between 0.3 and 0.98 of the
rays).  Neither move makes every box the whole scene (vertex positions permuted, a mesh collapsed: each ray would open
millions of nodes).  A wrong kernel cannot hang: the refit kernels' loops are bounded by `tiles` and `levels`, the
traversal's by node_count.

Wall time of this module on the MI355X machine: 8.2 s, 2.2 s of it the module's references (the host program's four brute
forces; test_gpu_nearest_deep.py: 6.7 s, 2.9 s), no test above 3.4 s (deep_grid: two trees of 2^21 triangles built on the host,
three reads of 2^22 nodes and the numpy union); nothing of the deep grid's checks was dropped."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_util as U
from nearest_host_check_util import build, mixed_stream, run_file, write_mesh
from nearest_refit_util import jittered, moved, twisted, union_fast
from test_gpu_nearest import _dev, _host, check_found, query
from test_gpu_nearest_deep import BINS, all_bytes, frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """the meshes, the moved meshes, the streams and the references, before any launch"""
    work = tmp_path_factory.mktemp("gpu_nearest_refit_deep")
    exe = build(work)
    out = {}
    for name, make, move in (("mid_soup", U.mid_soup, lambda m: jittered(m, 31, 0.15)), ("deep_grid", U.deep_grid, lambda m: twisted(m.V, 2.0))):
        mesh = make()
        b = moved(mesh, move(mesh))
        assert np.isfinite(b.V).all() and (b.V != mesh.V).mean() > 0.5
        path = write_mesh(work / f"{name}_moved.bin", b)
        rays = mixed_stream(exe, path, b, 1024, 17)
        r = run_file(exe, path, *rays)
        assert 0.3 < r.hit.mean() < 0.98, (name, r.hit.mean())
        out[name] = SimpleNamespace(mesh=mesh, moved=b, rays=rays, h=frame(b, *rays, r),
                                    last=np.where(r.hit, r.prim, rays[3]).astype(np.uint32))
    return out


@pytest.fixture(scope="module")
def ctx(ref):
    from rlshaders_amd import nearest, nearest_refit
    nearest.load(), nearest_refit.load()                             # (a missing library is an error, not a build)
    c = R.Context(0)
    yield c
    c.close()


def scene_on(ctx, mesh, leaf):
    from rlshaders_amd import nearest
    return nearest.Scene(ctx, mesh.V, mesh.tri, surface=mesh.surface, normals=mesh.normals, leaf_size=leaf)


def found(ctx, scene, case, **kw):
    f, last, _ = query(ctx, scene, *case.rays, bin_table=BINS, **kw)
    return f, last, all_bytes(f, last)


def same(a, b, what):
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), what


def refit_there_and_back(ctx, case, leaf, depth, capped=None):
    from rlshaders_amd import nearest_refit
    scene = scene_on(ctx, case.mesh, leaf)
    assert scene.depth == depth and scene.depth - 1 <= U.STACK
    refit = nearest_refit.Refit(scene)
    assert refit.levels == depth and refit.nodes == scene.nodes
    boxes0, links0, prims0 = refit.read_tree()
    assert leaf != 1 or links0.shape[0] == 2 * case.mesh.nt - 1
    _, _, before = found(ctx, scene, case)
    parked = torch.full((1,), 99, dtype=torch.int64, device="cuda")
    refit.update(_dev(case.moved.V), parked=parked)
    f, last, after = found(ctx, scene, case)
    check_found(f, case.h, f.rays, ("refit", leaf), bin_table=BINS)
    assert np.array_equal(_host(last).view(np.uint32), case.last) and int(parked.item()) == 0
    if capped is not None:
        same(found(ctx, scene, case, use_ctx=capped)[2], after, "one workgroup per CU")
    # a stale box need not show in 1024 rays (the deepest level of mid_soup is two leaves of 2^18 + 1 nodes): every box
    boxes, links, prims = refit.read_tree()
    assert np.array_equal(links, links0) and np.array_equal(prims, prims0)
    assert np.array_equal(boxes, union_fast(boxes, links, prims, case.moved.V, case.mesh.tri)), "the boxes on the moved mesh"
    fresh = scene_on(ctx, case.moved, leaf)
    same(found(ctx, fresh, case)[2], after, "a fresh scene on the moved mesh")
    fresh.close()
    refit.update(_dev(case.mesh.V))
    same(found(ctx, scene, case)[2], before, "back on the first mesh")
    assert np.array_equal(refit.read_tree()[0], boxes0), "the boxes back on the first mesh"
    refit.close(), scene.close()


@pytest.mark.parametrize("leaf,depth", [(1, 19), (8, 16)])
def test_mid_soup_jittered(ctx, ref, leaf, depth):
    refit_there_and_back(ctx, ref["mid_soup"], leaf, depth)


def test_deep_grid_twisted(ctx, ref):
    mp = pytest.MonkeyPatch()
    mp.setenv("RLS_BLOCKS_PER_CU", "1")                              # read at context creation: one workgroup per CU
    try:
        capped = R.Context(0)
    finally:
        mp.undo()
    try:
        refit_there_and_back(ctx, ref["deep_grid"], 1, 23, capped=capped)
    finally:
        capped.close()
