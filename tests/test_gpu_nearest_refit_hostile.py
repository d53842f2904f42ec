"""-m gpu: the device's update (refit_records_kernel, one refit_level_kernel launch per wide level, refit_top_kernel over the
folded top; rlshaders_amd/csrc_nearest/refit.hip) on the moves that tests/test_nearest_refit_host.py gives the CPU's serial loop:
vertices jittered, vertex positions dealt to other vertices, the mesh collapsed to a point, a grid flattened, coordinates up to
3e38, a quarter of the vertices non-finite -- its PAIRS, imported -- and `stacked` (nearest_refit_util): every triangle of a
4097-triangle soup moved onto the same three points, so that every hit ties on a tree whose leaf order was made for another mesh
and is arbitrary with respect to the triangle ids the statement breaks a tie by.

At leaf 1, 4 and 8: the scene is built on A, updated to B with a `parked` counter that holds junk, queried, updated back and
queried again.  read_tree: links and leaf order unchanged, boxes == the numpy union on B and finite, == the first read after the
update back; parked == the triangles of B with a non-finite coordinate, counted here, and 0 after the update back; every found
plane, bin and `last` == nearest_np on B (with the parked triangles made degenerate: they never hit), the bytes of a fresh scene
on B where B is finite, and the untouched scene's bytes after the update back.  Nothing here has a tolerance: the refit
compares and copies.

The caps are asserted on the numpy reference before anything is launched: at least half of the 512 rays hit on B and at least
half change their result between A and B (measured: hit share 0.65 .. 0.93, differing share 0.84 .. 0.93) -- an update that
does nothing, skips a level or leaves a stale root cannot pass --; `collapsed`: no ray hits on B, on rays aimed at where A stood
and at the point; `stacked`, on nearest_util.copies_rays: triangle 0 of the soup is degenerate, so triangle 1 wins every tie,
and the one ray that skips triangle 1 reports triangle 2 (7 of the 9 rays hit)."""
import numpy as np
import pytest
import torch

import nearest_util as U
from nearest_util import F
from nearest_refit_util import moved, stacked, union_np, without
from test_gpu_nearest import _dev, _host, check_found
from test_gpu_nearest_refit import BINS, ctx, device_scene, found_bytes, rays_for, same  # noqa: F401  (ctx: the module's fixture)
from test_nearest_refit_host import PAIRS

pytestmark = pytest.mark.gpu

assert "stacked" in PAIRS and PAIRS["stacked"][0] is stacked
_cache = {}


def differing(ha, hb):
    """the rays whose result on B is not their result on A"""
    return (ha.hit != hb.hit) | ((hb.hit != 0) & ((ha.prim != hb.prim) | (ha.t.view(np.uint32) != hb.t.view(np.uint32))))


def case_of(name):
    """(A, B as vertices, B as the statement sees it, the parked triangles, the rays, the statement on A, on B), computed once.
    The makers give vertices and triangles alone; the surfaces and the per-vertex normals are this module's."""
    if name not in _cache:
        A, B, tri = PAIRS[name][0]()
        rng = np.random.default_rng(41)
        a = U.Mesh(A, tri, surface=np.arange(tri.shape[0]) % 7, normals=rng.normal(size=A.shape))
        B = np.ascontiguousarray(B, F)
        gone = ~np.isfinite(B[a.tri.astype(np.int64)]).all(axis=(1, 2))
        b = without(a, B, gone) if gone.any() else moved(a, B)
        rays = U.copies_rays(a.nt) if name == "stacked" else rays_for(a, b, 448, 17)
        _cache[name] = (a, B, b, gone, rays, U.nearest_np(a, *rays), U.nearest_np(b, *rays))
    return _cache[name]


@pytest.mark.parametrize("leaf", [1, 4, 8])
@pytest.mark.parametrize("name", list(PAIRS))
def test_hostile_moves(ctx, name, leaf):
    from rlshaders_amd import nearest_refit
    a, B, b, gone, rays, ha, hb = case_of(name)
    o, d, m, skip = rays
    n = d.shape[1]
    # ---- the caps, on the reference alone
    assert gone.any() == (name == "non_finite") and np.isfinite(a.V).all()
    if name == "stacked":
        assert a.nt == 4097 and n == 9 and hb.hit.sum() == 7
        skips_1 = skip == 1
        assert skips_1.sum() == 1 and hb.hit[skips_1].all()
        assert (hb.prim[(hb.hit != 0) & ~skips_1] == 1).all() and (hb.prim[skips_1] == 2).all()
    else:
        assert n == 512
        assert differing(ha, hb).mean() >= 0.5, differing(ha, hb).mean()
        if name == "collapsed":
            assert hb.hit.sum() == 0
        else:
            assert hb.hit.mean() >= 0.5, hb.hit.mean()
    if name == "non_finite":
        assert a.nt == 320 and gone.sum() == 189
        assert not np.isin(hb.prim[hb.hit != 0], np.flatnonzero(gone)).any()
    want_last = np.where(hb.hit != 0, hb.prim, skip).astype(np.uint32)
    # ---- the device
    scene = device_scene(ctx, a, leaf)
    refit = nearest_refit.Refit(scene)
    boxes0, links0, prims0 = refit.read_tree()
    f0, before = found_bytes(ctx, scene, *rays)
    check_found(f0, ha, n, (name, leaf, "the untouched scene"), bin_table=BINS)
    parked = torch.full((1,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
    assert refit.update(_dev(B), parked=parked) is parked
    boxes, links, prims = refit.read_tree()
    assert np.array_equal(links, links0) and np.array_equal(prims, prims0), (name, leaf, "links or leaf order changed")
    assert np.isfinite(boxes).all() and np.array_equal(boxes, union_np(boxes, links, prims, B, a.tri)), (name, leaf, "boxes on B")
    assert int(parked.item()) == int(gone.sum()), (name, leaf, "parked")
    f1, after = found_bytes(ctx, scene, *rays)
    check_found(f1, hb, n, (name, leaf, "refit to B"), bin_table=BINS)
    assert np.array_equal(after[-1].view(np.uint32), want_last), (name, leaf, "last on B")
    hit, prim = _host(f1.hit), _host(f1.prim).view(np.uint32)
    if name == "collapsed":
        assert not hit.any()
    if name == "stacked":
        assert hit.sum() == 7 and (prim[(hit != 0) & (skip != 1)] == 1).all() and (prim[skip == 1] == 2).all()
    if not gone.any():
        fresh = device_scene(ctx, b, leaf)
        _, rebuilt = found_bytes(ctx, fresh, *rays)
        same(after, rebuilt, (name, leaf, "a fresh scene on B"))
        fresh.close()
    refit.update(_dev(a.V), parked=parked)
    assert int(parked.item()) == 0, (name, leaf, "parked after the update back")
    boxes1, links1, prims1 = refit.read_tree()
    assert np.array_equal(boxes1, boxes0) and np.array_equal(links1, links0) and np.array_equal(prims1, prims0), (name, leaf, "back on A")
    _, back = found_bytes(ctx, scene, *rays)
    same(back, before, (name, leaf, "back on A"))
    assert refit.info()["updates"] == 2
    refit.close(), scene.close()
