"""-m gpu: nearest_kernel (rlshaders_amd/csrc_nearest/rls_nearest_device.hpp) at the edges of its loops.

  A. two and a half grid rounds on a context capped at one workgroup per CU (RLS_BLOCKS_PER_CU=1) and a last tile of ONE ray:
     the default context's bytes in every plane, and the numpy statement (tests/nearest_util.py) on the 512-ray windows at the
     round boundaries and at the end;
  B. a wavefront in which one lane alone walks the tree -- a ray in the plane of a flat quad grid from corner to corner, through
     the boxes of every node on its diagonal, its node count taken from the host run of the same traversal source -- among 63
     rays that miss the root box;
  C. a wavefront of 64 identical rays."""
import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_util as U
from nearest_util import F
from test_gpu_nearest import VEC, SCALAR, _bytes, _dev, _host, check_found, mesh_of, mixed_rays, query

pytestmark = pytest.mark.gpu

TILE = 256


@pytest.fixture(scope="module")
def gpu_ctx():
    from rlshaders_amd import nearest
    nearest.load()
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def one_block_per_cu():
    """a context whose grids are capped at one workgroup per CU (RLS_BLOCKS_PER_CU, read at context creation)"""
    mp = pytest.MonkeyPatch()
    mp.setenv("RLS_BLOCKS_PER_CU", "1")
    try:
        ctx = R.Context(0)
    finally:
        mp.undo()
    yield ctx
    ctx.close()


def scene(ctx, name):
    from rlshaders_amd import nearest
    m = mesh_of(name)
    return nearest.Scene(ctx, m.V, m.tri, surface=m.surface, normals=m.normals)


def test_two_and_a_half_grid_rounds_and_a_last_tile_of_one_ray(gpu_ctx, one_block_per_cu):
    cu = one_block_per_cu.device_info()["compute_units"]
    grid = (cu + 7) // 8 * 8                                        # the workgroups of a capped launch
    n = 2 * grid * TILE + grid * TILE // 2 + 1                      # the last tile holds one ray
    assert n % TILE == 1 and n / TILE / grid >= 2.4
    mesh = mesh_of("icosphere")
    base = mixed_rays(mesh, 4096, 41)
    reps = -(-n // 4096)
    o, d = np.tile(base[0], (1, reps))[:, :n].copy(), np.tile(base[1], (1, reps))[:, :n].copy()
    m, skip = np.tile(base[2], reps)[:n].copy(), np.tile(base[3], reps)[:n].copy()
    o += (np.arange(n, dtype=F) * F(1e-6))[None, :]                 # no two rays alike
    s = scene(gpu_ctx, "icosphere")
    a, la, _ = query(gpu_ctx, s, o, d, m, skip)
    b, lb, _ = query(gpu_ctx, s, o, d, m, skip, use_ctx=one_block_per_cu)
    for x, y in zip(_bytes(a) + [_host(la)], _bytes(b) + [_host(lb)]):
        assert np.array_equal(x, y)
    hits = _host(b.hit)
    assert 0.3 < hits.mean() < 0.95
    for lo in [max(k * grid * TILE - 256, 0) for k in (1, 2)] + [n - 512]:
        hi = min(lo + 512, n)
        h = U.nearest_np(mesh, o[:, lo:hi], d[:, lo:hi], m[lo:hi], skip[lo:hi])
        w = hi - lo
        assert np.array_equal(hits[lo:hi], h.hit), lo
        sel = h.hit != 0
        for name in ("t",) + VEC + SCALAR:
            got = _host(getattr(b, name))[..., lo:hi][..., sel]
            want = getattr(h, name)[..., sel]
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (lo, name)
        assert np.array_equal(_host(lb).view(np.uint32)[lo:hi], np.where(sel, h.prim, skip[lo:hi])), (lo, w)
    s.close()


def test_one_lane_walks_the_tree_among_misses(gpu_ctx):
    """63 lanes miss the root box and stop at the first node; lane 37's ray lies IN the plane of a flat 33 x 33 grid, along its
    diagonal: parallel to every triangle (det = 0, no hit ever, so nothing is culled by a best t) and inside the boxes of the 33
    quads on the diagonal.  A leaf holds at most 4 triangles, two quads, so the ray opens at least 17 leaves, and a binary tree's
    17 leaves have at least 16 inner nodes above them: at least 33 nodes, counted by the kernel's traversal source on the host
    (nearest.host_stats)."""
    from rlshaders_amd import nearest
    mesh = U.quad_grid(33, flat=True)
    n, lane = 64, 37
    o = np.tile(np.array([[0.0], [0.0], [5.0]], F), (1, n))
    d = np.tile(np.array([[0.0], [0.0], [1.0]], F), (1, n))         # away from the grid: the root box fails
    o[:2, :] += (np.arange(n, dtype=F) * F(0.01))[None, :]
    o[:, lane] = (-1.25, -1.25, 0.0)
    d[:, lane] = (1.0, 1.0, 0.0)
    h = U.nearest_np(mesh, o, d)
    assert not h.hit.any()
    st = np.array(nearest.host_stats(mesh.V, mesh.tri, o, d, per_ray=True)["per_ray"])
    others = np.arange(n) != lane
    assert (st[others, 2] == 1).all() and (st[others, 3] == 0).all(), st[others][:4]
    assert st[lane, 2] >= 33 and st[lane, 3] >= 66, st[lane]
    print("one lane:", dict(nodes=int(st[lane, 2]), triangles=int(st[lane, 3])))
    s = nearest.Scene(gpu_ctx, mesh.V, mesh.tri, surface=mesh.surface)
    f, _, _ = query(gpu_ctx, s, o, d)
    check_found(f, h, n, "one lane")
    # the complement: the diagonal ray on every lane but two -- one that stops at the root, and one lifted a hair and aimed
    # down, which meets the plane near the far corner: a hit among lanes that walk the tree and find nothing
    o2, d2 = np.tile(o[:, lane:lane + 1], (1, n)), np.tile(d[:, lane:lane + 1], (1, n))
    o2[:, 5], d2[:, 5] = o[:, 0], d[:, 0]
    o2[2, 9], d2[2, 9] = F(0.002), F(-0.001)
    h2 = U.nearest_np(mesh, o2, d2)
    assert h2.hit[9] == 1 and h2.hit.sum() == 1 and h2.P[0, 9] > 0.7
    f2, _, _ = query(gpu_ctx, s, o2, d2)
    check_found(f2, h2, n, "one lane idle")
    s.close()


def test_a_wavefront_of_identical_rays(gpu_ctx):
    mesh = mesh_of("soup")
    rng = np.random.default_rng(43)
    o1, d1 = U.rays_at_targets(rng, U.interior_targets(rng, mesh, 1), spread=2.0)
    for n in (64, 256 + 64):
        o, d = np.tile(o1, (1, n)), np.tile(d1, (1, n))
        h = U.nearest_np(mesh, o, d)
        assert h.hit.all() and len(set(h.prim)) == 1
        s = scene(gpu_ctx, "soup")
        f, _, _ = query(gpu_ctx, s, o, d)
        check_found(f, h, n, ("identical", n))
        s.close()
