"""-m gpu: the grid and stack edges of the group query (librls_nearest_group.so), as test_gpu_nearest_edges.py has them for one mesh.
  A. two and a half grid rounds on a context capped at one workgroup per CU (RLS_BLOCKS_PER_CU=1) and a last tile of ONE ray: the
     default context's bytes, and group_np's on windows about the round boundaries and the tail;
  B. the deepest top tree, 2^16 one-triangle instances on a line at top leaf 1 (17 levels), queried once: a wavefront in which
     lane 37 alone crosses every instance's box without hitting a triangle (it opens all 131071 top nodes) among 63 lanes that miss
     the root; a wavefront of 64 identical stack-filling rays (the ray along the line holds 16 top entries on its way to instance 0);
     the rays of the CPU test.  Every result equals the CPU program's (tests/native/nearest_group_host_check.cpp: the same
     traversal source, held to its brute force there), and the stack-filling ray's is instance 0 at t = 1;
  C. both stacks live in one lane: three exact translations of the deep grid (23 levels at leaf 1) under its stack-filling stream,
     where a ray fills the object rows of the kernel's stack array while it holds entries in the top rows."""
import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_group_host_util as H
import nearest_group_util as G
import nearest_util as U
from nearest_group_util import group_rays, line_rays, skips
from nearest_util import F
from test_gpu_nearest import _host
from test_gpu_nearest_group import SCALAR, VEC, DeviceGroup, all_bytes, mesh_of, query

pytestmark = pytest.mark.gpu
TILE = 256
DEEP_BOTH = 106                                                      # rays at 22 object entries while a top entry is held
DEEP_HITS = 394


@pytest.fixture(scope="module")
def gpu_ctx():
    from rlshaders_amd import nearest_group
    nearest_group.load()
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


def test_two_and_a_half_grid_rounds_and_a_last_tile_of_one_ray(gpu_ctx, one_block_per_cu):
    cu = one_block_per_cu.device_info()["compute_units"]
    grid = (cu + 7) // 8 * 8                                        # the workgroups of a capped launch
    n = 2 * grid * TILE + grid * TILE // 2 + 1                      # the last tile holds one ray
    assert n % TILE == 1 and n / TILE / grid >= 2.4
    insts = G.general_instances(mesh_of("icosphere"), 5, seed=91)
    bo, bd, bm = group_rays(insts, 4096 - 64, 41)
    bs = skips(np.random.default_rng(42), G.group_np(insts, bo, bd, bm))
    reps = -(-n // 4096)
    o, d = np.tile(bo, (1, reps))[:, :n].copy(), np.tile(bd, (1, reps))[:, :n].copy()
    m, skip = np.tile(bm, reps)[:n].copy(), (np.tile(bs[0], reps)[:n].copy(), np.tile(bs[1], reps)[:n].copy())
    o += (np.arange(n, dtype=F) * F(1e-6))[None, :]                 # no two rays alike
    g = DeviceGroup(gpu_ctx, insts)
    try:
        a, la, ja = query(gpu_ctx, g.group, o, d, m, skip)
        b, lb, jb = query(gpu_ctx, g.group, o, d, m, skip, use_ctx=one_block_per_cu)
        for x, y in zip(all_bytes(a) + [_host(la), _host(ja)], all_bytes(b) + [_host(lb), _host(jb)]):
            assert np.array_equal(x, y)
        hits = _host(b.hit)
        assert 0.3 < hits.mean() < 0.98
        for lo in [max(k * grid * TILE - 256, 0) for k in (1, 2)] + [n - 512]:
            hi = min(lo + 512, n)
            h = G.group_np(insts, o[:, lo:hi], d[:, lo:hi], m[lo:hi], (skip[0][lo:hi], skip[1][lo:hi]))
            assert np.array_equal(hits[lo:hi], h.hit), lo
            sel = h.hit != 0
            for name in ("t",) + VEC + SCALAR:
                got = _host(getattr(b, name))[..., lo:hi][..., sel]
                want = getattr(h, name)[..., sel]
                assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (lo, name)
            assert np.array_equal(_host(lb).view(np.uint32)[lo:hi], np.where(sel, h.prim, skip[1][lo:hi])), lo
            assert np.array_equal(_host(jb).view(np.uint32)[lo:hi], np.where(sel, h.instance, skip[0][lo:hi])), lo
    finally:
        g.close()


def test_the_deepest_top_tree_once(gpu_ctx, tmp_path):
    n = G.MAX_INSTANCES
    insts = G.line_instances(n)
    lo, ld, want = line_rays(n)
    miss_o, miss_d = np.array([-1.0, 50.0, 0.0], F), np.array([1.0, 0.0, 0.0], F)       # misses the root box
    o, d = np.tile(miss_o[:, None], (1, 64)), np.tile(miss_d[:, None], (1, 64))
    o[:, 37], d[:, 37] = (-1.0, 0.9, 0.9), (1.0, 0.0, 0.0)           # inside every instance's box, outside every triangle
    o = np.concatenate([o, np.tile(lo[:, :1], (1, 64)), lo], axis=1)
    d = np.concatenate([d, np.tile(ld[:, :1], (1, 64)), ld], axis=1)
    g = DeviceGroup(gpu_ctx, insts, leaf=1, scene_leaf=1)
    try:
        info = g.group.info()
        assert info["top_depth"] == 17 and info["top_nodes"] == 2 * n - 1 and info["scenes"] == 1
        f, _, _ = query(gpu_ctx, g.group, o, d)
    finally:
        g.close()
    r = H.run(H.build(tmp_path), H.write_group(tmp_path / "line.bin", insts), o, d, top_leaf=1, scene_leaf=1)
    assert r.differ == 0 and r.ray_max_top[64] == 16 and r.ray_top_nodes[37] == 2 * n - 1 and r.entered[37] == n
    hit = _host(f.hit) != 0
    assert np.array_equal(hit, r.hit) and not hit[:64].any() and hit[64:128].all()
    assert np.array_equal(_host(f.instance).view(np.uint32)[hit], r.tree_instance[hit])
    assert np.array_equal(_host(f.prim).view(np.uint32)[hit], r.tree_prim[hit])
    assert np.array_equal(_host(f.t).view(np.uint32)[hit], r.tree_t.view(np.uint32)[hit])
    assert (_host(f.instance)[64:128] == 0).all() and (_host(f.t)[64:128] == 1.0).all()
    assert np.array_equal(_host(f.instance).view(np.uint32)[128:][hit[128:]], want[hit[128:]]) and np.array_equal(hit[128:], want != G.NO_INSTANCE)
    assert np.array_equal(_host(f.surface).view(np.uint32)[hit], r.tree_instance[hit] + 1)      # base j + the mesh's surface id 1


def deep_three():
    """three exact translations of the deep grid (2^21 + 20 triangles; 23 levels and an object stack of 22 at leaf 1) and its
    577-ray stack-filling stream, ray k mapped to the world of instance k % 3 and skipping its triangle there"""
    mesh = U.deep_grid()
    shifts = ((-1.25, 0.5, 0.0), (1.0, -0.25, 0.75), (0.25, 1.5, -0.5))
    insts = [G.Inst(mesh, G.affine(t=t), G.affine(t=[-x for x in t]), base=5000 * j) for j, t in enumerate(shifts)]
    o, d, m, skip, _ = U.deep_stream(mesh)
    j = np.arange(d.shape[1]) % len(insts)
    o = (o + np.array(shifts, F)[j].T).astype(F)
    return mesh, insts, o, d, m, (np.where(skip == U.NO_PRIM, G.NO_INSTANCE, j).astype(np.uint32), skip)


def test_both_stacks_live_in_one_lane(gpu_ctx, tmp_path):
    """The kernel keeps a lane's top stack in rows 0 .. 15 of one LDS array and its object stack in rows 16 .. 39.  Over one-triangle
    scenes the object rows stay empty; here a corner ray holds a top entry (the sibling of the instance it is in) while it fills
    all 22 object entries its tree has use for, and must find that top entry again afterwards.  Expected: the CPU program's brute
    force over the statement; the device equals it bit for bit on every ray."""
    mesh, insts, o, d, m, skip = deep_three()
    r = H.run(H.build(tmp_path), H.write_group(tmp_path / "deep.bin", insts), o, d, m, skip, top_leaf=1, scene_leaf=1)
    both = (r.ray_max_stack == 22) & (r.ray_max_top >= 1)
    print("rays at full object stack holding a top entry:", int(both.sum()), "max_top", r.max_top, "hits", r.hits)
    assert r.differ == 0 and r.depth == 3 and r.max_stack == 22 and both.sum() == DEEP_BOTH and r.hits == DEEP_HITS
    assert 0.2 < r.hit.mean() < 0.98
    g = DeviceGroup(gpu_ctx, insts, leaf=1, scene_leaf=1)
    try:
        f, last, last_instance = query(gpu_ctx, g.group, o, d, m, skip)
    finally:
        g.close()
    hit = _host(f.hit) != 0
    assert np.array_equal(hit, r.hit)
    assert np.array_equal(_host(f.instance).view(np.uint32)[hit], r.instance[hit])
    assert np.array_equal(_host(f.prim).view(np.uint32)[hit], r.prim[hit])
    assert np.array_equal(_host(f.t).view(np.uint32)[hit], r.t.view(np.uint32)[hit])
    base = np.array([i.base for i in insts], np.uint32)
    assert np.array_equal(_host(f.surface).view(np.uint32)[hit], base[r.instance[hit]] + mesh.surface[r.prim[hit]])
    assert np.array_equal(_host(last_instance).view(np.uint32), np.where(hit, r.instance, skip[0]))
    assert np.array_equal(_host(last).view(np.uint32), np.where(hit, r.prim, skip[1]))

