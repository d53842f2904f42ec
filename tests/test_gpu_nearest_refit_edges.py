"""-m gpu: the refit's kernels (rlshaders_amd/csrc_nearest/rls_nearest_refit.hpp) at the edges of their tile loops: on a context
capped at one workgroup per CU (RLS_BLOCKS_PER_CU=1) a grid mesh of 2.5 x compute_units x 256 + 77 triangles -- two and a half
rounds of the record kernel and of the widest levels, a partial last tile -- at leaf 1 and leaf 4 gives the bytes of the default
context and of a fresh scene, on a few thousand rays aimed at the moved mesh; `surface` and `bin` are intact (the update writes
nothing outside the records and the boxes); a second update in the same stream, nothing synchronised between the two, lands.

Both launch plans of the update (refit.hip): a refit made under RLS_NEAREST_REFIT_FOLD=0 launches refit_level_kernel once per
level up to the root, one made with the variable unset hands the top of the tree to refit_top_kernel.  On the trees of
nearest_refit_util.PLAN_TREES -- level sizes asserted from the links read back -- the two give the same read tree == the numpy
union and the same query bytes == nearest_np, after an update and after the update back."""
import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_util as U
from nearest_util import F
from nearest_refit_util import PLAN_GRIDS, PLAN_TREES, levels_fast, levels_np, moved, profile_np, squashed, union_fast, union_np
from test_gpu_nearest import SCALAR, VEC, _bytes, _dev, _host, check_found, query

pytestmark = pytest.mark.gpu

TILE = 256
NAMES = ("hit", "t") + VEC + SCALAR + ("bin",)
BINS = np.array([4, 1, 0, 9, 2], np.uint8)


@pytest.fixture(scope="module")
def gpu_ctx():
    from rlshaders_amd import nearest, nearest_refit
    nearest.load(), nearest_refit.load()
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


def strip(nt):
    """a bumped strip of quads two rows high, nt triangles (the last quad gives one triangle where nt is odd); surface = quad % 5"""
    cols = (nt + 3) // 4
    x = np.linspace(-1.0, 1.0, cols + 1)
    V = np.array([(xi, -1.0 + j, 0.1 * np.sin(7.0 * xi) * (j - 1)) for j in range(3) for xi in x], np.float64)
    tri, S = [], []
    for j in range(2):
        for i in range(cols):
            a = j * (cols + 1) + i
            tri += [(a, a + 1, a + cols + 2), (a, a + cols + 2, a + cols + 1)]
            S += [(j * cols + i) % 5] * 2
    return U.Mesh(V, np.array(tri[:nt], np.uint32), surface=np.array(S[:nt], np.uint32))


def wave(V, phase):
    V = np.asarray(V, np.float64).copy()
    V[:, 2] += 0.3 * np.sin(5.0 * V[:, 0] + phase) * np.cos(2.0 * V[:, 1])
    V[:, 1] *= 1.0 + 0.2 * np.sin(phase)
    return V.astype(F)


@pytest.fixture(scope="module")
def setting(one_block_per_cu):
    cu = one_block_per_cu.device_info()["compute_units"]
    nt = 5 * cu * TILE // 2 + 77
    grid = (cu + 7) // 8 * 8
    assert nt % TILE and nt / TILE / grid >= 2.2
    a = strip(nt)
    assert a.nt == nt
    B, C = wave(a.V, 0.7), wave(a.V, 2.1)
    rng = np.random.default_rng(3)
    rays = []
    for V in (B, C):
        m = U.Mesh(V, a.tri)
        # targets over the whole strip, the first and the last triangles (the last tile) among them
        k = np.concatenate([rng.integers(0, nt, 2800), np.arange(100), np.arange(nt - 100, nt)])
        bary = rng.dirichlet((1, 1, 1), k.size)
        targets = np.einsum("kv,kvc->kc", bary, m.V.astype(np.float64)[m.tri[k].astype(np.int64)])
        rays.append(U.rays_at_targets(rng, targets, spread=1.5))
    return a, B, C, rays


def found(ctx, scene, o, d, use_ctx=None):
    f, _, _ = query(ctx, scene, o, d, bin_table=BINS, use_ctx=use_ctx)
    return _bytes(f, NAMES)


@pytest.mark.parametrize("leaf", [1, 4])
def test_two_and_a_half_rounds_and_a_partial_last_tile(gpu_ctx, one_block_per_cu, setting, leaf):
    from rlshaders_amd import nearest, nearest_refit
    a, B, C, rays = setting
    make = lambda V: nearest.Scene(gpu_ctx, V, a.tri, surface=a.surface, leaf_size=leaf)
    capped, plain, fresh_b, fresh_c = make(a.V), make(a.V), make(B), make(C)
    rc, rp = nearest_refit.Refit(capped), nearest_refit.Refit(plain)
    boxes0, links0, prims0 = rc.read_tree()
    widest = np.bincount(levels_np(links0)).max()
    cu = one_block_per_cu.device_info()["compute_units"]
    # the levels walk the capped grid in rounds too: the widest level fills two rounds at leaf 1 and one at leaf 4, and the
    # levels next to it end in partial rounds and tiles
    assert widest >= (2 if leaf == 1 else 1) * ((cu + 7) // 8 * 8) * TILE
    parked = torch.full((1,), 3, dtype=torch.int64, device="cuda")
    rc.update(_dev(B), parked=parked, ctx=one_block_per_cu)
    rp.update(_dev(B))
    o, d = rays[0]
    got, want, rebuilt = found(gpu_ctx, capped, o, d), found(gpu_ctx, plain, o, d), found(gpu_ctx, fresh_b, o, d)
    assert got[0].mean() > 0.9                                     # the rays are aimed at the moved mesh
    for name, x, y, z in zip(NAMES, got, want, rebuilt):
        assert np.array_equal(x, y) and np.array_equal(x, z), (leaf, name)
    assert int(parked.item()) == 0
    boxes, links, prims = rc.read_tree(ctx=one_block_per_cu)
    assert np.array_equal(links, links0) and np.array_equal(prims, prims0)
    assert np.array_equal(boxes, union_np(boxes, links, prims, B, a.tri))
    # two updates in the same stream, nothing synchronised between them: the second one's mesh is what the queries see
    vb, vc = _dev(B), _dev(C)
    torch.cuda.synchronize()
    rc.update(vb, ctx=one_block_per_cu)
    rc.update(vc, ctx=one_block_per_cu)
    o, d = rays[1]
    got, rebuilt = found(gpu_ctx, capped, o, d, use_ctx=one_block_per_cu), found(gpu_ctx, fresh_c, o, d)
    for name, x, z in zip(NAMES, got, rebuilt):
        assert np.array_equal(x, z), (leaf, name, "second update")
    assert got[0].mean() > 0.9
    for r in (rc, rp):
        r.close()
    for s in (capped, plain, fresh_b, fresh_c):
        s.close()



# ---- both launch plans -----------------------------------------------------------------------------------------------------------------
def refit_under(scene, fold):
    """a refit created with RLS_NEAREST_REFIT_FOLD set to `fold`, or unset (None): the variable is read at creation"""
    from rlshaders_amd import nearest_refit
    mp = pytest.MonkeyPatch()
    if fold is None:
        mp.delenv("RLS_NEAREST_REFIT_FOLD", raising=False)
    else:
        mp.setenv("RLS_NEAREST_REFIT_FOLD", fold)
    try:
        return nearest_refit.Refit(scene)
    finally:
        mp.undo()


@pytest.mark.parametrize("nt,leaf", [(nt, 1) for nt in PLAN_TREES] + [(0, leaf) for leaf in PLAN_GRIDS])
def test_both_launch_plans(gpu_ctx, nt, leaf):
    """nt = 0: U.quad_grid(33).  The level sizes each tree was chosen for (PLAN_TREES) are the builder's, on the device as in
    the CPU test of the host program's tree: no nt had to be changed."""
    from rlshaders_amd import nearest
    from test_gpu_nearest_refit import rays_for
    a = U.soup(nt) if nt else U.quad_grid(33)
    b = moved(a, squashed(a, 3))
    rays = rays_for(a, b, 96, 1000 + nt)
    ha, hb = U.nearest_np(a, *rays), U.nearest_np(b, *rays)
    n = rays[1].shape[1]
    # (triangle 0 of a soup is degenerate: of 1 triangle next to nothing hits, of 2 a fifth of the rays)
    assert hb.hit.mean() >= (0.0 if nt == 1 else 0.1 if nt == 2 else 0.25), hb.hit.mean()
    make = lambda: nearest.Scene(gpu_ctx, a.V, a.tri, surface=a.surface, normals=a.normals, leaf_size=leaf)
    level_scene, top_scene = make(), make()
    by_level, by_top = refit_under(level_scene, "0"), refit_under(top_scene, None)
    boxes0, links0, prims0 = by_level.read_tree()
    assert profile_np(links0) == (PLAN_TREES[nt] if nt else PLAN_GRIDS[leaf])
    assert np.array_equal(levels_fast(links0), levels_np(links0))
    assert np.array_equal(boxes0, union_np(boxes0, links0, prims0, a.V, a.tri))

    def bytes_of(scene, h, what):
        f, last, _ = query(gpu_ctx, scene, *rays, bin_table=BINS)
        check_found(f, h, n, (nt, leaf, what), bin_table=BINS)
        return _bytes(f, NAMES) + [_host(last)]

    for V, h, what in ((b.V, hb, "updated"), (a.V, ha, "back")):
        parked = torch.full((2,), 77, dtype=torch.int64, device="cuda")
        by_level.update(_dev(V), parked=parked[:1])
        by_top.update(_dev(V), parked=parked[1:])
        trees = by_level.read_tree(), by_top.read_tree()
        for x, y in zip(*trees):
            assert np.array_equal(x, y), (nt, leaf, what, "the two plans' trees differ")
        boxes, links, prims = trees[0]
        assert np.array_equal(links, links0) and np.array_equal(prims, prims0)
        want = union_np(boxes, links, prims, V, a.tri)
        assert np.array_equal(boxes, want) and np.array_equal(union_fast(boxes, links, prims, V, a.tri), want), (nt, leaf, what)
        assert _host(parked).tolist() == [0, 0]
        for x, y in zip(bytes_of(level_scene, h, what + ", a launch a level"), bytes_of(top_scene, h, what + ", the top folded")):
            assert np.array_equal(x, y), (nt, leaf, what, "the two plans' bytes differ")
    assert np.array_equal(boxes, boxes0)
    by_level.close(), by_top.close(), level_scene.close(), top_scene.close()
