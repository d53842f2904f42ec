"""-m gpu: the refit's kernels (rlshaders_amd/csrc_nearest/rls_nearest_refit.hpp) at the edges of their tile loops: on a context
capped at one workgroup per CU (RLS_BLOCKS_PER_CU=1) a grid mesh of 2.5 x compute_units x 256 + 77 triangles -- two and a half
rounds of the record kernel and of the widest levels, a partial last tile -- at leaf 1 and leaf 4 gives the bytes of the default
context and of a fresh scene, on a few thousand rays aimed at the moved mesh; `surface` and `bin` are intact (the update writes
nothing outside the records and the boxes); a second update in the same stream, nothing synchronised between the two, lands."""
import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_util as U
from nearest_util import F
from nearest_refit_util import levels_np, union_np
from test_gpu_nearest import SCALAR, VEC, _bytes, _dev, _host, query

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

