"""-m gpu: the rebuild's kernels (rlshaders_amd/csrc_nearest/rls_nearest_rebuild.hpp) at the edges of their tile loops.  Every one
of the nine is a loop of a workgroup over 256-element tiles, and four of them (the scan's reduce and apply, the sort's count and
scatter) reuse a __shared__ array from one iteration to the next.  On a context capped at one workgroup per CU
(RLS_BLOCKS_PER_CU=1) a mesh of 2.5 x compute_units x 256 + 77 triangles gives init, mark, partition, leaf and the records two
and a half rounds, the sort (three lists a launch) seven and a half, the scan more than one run of its single workgroup, and a
partial last tile; the default context runs every one of these launches in ONE round, so its tree is a second, independent
answer.  The reference throughout is the host builder's tree of a fresh nearest.Scene on the moved vertices, read through a
nearest_refit.Refit(fresh).read_tree() that is never updated: links and triangle order exactly, boxes by value.

On the random soup and on the flat grid (whole rows of equal keys across tiles and rounds: the tie-break by id is the sort's
stability between tiles of different rounds) at leaf 1 and 4; a second update in the same stream with nothing synchronised
between the two; a few thousand rays on the capped rebuild == a fresh scene's bytes; the parked count, one atomic a tile round,
over hostile vertices.  And, on the default context: lists that end on a wavefront edge inside a tile or leave whole wavefronts
of the only tile empty (63 .. 193 triangles), and the leaf sizes 2, 5, 6 and 7 of the leaf kernel's 8-wide sorting network."""
import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_util as U
from nearest_util import NO_PRIM
from nearest_rebuild_util import PAIRS, TILE, hostile_pair, parked_of, same_tree
from nearest_refit_util import twisted, without
from test_gpu_nearest import _dev
from test_gpu_nearest_rebuild import both_entry_points, fresh_tree, rebuilt_tree, scene_on

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from rlshaders_amd import nearest, nearest_rebuild, nearest_refit
    nearest.load(), nearest_refit.load(), nearest_rebuild.load()     # (a missing library is an error, not a build)
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


class Big:
    """the mesh pairs of `nt` triangles and the builder's trees on them, each made once: tree(name, leaf, "A" | "B" | "C"),
    C = B twisted by 2 rad"""

    def __init__(self, ctx, nt):
        self.ctx, self.nt, self._pairs, self._trees = ctx, nt, {}, {}

    def pair(self, name):
        if name not in self._pairs:
            A, B, tri = PAIRS[name](self.nt)
            assert tri.shape[0] == self.nt
            self._pairs[name] = dict(A=A, B=B, C=twisted(B, 2.0), tri=tri)
        return self._pairs[name]

    def tree(self, name, leaf, which):
        if (name, leaf, which) not in self._trees:
            p = self.pair(name)
            self._trees[name, leaf, which] = fresh_tree(self.ctx, p[which], p["tri"], leaf)
        return self._trees[name, leaf, which]


@pytest.fixture(scope="module")
def big(ctx, one_block_per_cu):
    cu = one_block_per_cu.device_info()["compute_units"]
    grid = (cu + 7) // 8 * 8
    nt = 5 * cu * TILE // 2 + 77
    tiles = -(-nt // TILE)
    assert nt % TILE != 0
    assert nt / TILE / grid >= 2.2                                   # init, mark, partition, leaf, records: two and a half rounds
    assert 3 * tiles / grid >= 7                                     # the sort: seven and a half
    assert 3 * nt > TILE * TILE                                      # the scan's tile sums: more than one run of the one workgroup
    assert 3 * tiles <= 64 * grid                                    # the default context: every launch in one round
    return Big(ctx, nt)


def aimed_rays(B, tri, seed):
    """about 3000 rays at points inside triangles of the moved mesh, the first and the last 100 triangles among them"""
    rng = np.random.default_rng(seed)
    nt = tri.shape[0]
    ends = np.concatenate([np.arange(100), np.arange(nt - 100, nt)])
    targets = np.concatenate([U.interior_targets(rng, U.Mesh(B, tri), 2800, margin=0.0),
                              np.einsum("kv,kvc->kc", rng.dirichlet((1, 1, 1), ends.size), B.astype(np.float64)[tri[ends].astype(np.int64)])])
    return U.rays_at_targets(rng, targets, spread=2.0)


@pytest.mark.parametrize("leaf", [1, 4])
@pytest.mark.parametrize("name", ["random", "flat"])
def test_grid_rounds_give_the_builders_tree(ctx, one_block_per_cu, big, name, leaf):
    from rlshaders_amd import nearest_rebuild
    capped_ctx = one_block_per_cu
    p = big.pair(name)
    A, B, Cv, tri = p["A"], p["B"], p["C"], p["tri"]
    want = big.tree(name, leaf, "B")
    # a rebuild that does nothing cannot pass: the tree on A is another one
    assert same_tree(big.tree(name, leaf, "A"), want) is not None, (name, leaf)
    capped, plain = scene_on(ctx, A, tri, leaf), scene_on(ctx, A, tri, leaf)
    rc, rp = nearest_rebuild.Rebuild(capped), nearest_rebuild.Rebuild(plain)
    parked = torch.full((2,), 3, dtype=torch.int64, device="cuda")
    rc.update(_dev(B), parked=parked[:1], ctx=capped_ctx)
    rp.update(_dev(B), parked=parked[1:])
    in_rounds, in_one = rc.read_tree(ctx=capped_ctx), rp.read_tree()
    assert same_tree(in_rounds, want) is None, (name, leaf, "one workgroup per CU", same_tree(in_rounds, want))
    assert same_tree(in_one, want) is None, (name, leaf, "the default context", same_tree(in_one, want))
    for x, y in zip(in_rounds, in_one):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (name, leaf, "the two contexts' trees differ")
    assert parked.tolist() == [0, 0]
    if (name, leaf) == ("random", 4):
        # queries on the tree made in rounds: every found plane and `last`, of both entry points, are a fresh scene's bytes
        o, d = aimed_rays(B, tri, 3)
        none = np.full(d.shape[1], NO_PRIM, np.uint32)
        fresh = scene_on(ctx, B, tri, leaf)
        got, ref = both_entry_points(ctx, capped, o, d, none), both_entry_points(ctx, fresh, o, d, none)
        fresh.close()
        assert (ref[0] != 0).mean() > 0.9                             # the rays are aimed at the moved mesh
        for k, (x, y) in enumerate(zip(got, ref)):
            assert np.array_equal(x, y), (name, leaf, k)
    # two updates in the same stream, nothing synchronised between them: the working set (counts, sums, flag, node_at, both
    # list arrays) is what the first left, and the second starts from id order all the same
    vb, vc = _dev(B), _dev(Cv)
    torch.cuda.synchronize()
    rc.update(vb, ctx=capped_ctx)
    rc.update(vc, ctx=capped_ctx)
    again = rc.read_tree(ctx=capped_ctx)
    assert same_tree(again, big.tree(name, leaf, "C")) is None, (name, leaf, "second update", same_tree(again, big.tree(name, leaf, "C")))
    assert same_tree(again, want) is not None and rc.info()["updates"] == 3
    rc.close(), rp.close(), capped.close(), plain.close()


def test_parked_count_over_grid_rounds(ctx, one_block_per_cu, big):
    """refit_records_kernel adds to *parked once a tile round: a non-zero count over two and a half rounds"""
    from rlshaders_amd import nearest_rebuild
    nt, leaf = big.nt, 4
    A, B, tri = hostile_pair(nt)
    assert np.array_equal(A, big.pair("random")["A"])                 # the way back is the random pair's tree on A
    gone = parked_of(B, tri)
    rest = without(U.Mesh(A, tri), B, gone)
    scene = scene_on(ctx, A, tri, leaf)
    rb = nearest_rebuild.Rebuild(scene)
    parked = torch.full((1,), -9, dtype=torch.int64, device="cuda")
    rb.update(_dev(B), parked=parked, ctx=one_block_per_cu)
    assert int(parked.item()) == int(gone.sum()) and 0 < gone.sum() < nt
    got, want = rb.read_tree(ctx=one_block_per_cu), fresh_tree(ctx, rest.V, rest.tri, leaf)
    assert np.isfinite(got[0]).all() and same_tree(got, want) is None, same_tree(got, want)
    rb.update(_dev(A), parked=parked, ctx=one_block_per_cu)
    back = rb.read_tree(ctx=one_block_per_cu)
    assert int(parked.item()) == 0 and same_tree(back, big.tree("random", leaf, "A")) is None
    rb.close(), scene.close()


# ---- small trees on the default context ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [1, 8])
@pytest.mark.parametrize("name", ["flat", "identical", "random"])
def test_the_lists_end_on_a_wavefront_edge(ctx, name, leaf):
    """rebuild_wave_rank ranks by ballots of 64 lanes under an `inside` mask: a list that ends one lane before, on and one lane
    past each wavefront edge inside the only tile -- one, two and three wavefronts of the tile are then empty or hold one lane"""
    for nt in (63, 64, 65, 127, 128, 129, 191, 192, 193):
        A, B, tri = PAIRS[name](nt)
        got, want = rebuilt_tree(ctx, A, B, tri, leaf), fresh_tree(ctx, B, tri, leaf)
        assert same_tree(got, want) is None, (name, leaf, nt, same_tree(got, want))


@pytest.mark.parametrize("leaf", [2, 5, 6, 7])
def test_every_leaf_size(ctx, leaf):
    """rebuild_leaf sorts 8 registers padded with 0xFFFFFFFF whatever the leaf holds: leaves of 2, 5, 6 and 7 ids (and, at
    nt = 1000, of the counts the halving leaves under each)"""
    for name in ("random", "identical"):
        for nt in (leaf, leaf + 1, 2 * leaf + 1, 1000):
            A, B, tri = PAIRS[name](nt)
            got, want = rebuilt_tree(ctx, A, B, tri, leaf), fresh_tree(ctx, B, tri, leaf)
            assert same_tree(got, want) is None, (name, leaf, nt, same_tree(got, want))
            if nt > leaf:
                assert same_tree(fresh_tree(ctx, A, tri, leaf), want) is not None, (name, leaf, nt)
