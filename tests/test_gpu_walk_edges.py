"""-m gpu: the probe walk's kernels (rlshaders_amd/csrc_walk/rls_walk_device.hpp) at the edges of their loops.

  A. two and a half grid rounds of walk_begin_kernel, walk_step_kernel and walk_place_kernel on a context capped at one workgroup
     per CU (RLS_BLOCKS_PER_CU=1), the list ending in a tile of ONE ray: the default context's bytes, and the statement's
     (tests/walk_util.py, walk_np) on every entry -- the windows at the round boundaries and the tail among them;
  B. the tile counts across 2 and 4 tiles of the scan (trace_scan_*: 2048 counts a tile, each the survivors of 256 entries), the
     add-back carrying the earlier tiles' sums, again with a last tile of one ray."""
import numpy as np
import pytest
import torch

import rlshaders_amd as R
from test_gpu_walk import TILE, _dev, _host, assert_same_hits, assert_same_list, device_found, moved, unit
from walk_util import Found, walk_np

pytestmark = pytest.mark.gpu

SCAN_TILE = 2048                             # kScanTile


@pytest.fixture(scope="module")
def gpu_ctx():
    from rlshaders_amd import build
    build.build_trace_library()
    build.build_walk_library()
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def one_block_per_cu():
    """a context whose grids are capped at one workgroup per CU (RLS_BLOCKS_PER_CU, read at context creation):
    tests/test_gpu_loop_edges.py"""
    mp = pytest.MonkeyPatch()
    mp.setenv("RLS_BLOCKS_PER_CU", "1")
    try:
        ctx = R.Context(0)
    finally:
        mp.undo()
    yield ctx
    ctx.close()


def contents(n, seed):
    g = np.random.default_rng(seed)
    P = g.standard_normal((3, n)).astype(np.float32)
    d = g.standard_normal((3, n)).astype(np.float32)
    md = g.uniform(0.5, 2.0, n).astype(np.float32)
    md[g.random(n) < 0.1] = 0.0                                     # some rays never listed
    return P, (P + np.float32(0.01) * d).astype(np.float32), d, md


def queue_of(ctx, P, o, d, md):
    from rlshaders_amd import trace
    q = trace.ProbeQueue(ctx, P.shape[1], 1)
    q.origin.copy_(_dev(o)); q.dir.copy_(_dev(d)); q.maxdist.copy_(_dev(md))
    return q


def stream(step, wn, rng):
    """about two thirds of the listed rays hit, most hits accepted"""
    m = wn.active
    return Found(rng.random(m) < 0.67, rng.uniform(0.02, 0.1, m), moved(wn, rng), unit(rng, m), unit(rng, m))


def walk_on(contexts, n, steps, seed):
    """the same walk on every context and in the statement, each step compared; the contexts' buffers byte for byte"""
    from rlshaders_amd import walk
    P, o, d, md = contents(n, seed)
    zeros = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")       # (the statement's untouched slots are 0)
    ws = [walk.ProbeWalk(c, queue_of(c, P, o, d, md), _dev(P), max_hits=4, alloc=zeros) for c in contexts]
    wn = walk_np(o, d, md, P, 1, max_hits=4)
    rng = np.random.default_rng(seed + 1)
    counts = []
    for w in ws:
        assert_same_list(w, wn, (n, "begin"))
    for step in range(steps):
        counts.append(wn.active)
        f = stream(step, wn, rng)
        fd = device_found(f)
        for w in ws:
            w.step(fd, bound=wn.active)
        wn.step(f)
        for w in ws:
            assert_same_list(w, wn, (n, "step", step))
    for w in ws:
        assert_same_hits(w, wn, n)
    for w in ws[1:]:
        m = wn.active
        for a, b in ((w.hit_count, ws[0].hit_count), (w.hit_P, ws[0].hit_P), (w.hit_N, ws[0].hit_N),
                     (w.rays.ray[:m], ws[0].rays.ray[:m]), (w.rays.maxdist[:m].view(torch.int32), ws[0].rays.maxdist[:m].view(torch.int32))):
            assert torch.equal(a, b)
    return counts + [wn.active]


def test_two_and_a_half_grid_rounds_and_a_last_tile_of_one_ray(gpu_ctx, one_block_per_cu):
    cu = one_block_per_cu.device_info()["compute_units"]
    n = 2 * cu * TILE + cu * TILE // 2 + 1
    assert n % TILE == 1 and n / TILE / ((cu + 7) // 8 * 8) >= 2.4
    counts = walk_on([gpu_ctx, one_block_per_cu], n, 3, 31)
    print("walk grid rounds:", dict(cu=cu, n=n, active=counts))
    assert counts[0] > 0.85 * n and counts[-1] > 0.1 * n            # every step's list spans more than one round's tiles x 0.1


@pytest.mark.parametrize("scan_tiles", [2, 4])
def test_tile_counts_across_scan_tiles(gpu_ctx, scan_tiles):
    tiles = (scan_tiles - 1) * SCAN_TILE * 115 // 100 + 5           # (a tenth of the rays is never listed)
    n = (tiles - 1) * TILE + 1
    assert -(-tiles // SCAN_TILE) == scan_tiles
    counts = walk_on([gpu_ctx], n, 2, 37 + scan_tiles)
    # the first step's list still needs `scan_tiles` tiles of the scan, so both the begin's and a step's scan carry across them
    assert -(-(-(-counts[0] // TILE)) // SCAN_TILE) == scan_tiles, counts
