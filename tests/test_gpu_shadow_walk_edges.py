"""-m gpu: the shadow walk's kernels (rlshaders_amd/csrc_shadow_walk/rls_shadow_walk_device.hpp) at the edges of their loops.

  A. two and a half grid rounds of shadow_begin_kernel, shadow_step_kernel and shadow_place_kernel on a context capped at one
     workgroup per CU (RLS_BLOCKS_PER_CU=1), at 2.5 x compute_units x 256 + 77 rays: the default context's bytes, and the
     statement's (tests/shadow_walk_util.py, shadow_walk_np) on every entry -- the 512-ray windows at the round boundaries among
     them, named one by one;
  B. a last tile of ONE ray;
  C. the tile counts across 2 and 4 tiles of the scan (trace_scan_*: 2048 counts a tile, each the survivors of 256 entries), the
     add-back carrying the earlier tiles' sums."""
import numpy as np
import pytest
import torch

import rlshaders_amd as R
from shadow_walk_util import F, Found, shadow_walk_np
from test_gpu_shadow_walk import TILE, _dev, _host, assert_same_state, device_found, raw_queue

pytestmark = pytest.mark.gpu

SCAN_TILE = 2048                             # kScanTile


@pytest.fixture(scope="module")
def gpu_ctx():
    from rlshaders_amd import build
    build.build_trace_library()
    build.build_shadow_walk_library()
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
    points = max(n // 3, 1)
    O = g.standard_normal((3, points)).astype(F)
    point = g.integers(0, points, n).astype(np.int32)
    d = g.standard_normal((3, n)).astype(F)
    md = g.uniform(0.5, 2.0, n).astype(F)
    md[g.random(n) < 0.1] = 0.0                                     # some rays never listed
    base = (g.random((3, n), F) + F(0.25)).astype(F)
    return O, point, d, md, base


def stream(wn, rng):
    """about four fifths of the listed rays hit; one hit in six is opaque"""
    m = wn.active
    o = rng.random((3, m), F)
    o[:, rng.random(m) < 1 / 6] = 1.0
    P = rng.standard_normal((3, m)).astype(F)
    return Found(rng.random(m) < 0.8, rng.uniform(0.02, 0.2, m), P, o)


def walk_on(contexts, n, steps, seed, windows=()):
    """the same walk on every context and in the statement, each step compared; the contexts' buffers byte for byte"""
    from rlshaders_amd import shadow_walk
    O, point, d, md, base = contents(n, seed)
    zeros = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    ws = [shadow_walk.ShadowWalk(c, raw_queue(d, md, point), _dev(O), base=_dev(base), max_steps=steps + 1, alloc=zeros)
          for c in contexts]
    wn = shadow_walk_np(O, point, d, md, steps + 1, base=base)
    rng = np.random.default_rng(seed + 1)
    counts = []

    def compare(what):
        for w in ws:
            assert_same_state(w, wn, (n, what))
            T, r = _host(w.visibility), w.rays
            for lo in windows:                                      # the windows at the round boundaries, by name
                hi = min(lo + 512, n)
                assert np.array_equal(T[:, lo:hi].view(np.uint32), wn.T[:, lo:hi].view(np.uint32)), (what, "T window", lo)
                hi = min(lo + 512, wn.active)
                if lo < hi:
                    assert np.array_equal(_host(r.ray[lo:hi]).view(np.uint32), wn.ray[lo:hi]), (what, "list window", lo)

    compare("begin")
    for step in range(steps):
        counts.append(wn.active)
        f = stream(wn, rng)
        fd = device_found(f)
        for w in ws:
            w.step(fd, bound=wn.active)
        wn.step(f)
        compare(("step", step))
    for w in ws[1:]:
        m = wn.active
        for a, b in ((w.visibility.view(torch.int32), ws[0].visibility.view(torch.int32)), (w.rays.ray[:m], ws[0].rays.ray[:m]),
                     (w.rays.trials[:m], ws[0].rays.trials[:m]),
                     (w.rays.origin[:, :m].view(torch.int32), ws[0].rays.origin[:, :m].view(torch.int32)),
                     (w.rays.maxdist[:m].view(torch.int32), ws[0].rays.maxdist[:m].view(torch.int32))):
            assert torch.equal(a, b)
    return counts + [wn.active]


def test_two_and_a_half_grid_rounds(gpu_ctx, one_block_per_cu):
    cu = one_block_per_cu.device_info()["compute_units"]
    n = 2 * cu * TILE + cu * TILE // 2 + 77
    grid = (cu + 7) // 8 * 8                                        # the workgroups of a capped launch
    assert n / TILE / grid >= 2.4
    windows = [max(k * grid * TILE - 256, 0) for k in (1, 2)] + [max(n - 512, 0)]
    counts = walk_on([gpu_ctx, one_block_per_cu], n, 3, 31, windows)
    print("shadow walk grid rounds:", dict(cu=cu, n=n, active=counts))
    assert counts[0] > 0.85 * n and counts[-1] > 0.1 * n            # every step's list spans more than one round's tiles x 0.1


def test_last_tile_of_one_ray(gpu_ctx, one_block_per_cu):
    n = 5 * TILE + 1
    counts = walk_on([gpu_ctx, one_block_per_cu], n, 2, 33, [n - 1])
    assert counts[0] > 0.85 * n
    # and a list whose last tile holds one entry: every ray listed, then 4 * TILE + 1 survivors
    from rlshaders_amd import shadow_walk
    O, point, d, md, _ = contents(n, 34)
    md[:] = 1.0
    w = shadow_walk.ShadowWalk(gpu_ctx, raw_queue(d, md, point), _dev(O), max_steps=3)
    wn = shadow_walk_np(O, point, d, md, 3)
    assert w.active == n
    hit = np.zeros(n, np.uint8)
    hit[np.r_[0:4 * TILE, n - 1]] = 1
    f = Found(hit, np.full(n, 0.25, F), np.zeros((3, n), F), np.full((3, n), 0.5, F))
    w.step(device_found(f), bound=n)
    wn.step(f)
    assert wn.active == 4 * TILE + 1 and wn.ray[-1] == n - 1
    assert_same_state(w, wn, "one entry in the last tile")


@pytest.mark.parametrize("scan_tiles", [2, 4])
def test_tile_counts_across_scan_tiles(gpu_ctx, scan_tiles):
    tiles = (scan_tiles - 1) * SCAN_TILE * 115 // 100 + 5           # (a tenth of the rays is never listed)
    n = (tiles - 1) * TILE + 1
    assert -(-tiles // SCAN_TILE) == scan_tiles
    counts = walk_on([gpu_ctx], n, 2, 37 + scan_tiles)
    # the first step's list still needs `scan_tiles` tiles of the scan, so both the begin's and a step's scan carry across them
    assert -(-(-(-counts[0] // TILE)) // SCAN_TILE) == scan_tiles, counts
