"""GPU: the routing kernels (csrc_trace/rls_trace_route.hpp) past one round of their loops and past one scan tile, on a context
capped at one workgroup per CU (tests/test_gpu_trace_node_edges.py, one_block_per_cu) and on the default context, both held to
numpy:
  * two and a half grid rounds of route_count_kernel / route_place_kernel (2.5 x compute_units tiles) and of the three movers
    (2.5 x compute_units x kBlock elements);
  * with 16 bins the bin-major count array of 17 x tiles cells crosses 2 and 4 scan tiles (17 x tiles > 2048 and > 8192), so the
    scan's add-back carries across them; rays at those tile counts - 1, + 0, + 1: a last tile short of one ray, full, a single ray."""
import numpy as np
import pytest
import torch

import trace_route_util as U
from gpu_util import dev, host
from test_gpu_trace_node_edges import one_block_per_cu  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    from rlshaders_amd import build, trace
    build.build_trace_library()
    trace.load()
    return trace


def _routed(T, ctx, b, bins):
    r = T.route_hits(ctx, dev(b), bins, slot=True)
    return host(r.order).view(np.uint32), host(r.offsets), host(r.slot).view(np.uint32)


def test_the_partition_over_several_grid_rounds(gpu, one_block_per_cu, T):
    cu = gpu.device_info()["compute_units"]
    rays, bins = (5 * cu // 2) * U.TILE + 5, 3
    b = U.mix("uniform", rays, bins, seed=40)
    want = U.reference(b, bins)
    for ctx in (one_block_per_cu, gpu):
        for got, ref in zip(_routed(T, ctx, b, bins), want):
            assert np.array_equal(got, ref)


@pytest.mark.parametrize("cells", [2048, 8192])
def test_the_count_matrix_across_scan_tiles(gpu, one_block_per_cu, T, cells):
    bins = 16
    tiles = cells // (bins + 1) + 1
    assert (bins + 1) * tiles > cells and (bins + 1) * (tiles - 1) <= cells
    for rays in (tiles * U.TILE - 1, tiles * U.TILE, tiles * U.TILE + 1):
        for name in ("uniform", "every_second_tile"):
            b = U.mix(name, rays, bins, seed=41)
            want = U.reference(b, bins)
            for ctx in (one_block_per_cu, gpu):
                for what, got, ref in zip(("order", "offsets", "slot"), _routed(T, ctx, b, bins), want):
                    assert np.array_equal(got, ref), (rays, name, what)


def test_the_movers_over_several_grid_rounds(gpu, one_block_per_cu, T):
    cu = gpu.device_info()["compute_units"]
    m = 5 * cu * U.KBLOCK // 2 + 37
    rays = m + 1000
    index = np.sort(np.random.default_rng(42).choice(rays, m, replace=False)).astype(np.uint32)      # ascending, as a bin's
    words, octets = U.hostile_words(43, 3, rays), np.random.default_rng(44).integers(0, 256, (2, rays), dtype=np.uint8)
    value = (0.5, -0.0, 3.0)
    got = []
    for ctx in (one_block_per_cu, gpu):
        didx, dw, do = dev(index.view(np.int32)), dev(words.view(np.int32)), dev(octets)
        gw, go = torch.empty(3, m, dtype=torch.int32, device="cuda"), torch.empty(2, m, dtype=torch.uint8, device="cuda")
        T.route_gather(ctx, didx, list(dw) + list(do), list(gw) + list(go))
        sw, so = torch.full((3, rays), -1, dtype=torch.int32, device="cuda"), torch.full((2, rays), 255, dtype=torch.uint8, device="cuda")
        T.route_scatter(ctx, didx, list(gw) + list(go), list(sw) + list(so))
        fill = torch.full((3, rays), float("nan"), dtype=torch.float32, device="cuda")
        T.route_fill(ctx, didx, value, list(fill))
        got.append([host(t) for t in (gw, go, sw, so, fill)])
    want_sw = np.full((3, rays), 0xFFFFFFFF, np.uint32)
    want_sw[:, index] = words[:, index]
    want_so = np.full((2, rays), 255, np.uint8)
    want_so[:, index] = octets[:, index]
    want_fill = np.full((3, rays), np.float32("nan")).view(np.uint32)
    want_fill[:, index] = np.array(value, np.float32).view(np.uint32)[:, None]
    for g in got:
        assert np.array_equal(g[0].view(np.uint32), words[:, index]) and np.array_equal(g[1], octets[:, index])
        assert np.array_equal(g[2].view(np.uint32), want_sw) and np.array_equal(g[3], want_so)
        assert np.array_equal(g[4].view(np.uint32), want_fill)
