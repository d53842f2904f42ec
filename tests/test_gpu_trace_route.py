"""GPU: routing a queue's hits to the nodes (rls_trace_route_hits / _gather / _scatter / _fill, csrc_trace/rls_trace_route.hpp;
rlshaders_amd.trace.route_hits, HitRoutes).

  1. the partition against numpy (argsort(kind="stable"), bincount), exact: every size around the wavefront, the workgroup and
     the partition tile, 1 / 2 / 3 / 16 bins, nine bin mixes, every output inside sentinels, slot present and absent;
  2. gather, scatter and fill against numpy fancy indexing, as bits: 1 .. 24 word planes with 0 .. 8 byte planes, an index that
     is a strict sub-range of an order, every element written exactly once by the bins' scatters plus the fill, gather after
     scatter, dst == src refused;
  3. the consumer: a camera batch whose glossy queue's hits are shaded by two nodes and put back, routed by the library, gives the
     bytes the same calls give when torch indexing moves the data, in both math modes;
  4. graph replay;  5. one case past 2^31 rays."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import rlshaders_amd as R
import trace_route_util as U
from gpu_util import dev, host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    from rlshaders_amd import build, trace
    build.build_trace_library()
    trace.load()
    return trace


# ---- 1. the partition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [1, 2, 3, 16])
def test_the_partition_is_numpys_stable_argsort(gpu, T, bins):
    wrong = []
    for rays, name in itertools.product(U.SIZES, U.MIXES):
        b = U.mix(name, rays, bins)
        order, offsets, slot = U.raw_route(T, gpu, b, bins, slot=True)
        want = U.reference(b, bins)
        for what, got, ref in zip(("order", "offsets", "slot"), (order, offsets, slot), want):
            if not np.array_equal(got, ref):
                wrong.append((rays, name, what))
    assert not wrong, wrong[:20]


def test_without_slot_order_has_the_same_bytes(gpu, T):
    for rays, bins in ((3 * U.TILE + 5, 3), (U.KBLOCK + 1, 16), (1, 1)):
        b = U.mix("uniform", rays, bins, seed=1)
        with_slot = U.raw_route(T, gpu, b, bins, slot=True)
        order, offsets, _ = U.raw_route(T, gpu, b, bins, slot=False, scratch_extra=512)
        assert np.array_equal(order, with_slot[0]) and np.array_equal(offsets, with_slot[1])


def test_the_python_owner(gpu, T):
    rays, bins = 3 * U.TILE + 5, 3
    b = U.mix("uniform", rays, bins, seed=2)
    r = T.route_hits(gpu, dev(b), bins, slot=True)
    order, offsets, slot = U.reference(b, bins)
    assert r.bounds() == offsets.tolist() and r.sizes() == np.diff(offsets).tolist()
    assert np.array_equal(host(r.order).view(np.uint32), order) and np.array_equal(host(r.slot).view(np.uint32), slot)
    for k in range(bins + 1):
        assert np.array_equal(host(r.index(k)).view(np.uint32), order[offsets[k]:offsets[k + 1]])
    # written again without an allocation
    b2 = U.mix("rare", rays, bins, seed=3)
    assert T.route_hits(gpu, dev(b2), bins, routes=r) is r
    assert r.bounds() == U.reference(b2, bins)[1].tolist()
    with pytest.raises(ValueError):
        T.route_hits(gpu, dev(b2), bins + 1, routes=r)


# ---- 2. the movers --------------------------------------------------------------------------------------------------------------
R_POOL = 3 * U.TILE + 5 + 100


@pytest.fixture(scope="module")
def pool():
    """the per-ray planes every mover case reads: 24 word planes and 8 byte planes of R_POOL elements, and an order of R_POOL rays"""
    words = U.hostile_words(7, 24, R_POOL)
    octets = np.random.default_rng(8).integers(0, 256, (8, R_POOL), dtype=np.uint8)
    order = U.reference(U.mix("uniform", R_POOL, 3, seed=9), 3)[0]
    return dict(words=words, octets=octets, order=order, dwords=dev(words.view(np.int32)), doctets=dev(octets),
                dorder=dev(order.view(np.int32)))


def _raw_move(T, ctx, verb, m, index_ptr, src, dst):
    """one call over plane pointers: src / dst lists of (pointer, is_byte)"""
    p = T.RoutePlanes_()
    for (s, byte), (d, _) in zip(src, dst):
        if byte:
            p.src_u8[p.n_u8], p.dst_u8[p.n_u8] = s, d
            p.n_u8 += 1
        else:
            p.src_w32[p.n_w32], p.dst_w32[p.n_w32] = s, d
            p.n_w32 += 1
    st = getattr(T.load(), f"rls_trace_route_{verb}")(ctx.handle, m, index_ptr, C.byref(p))
    assert st == 0, (verb, m, st)


@pytest.mark.parametrize("nw,nb", list(itertools.product((1, 3, 12, 24), (0, 5, 8))))
def test_gather_and_scatter_are_numpys_fancy_indexing(gpu, T, pool, nw, nb):
    first = 11                                                           # the index: order[11, 11 + m), a strict sub-range
    for m in U.SIZES:
        index = pool["order"][first:first + m]
        iptr = pool["dorder"].data_ptr() + 4 * first
        rows = lambda t, k, byte: (t[k].data_ptr(), byte)
        src = [rows(pool["dwords"], k, False) for k in range(nw)] + [rows(pool["doctets"], k, True) for k in range(nb)]
        # gather: dst[j] = src[index[j]] into guarded planes of m elements
        gw = [U.Guarded(m, np.uint32) for _ in range(nw)]
        gb = [U.Guarded(m, np.uint8) for _ in range(nb)]
        _raw_move(T, gpu, "gather", m, iptr, src, [(g.ptr, False) for g in gw] + [(g.ptr, True) for g in gb])
        torch.cuda.synchronize()
        for k, g in enumerate(gw):
            assert np.array_equal(g.get(), pool["words"][k][index]), ("gather", m, k)
        for k, g in enumerate(gb):
            assert np.array_equal(g.get(), pool["octets"][k][index]), ("gather bytes", m, k)
        # scatter: dst[index[j]] = src[j] into guarded planes of R_POOL elements; every other element keeps the sentinel
        sw = [U.Guarded(R_POOL, np.uint32) for _ in range(nw)]
        sb = [U.Guarded(R_POOL, np.uint8) for _ in range(nb)]
        _raw_move(T, gpu, "scatter", m, iptr, src, [(g.ptr, False) for g in sw] + [(g.ptr, True) for g in sb])
        torch.cuda.synchronize()
        for k, g in enumerate(sw):
            want = np.full(R_POOL, U.FILL * 0x01010101, np.uint32)
            want[index] = pool["words"][k][:m]
            assert np.array_equal(g.get(), want), ("scatter", m, k)
        for k, g in enumerate(sb):
            want = np.full(R_POOL, U.FILL, np.uint8)
            want[index] = pool["octets"][k][:m]
            assert np.array_equal(g.get(), want), ("scatter bytes", m, k)


@pytest.mark.parametrize("planes", [1, 3, 24])
def test_fill_is_numpys_fancy_assignment(gpu, T, pool, planes):
    first = 11
    value = U.hostile_words(10, 1, planes)[0].view(np.float32)
    for m in U.SIZES:
        index = pool["order"][first:first + m]
        g = [U.Guarded(R_POOL, np.uint32) for _ in range(planes)]
        ptrs = (C.c_void_p * planes)(*[x.ptr for x in g])
        vals = (C.c_float * planes)()
        C.memmove(vals, value.ctypes.data, 4 * planes)                   # as bits: a float() round trip would quiet a NaN
        st = T.load().rls_trace_route_fill(gpu.handle, m, pool["dorder"].data_ptr() + 4 * first, planes, ptrs, vals)
        assert st == 0
        torch.cuda.synchronize()
        for k in range(planes):
            want = np.full(R_POOL, U.FILL * 0x01010101, np.uint32)
            want[index] = value.view(np.uint32)[k]
            assert np.array_equal(g[k].get(), want), (m, k)


def test_the_bins_scatters_and_the_fill_write_every_ray_once(gpu, T):
    rays, bins = 3 * U.TILE + 5, 3
    b = U.mix("uniform", rays, bins, seed=4)
    order, offsets, _ = U.reference(b, bins)
    r = T.route_hits(gpu, dev(b), bins)
    sentinel = np.uint32(0xFFC0A5A5)
    dst = dev(np.full((3, rays), sentinel, np.uint32).view(np.float32))
    want = np.empty((3, rays), np.uint32)
    env = (0.25, -0.0, float("inf"))
    srcs = []
    for k in range(bins):
        m = int(offsets[k + 1] - offsets[k])
        src = U.hostile_words(20 + k, 3, m)
        src[src == sentinel] = 0
        srcs.append(src)
        r.scatter(k, dev(src.view(np.float32)), dst)
        want[:, order[offsets[k]:offsets[k + 1]]] = src
    r.fill_misses(env, dst)
    want[:, order[offsets[bins]:]] = np.array(env, np.float32).view(np.uint32)[:, None]
    got = host(dst).view(np.uint32)
    assert not (got == sentinel).any() and np.array_equal(got, want)
    # gather after scatter is the identity, through the tensor interface: [3, rays] float32 beside 1-D int32 and uint8
    ids = np.arange(rays, dtype=np.int32) * 7
    for k in range(bins):
        back, gi, gb = r.gather(k, dst, dev(ids), dev(b))
        assert np.array_equal(host(back).view(np.uint32), srcs[k])
        assert np.array_equal(host(gi), ids[order[offsets[k]:offsets[k + 1]]]) and (host(gb) == k).all()
    # the state, five byte planes
    state = T.RayState(*[dev(np.random.default_rng(30 + p).integers(0, 256, rays, dtype=np.uint8)) for p in range(5)])
    sub = r.gather_state(1, state)
    for name in T.RayState.PLANES:
        assert np.array_equal(host(getattr(sub, name)), host(getattr(state, name))[order[offsets[1]:offsets[2]]])


def test_a_plane_moved_onto_itself_is_refused(gpu, T, pool):
    x = pool["dwords"][0]
    idx = pool["dorder"][:64]
    for move in (T.route_gather, T.route_scatter):
        with pytest.raises(Exception, match="a plane's dst is its src"):
            move(gpu, idx, [pool["dwords"][1], x], [torch.empty_like(x), x])


# ---- 3. the consumer ------------------------------------------------------------------------------------------------------------
def _seeded_bins(rays):
    return np.random.default_rng([11, rays]).choice(np.array([0, 1, 255], np.uint8), rays, p=[0.45, 0.35, 0.2])


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("n", [67, U.KBLOCK + 1])
def test_the_routed_bounce_is_the_torch_indexed_bounce(T, n, fast):
    ctx = R.Context(0)
    try:
        ctx.set_math_mode(fast)
        routed = U.two_bounces(ctx, n, 2, _seeded_bins, "route")
        indexed = U.two_bounces(ctx, n, 2, _seeded_bins, "torch")
    finally:
        ctx.close()
    assert routed["rays"] == indexed["rays"] > n and routed["sizes"] == indexed["sizes"] and min(routed["sizes"]) > 0
    assert sorted(routed) == sorted(indexed)
    for k, a in routed.items():
        if isinstance(a, np.ndarray):
            assert np.array_equal(a.view(np.uint32), indexed[k].view(np.uint32)), k
    # the children's radiance reached the camera batch: the indirect specular AOV is lit, and differs from the environment's alone
    assert (routed["indirect_specular"] > 0).mean() > 0.5 and (routed["out0"] > 0).any() and (routed["out1"] > 0).any()


# ---- 4. graph replay ------------------------------------------------------------------------------------------------------------
def test_route_gather_and_scatter_replay_in_a_graph(T):
    rays, bins = 3 * U.TILE + 5, 3
    b = U.mix("uniform", rays, bins, seed=5)
    order, offsets, slot = U.reference(b, bins)
    words = U.hostile_words(6, 3, rays)
    gctx = R.Context(0, use_torch_stream=False)          # the context's own stream: the NULL stream cannot be captured
    try:
        dbin, src = dev(b), dev(words.view(np.float32))
        r = T.HitRoutes(gctx, rays, bins, slot=True)
        m = int(offsets[2] - offsets[1])
        dense = torch.empty(3, m, dtype=torch.float32, device="cuda")
        back = torch.zeros(3, rays, dtype=torch.float32, device="cuda")
        index = r.order[int(offsets[1]):int(offsets[2])]          # bin 1's range, known from the host reference
        torch.cuda.synchronize()
        with gctx.capture() as g:
            r.route(dbin)
            T.route_gather(gctx, index, list(src), list(dense))
            T.route_scatter(gctx, index, list(dense), list(back))
        for t in (r.order, r.slot, r.offsets):
            t.fill_(-1)
        dense.fill_(float("nan"))
        torch.cuda.synchronize()
        g.launch()
        gctx.synchronize()
        g.close()
        assert np.array_equal(host(r.order).view(np.uint32), order) and np.array_equal(host(r.slot).view(np.uint32), slot)
        assert np.array_equal(host(r.offsets), offsets)
        at = order[offsets[1]:offsets[2]]
        assert np.array_equal(host(dense).view(np.uint32), words[:, at])
        want = np.zeros((3, rays), np.uint32)
        want[:, at] = words[:, at]
        assert np.array_equal(host(back).view(np.uint32), want)
    finally:
        gctx.close()


# ---- 5. past 2^31 rays ----------------------------------------------------------------------------------------------------------
def test_a_queue_of_more_than_2_to_the_31_rays(gpu, T):
    """rays = 2^31 + 2049, 3 bins, no slot, checked on the device in chunks of 2^26 over ALL of order: the keys of bin[order] never
    decrease, order ascends strictly within a key, and offsets is the device's count of every key -- together: order is the
    stable partition."""
    rays, bins, chunk = (1 << 31) + 2049, 3, 1 << 26
    free, _ = torch.cuda.mem_get_info()
    if free < 64 << 30:
        pytest.skip("needs 64 GB of free device memory")
    b = torch.randint(0, 4, (rays,), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(12))
    r = T.route_hits(gpu, b, bins)
    offsets = r.bounds()
    counts = torch.zeros(bins + 1, dtype=torch.int64, device="cuda")
    for a in range(0, rays, chunk):
        key = torch.clamp(b[a:a + chunk], max=bins)
        counts += torch.bincount(key.to(torch.int64), minlength=bins + 1)
    assert offsets == [0] + torch.cumsum(counts, 0).tolist() and offsets[-1] == rays
    ok = torch.ones((), dtype=torch.bool, device="cuda")
    last_key, last_ray = -1, -1
    for a in range(0, rays, chunk):
        o = r.order[a:a + chunk].to(torch.int64) & 0xFFFFFFFF
        key = torch.clamp(b[o], max=bins).to(torch.int64)
        same = key[1:] == key[:-1]
        ok &= (key[1:] >= key[:-1]).all() & (o[1:] > o[:-1])[same].all()
        first_key, first_ray = int(key[0]), int(o[0])
        assert first_key > last_key or (first_key == last_key and first_ray > last_ray)
        last_key, last_ray = int(key[-1]), int(o[-1])
    assert bool(ok)
