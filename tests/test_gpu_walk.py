"""-m gpu: rlSss's probe walk on the device (include/rlshaders_amd_walk.h, rlshaders_amd/walk.py).

1. Every step = the statement (tests/walk_util.py, walk_np) bit for bit -- the device count, ray, origin, dir, maxdist, trials and
   the hits -- on the plane and the sphere under a nearest-hit tracer, at ray counts around a wavefront and the place kernel's
   tile (kBlock = 256 entries, one per lane), every plane and the exact-size scratch inside sentinel-filled buffers.
2. Synthetic streams of nearest hits, one rule of the walk each.
3. End to end: the walk over a cumulative tracer, resolved by rls_trace_sss_scatter_resolve, IS rls_sss_integrate_scatter.
4. A whole walk recorded into a graph and replayed on fresh hits.
5. The walk's hits through the other hand-offs: the rlSkin node's probes (rls_trace_skin_resolve = rls_skin_integrate) and
   rls_trace_sss_hits_emit / _resolve."""
import inspect

import numpy as np
import pytest
import torch

import cases
import oracle_lib as O
from test_walk_statement import SEED, list_without_duplicates, setting
from trace_sss_util import EPS, light_irradiance, same_bits_or_both_nan, trace_queue
from walk_util import TRIALS, Found, cumulative_tracer, length_np, nearest_tracer, walk_np

pytestmark = pytest.mark.gpu

TILE = 256                                  # kWalkTile = kBlock
SENTINEL = 0xA5
FILL = np.frombuffer(bytes([SENTINEL] * 4), np.float32)[0]
GUARD = 512                                 # bytes of sentinel either side of every buffer


@pytest.fixture(scope="module")
def ctx():
    import rlshaders_amd as R
    from rlshaders_amd import build
    build.build_trace_library()
    build.build_walk_library()
    c = R.Context(0)
    yield c
    c.close()


def _host(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """an allocator for walk.ProbeWalk: every tensor an inner view of a sentinel-filled buffer"""

    def __init__(self):
        self.outer = []

    def __call__(self, shape, dtype):
        size = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        inner = (size + 255) // 256 * 256                          # (the views stay 256-byte aligned)
        buf = torch.full((GUARD + inner + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.outer.append((buf, size))
        return buf[GUARD:GUARD + size].view(dtype).view(shape)

    def check(self):
        for buf, size in self.outer:
            b = _host(buf)
            assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + size:] == SENTINEL).all(), size


def sampler(ctx, case):
    import rlshaders_amd as R
    return R.SssSampler(ctx, _dev(case["N"]), _dev(case["T"]), _dev(case["albedo"]), _dev(case["dist"]), has_dPdu=True)


def device_found(f, object=None):
    from rlshaders_amd import walk
    return walk.Found(_dev(f.hit), _dev(f.t), _dev(f.P), _dev(f.N), _dev(f.Ns), None if f.object is None else _dev(f.object))


def assert_same_list(w, wn, what):
    """the device's active list = the statement's, bit for bit"""
    m = w.active
    assert m == wn.active, (what, "active", m, wn.active)
    r = w.rays
    np.testing.assert_array_equal(_host(r.ray)[:m].view(np.uint32), wn.ray, str(what))
    np.testing.assert_array_equal(_host(r.trials)[:m], wn.trials, str(what))
    same_bits_or_both_nan(_host(r.origin)[:, :m], wn.origin, (what, "origin"))
    same_bits_or_both_nan(_host(r.dir)[:, :m], wn.dir, (what, "dir"))
    same_bits_or_both_nan(_host(r.maxdist)[:m], wn.maxdist, (what, "maxdist"))


def assert_same_hits(w, wn, what):
    """count, P, N = the statement's; the slots at or beyond count[j] untouched (wn was made with the buffers' fill)"""
    np.testing.assert_array_equal(_host(w.hit_count), wn.count, str(what))
    same_bits_or_both_nan(_host(w.hit_P), wn.hP, (what, "hits.P"))
    same_bits_or_both_nan(_host(w.hit_N), wn.hN, (what, "hits.N"))


def host_queue(q):
    return _host(q.origin), _host(q.dir), _host(q.maxdist)


def walk_both(ctx, q, P, tracer, max_hits=12, own=None, foreign="stop", steps=TRIALS, what="", point=None):
    """the device's walk and the statement's side by side over one host tracer, compared after begin and after every step
    -> (the device walk, the statement, the active count before every step)"""
    from rlshaders_amd import walk
    alloc = Guarded()
    w = walk.ProbeWalk(ctx, q, _dev(P), own=None if own is None else _dev(own), max_hits=max_hits, foreign=foreign, alloc=alloc,
                       point=None if point is None else _dev(point.astype(np.int32)))
    origin, dirs, maxdist = host_queue(q)
    wn = walk_np(origin, dirs, maxdist, P, q.spp_n * q.spp_n, own=own, max_hits=max_hits, foreign=foreign, fill=FILL, point=point)
    assert_same_list(w, wn, (what, "begin"))
    counts = []
    for step in range(steps):
        if wn.active == 0:
            break
        counts.append(wn.active)
        # a function is a synthetic stream (step, statement) -> Found; an object a scene tracer over the listed rays
        f = tracer(step, wn) if inspect.isfunction(tracer) else tracer(wn.ray, wn.origin, wn.dir, wn.maxdist)
        w.step(device_found(f), bound=wn.active)
        wn.step(f)
        assert_same_list(w, wn, (what, "step", step))
    assert_same_hits(w, wn, what)
    alloc.check()
    return w, wn, counts


# ---- 1. every step = the statement, on the analytic scenes -----------------------------------------------------------------------
@pytest.mark.parametrize("max_hits", [1, 2, 12])
@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_every_step_is_the_statement(ctx, kind, n, max_hits):
    from rlshaders_amd import trace
    case, scene = setting(kind, n)
    q = trace.sss_probe_rays(sampler(ctx, case), _dev(case["P"]), 1, SEED)
    _, wn, counts = walk_both(ctx, q, case["P"], nearest_tracer(scene), max_hits=max_hits, what=(kind, n, max_hits))
    assert wn.active == 0 and counts and counts[0] == int((_host(q.maxdist) > 0).sum())
    assert int(wn.count.max()) <= max_hits


# ---- 2. synthetic streams ---------------------------------------------------------------------------------------------------------
def synthetic_queue(ctx, n, rng, maxdist=None):
    """a probe queue of n rays (spp_n = 1) with random contents -> (queue, P [3, n])"""
    from rlshaders_amd import trace
    q = trace.ProbeQueue(ctx, n, 1)
    P = rng.standard_normal((3, n)).astype(np.float32)
    d = rng.standard_normal((3, n)).astype(np.float32)
    q.origin.copy_(_dev(P + np.float32(0.01) * d))
    q.dir.copy_(_dev(d))
    q.maxdist.copy_(_dev(rng.uniform(0.5, 2.0, n).astype(np.float32) if maxdist is None else maxdist))
    return q, P


def prev_of(wn):
    """the last accepted position of every listed ray"""
    j, c = wn.ray.astype(np.int64), wn.count[wn.ray.astype(np.int64)].astype(np.int64)
    return np.where(c > 0, wn.hP[:, np.maximum(c - 1, 0), j], wn.P0[:, j]).astype(np.float32)


def moved(wn, rng, by=0.5):
    """hit positions well away from prev"""
    m = wn.active
    return (prev_of(wn) + np.float32(by) * (1 + rng.random((3, m))).astype(np.float32)).astype(np.float32)


def unit(rng, m):
    v = rng.standard_normal((3, m))
    return (v / np.linalg.norm(v, axis=0)).astype(np.float32)


def test_rehits_within_epsilon_retire_after_twelve_steps(ctx):
    rng = np.random.default_rng(1)
    n = 3 * 64 + 7
    q, P = synthetic_queue(ctx, n, rng)

    def gen(step, wn):
        m = wn.active
        near = (prev_of(wn) + np.float32(2e-5) * unit(rng, m)).astype(np.float32)
        return Found(np.ones(m), rng.uniform(0, 0.01, m), near, unit(rng, m), unit(rng, m))
    _, wn, counts = walk_both(ctx, q, P, gen)
    assert counts == [n] * TRIALS and wn.active == 0 and not wn.count.any()


def test_distance_one_ulp_either_side_of_epsilon(ctx):
    rng = np.random.default_rng(2)
    n = 130
    q, _ = synthetic_queue(ctx, n, rng)
    P = np.zeros((3, n), np.float32)
    ulps = (np.arange(n) % 9 - 4).astype(np.int32)
    d = (np.full(n, EPS, np.float32).view(np.int32) + ulps).view(np.float32)

    def gen(step, wn):
        m = wn.active
        hp = np.zeros((3, m), np.float32)
        hp[step % 3] = d[wn.ray] * (1 if step % 2 == 0 else -1)
        return Found(np.ones(m), np.full(m, 0.01), hp, unit(rng, m), unit(rng, m))
    _, wn, _ = walk_both(ctx, q, P, gen, steps=1)
    dist = length_np(np.stack([d, 0 * d, 0 * d]))
    assert (dist == EPS).any() and (dist == np.nextafter(EPS, np.float32(1))).any() and (dist == np.nextafter(EPS, np.float32(0))).any()
    np.testing.assert_array_equal(wn.count, (dist > EPS).astype(np.uint8))


@pytest.mark.parametrize("case", ["t", "left", "normals"])
def test_special_values(ctx, case):
    """t = 0, negative, inf, NaN; left landing exactly on 0, going negative, NaN; N . Ns negative, 0, NaN"""
    rng = np.random.default_rng(3)
    n = 200
    q, P = synthetic_queue(ctx, n, rng, maxdist=np.ones(n, np.float32))
    ts = dict(t=[0.0, -0.25, np.inf, np.nan, -np.inf, 0.125], left=[1.0, 2.0, np.nan, 0.5, 0.25, 0.75])

    def gen(step, wn):
        m = wn.active
        N = unit(rng, m)
        t = rng.uniform(0.01, 0.05, m).astype(np.float32)
        Ns = N.copy()
        if case == "normals":
            kind = wn.ray % 5
            Ns[:, kind == 1] *= -1
            Ns[:, kind == 2] = np.cross(N.T, unit(rng, m).T).T[:, kind == 2]
            Ns[0, kind == 3] = np.nan
            N[1, kind == 4] = np.nan
            Ns[:, wn.ray % 7 == 0] = 0.0
        else:
            t = np.asarray(ts[case], np.float32)[(wn.ray + step) % 6]
        return Found(np.ones(m), t, moved(wn, rng), N, Ns)
    _, wn, counts = walk_both(ctx, q, P, gen, steps=4)
    assert len(counts) >= 2
    if case == "normals":
        assert np.isnan(wn.hN[:, 0]).any() and int(wn.count.min()) >= 1


@pytest.mark.parametrize("own", ["ids", "none"])
@pytest.mark.parametrize("foreign", ["stop", "skip"])
def test_foreign_policies(ctx, foreign, own):
    rng = np.random.default_rng(4)
    n = TILE + 40
    q, P = synthetic_queue(ctx, n, rng)
    ids = None if own == "none" else rng.integers(0, 3, n).astype(np.int32)

    def gen(step, wn):
        m = wn.active
        obj = None if ids is None else rng.integers(0, 3, m).astype(np.int32)
        return Found(rng.random(m) < 0.9, rng.uniform(0.01, 0.1, m), moved(wn, rng), unit(rng, m), unit(rng, m), object=obj)
    _, wn, counts = walk_both(ctx, q, P, gen, own=ids, foreign=foreign)
    assert len(counts) >= 3
    if ids is not None and foreign == "skip":
        assert len(counts) == TRIALS                               # a skipped hit costs a trial and nothing else


def test_rays_mapped_to_points_by_a_point_plane(ctx):
    """rls_walk.point: ray j belongs to point point[j], not j / spp -- the walk starts at that point's P and tests that point's
    object.  Half the first hits lie within epsilon of the mapped point: with the wrong point they would be accepted."""
    rng = np.random.default_rng(8)
    n = 300
    q, P = synthetic_queue(ctx, n, rng)
    point = rng.permutation(n)
    ids = rng.integers(0, 2, n).astype(np.int32)

    def gen(step, wn):
        m = wn.active
        near = (prev_of(wn) + np.float32(2e-5) * unit(rng, m)).astype(np.float32)
        hp = np.where(rng.random(m) < 0.5, near, moved(wn, rng)).astype(np.float32)
        return Found(np.ones(m), rng.uniform(0.01, 0.1, m), hp, unit(rng, m), unit(rng, m), object=rng.integers(0, 2, m).astype(np.int32))
    _, wn, counts = walk_both(ctx, q, P, gen, own=ids, foreign="skip", steps=3, point=point)
    assert len(counts) == 3 and 0.2 * n < int((wn.count > 0).sum()) < n


@pytest.mark.parametrize("keep", ["none", "all", "last_lane"])
def test_a_step_where_none_all_or_one_lane_a_wavefront_survives(ctx, keep):
    rng = np.random.default_rng(5)
    n = 2 * TILE + 64
    q, P = synthetic_queue(ctx, n, rng)

    def gen(step, wn):
        m = wn.active
        hit = np.ones(m) if keep == "all" else np.zeros(m) if keep == "none" else (np.arange(m) % 64 == 63)
        return Found(hit, np.full(m, 0.01), moved(wn, rng), unit(rng, m), unit(rng, m))
    _, wn, counts = walk_both(ctx, q, P, gen, steps=2)
    assert counts == dict(none=[n], all=[n, n], last_lane=[n, n // 64])[keep]


def test_empty_queue_and_inactive_rays(ctx):
    from rlshaders_amd import trace, walk
    rng = np.random.default_rng(6)
    q = trace.ProbeQueue(ctx, 0, 1)
    w = walk.ProbeWalk(ctx, q, torch.empty(3, 0, device="cuda"))
    assert w.active == 0
    n = 70
    md = rng.uniform(0.5, 2.0, n).astype(np.float32)
    md[::3], md[1::7], md[5] = 0.0, np.nan, -1.0
    q, P = synthetic_queue(ctx, n, rng, maxdist=md)
    _, wn, counts = walk_both(ctx, q, P, lambda step, wn: Found(np.zeros(wn.active), np.zeros(wn.active), moved(wn, rng),
                                                                 unit(rng, wn.active), unit(rng, wn.active)))
    assert counts == [int((md > 0).sum())]


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------
def walked_hits(ctx, q, case, scene, spp_n, max_hits=TRIALS):
    """the device's walk over the cumulative tracer, held to the statement at every step and to orc_scene_trace's list without
    its within-epsilon hits for EVERY ray -> (count, P, N, E) on the device"""
    origin, dirs, maxdist = host_queue(q)
    w, wn, counts = walk_both(ctx, q, case["P"], cumulative_tracer(scene, origin, dirs, maxdist), max_hits=max_hits)
    assert wn.active == 0 and len(counts) <= 3
    cnt, hP, hN = trace_queue(scene, origin, dirs, maxdist)
    P0 = case["P"][:, np.arange(len(maxdist)) // (spp_n * spp_n)]
    want_c, want_P, want_N = list_without_duplicates(P0, cnt, hP, hN, max_hits)
    np.testing.assert_array_equal(wn.count, want_c)
    live = np.arange(max_hits)[:, None] < want_c[None, :]
    assert np.array_equal(wn.hP.view(np.uint32)[:, live], want_P.view(np.uint32)[:, live])
    assert np.array_equal(wn.hN.view(np.uint32)[:, live], want_N.view(np.uint32)[:, live])
    hP, hN = np.where(live, _host(w.hit_P), np.float32(0)), np.where(live, _host(w.hit_N), np.float32(0))
    return w.hit_count, _dev(hP), _dev(hN), _dev(light_irradiance(scene, hP, hN))


def scene_pair(kind, n, **kw):
    import rlshaders_amd as R
    case, so = setting(kind, n, **kw)
    return case, so, R._capi.SssScene.from_buffer_copy(bytes(so))


@pytest.mark.parametrize("literal", [False, True], ids=["projection", "literal"])
@pytest.mark.parametrize("cavity", [False, True], ids=["nofade", "fade"])
@pytest.mark.parametrize("kind,spp_n", [("plane", 1), ("plane", 2), ("plane", 3), ("sphere", 1), ("sphere", 2), ("sphere", 3)])
def test_walked_scene_is_the_integrator_bit_for_bit(ctx, kind, spp_n, cavity, literal):
    from rlshaders_amd import trace
    n = 150
    case, so, sg = scene_pair(kind, n, use_cavity_fade=cavity, literal_matrix=literal)
    s = sampler(ctx, case)
    P = _dev(case["P"])
    q = trace.sss_probe_rays(s, P, spp_n, SEED)
    cnt, hP, hN, E = walked_hits(ctx, q, case, so, spp_n)
    got, dgot = q.resolve(cnt, hP, hN, E, use_cavity_fade=cavity, literal_matrix=literal, want_depth=True)
    ref, dref = s.integrateScatter(P, sg, spp_n, SEED, want_depth=True)
    print("walk e2e", kind, spp_n, cavity, literal, "words differing", int((_host(got).view(np.uint32) != _host(ref).view(np.uint32)).sum()),
          "depths differing", int((_host(dgot) != _host(dref)).sum()))
    cases.assert_same_bits(_host(got), _host(ref), (kind, spp_n, "result"))
    cases.assert_same_bits(_host(dgot), _host(dref), (kind, spp_n, "mean_depth"))
    assert float(_host(dref).mean()) > 0.2


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_walked_scene_under_a_fast_context(ctx, kind):
    """The whole chain under RLS_MATH_FAST against the FAST integrator: the FAST emit's rays, the walk (it has one flavour), the
    FAST resolve, against rls_sss_integrate_scatter under the same context.
    Plane: bit for bit in result and mean_depth, as under EXACT -- the host's plane trace is the integrator's in either mode.
    Sphere: the FAST integrator intersects the sphere in FAST arithmetic inside its kernel (the hardware's reciprocal and square
    root), which no host tracer reproduces, so its hits are not bit for bit the walked ones.  There the bitwise claim is replaced
    by the gates the FAST integrator itself is held to (tests/test_gpu_scatter.py, test_fast_mode_within_roundoff): relative error
    of result median <= 1e-5 and p99 <= 1e-3, nothing non-finite, mean_depth differing on fewer than 1e-3 of the points."""
    from rlshaders_amd import trace
    n, spp_n = 150, 2
    case, so, sg = scene_pair(kind, n, use_cavity_fade=True)
    P = _dev(case["P"])
    ctx.set_math_mode(True)
    try:
        s = sampler(ctx, case)
        q = trace.sss_probe_rays(s, P, spp_n, SEED)
        cnt, hP, hN, E = walked_hits(ctx, q, case, so, spp_n)
        got, dgot = (_host(t) for t in q.resolve(cnt, hP, hN, E, use_cavity_fade=True, want_depth=True))
        ref, dref = (_host(t) for t in s.integrateScatter(P, sg, spp_n, SEED, want_depth=True))
    finally:
        ctx.set_math_mode(False)
    st = cases.summarize(cases.rel_err(got, ref))
    print("walk chain FAST vs the FAST integrator", kind, "words differing", int((got.view(np.uint32) != ref.view(np.uint32)).sum()),
          "of", got.size, "depths differing", int((dgot != dref).sum()), st)
    assert float(dref.mean()) > 0.2
    if kind == "plane":
        cases.assert_same_bits(got, ref, "fast result")
        cases.assert_same_bits(dgot, dref, "fast mean_depth")
    else:
        assert st["nonfinite"] == 0 and st["median"] <= 1e-5 and st["p99"] <= 1e-3
        assert (dgot != dref).mean() < 1e-3


# ---- 4. a whole walk in a graph ----------------------------------------------------------------------------------------------------
def test_whole_walk_in_a_graph_replayed_on_fresh_hits(ctx):
    """begin + 12 steps over a tracer that is itself a torch op (a plane's closest hit), recorded once, replayed on a second
    queue's contents"""
    from rlshaders_amd import trace, walk
    n = TILE + 9
    rng = np.random.default_rng(7)
    nrm = torch.tensor([0.0, 0.0, 1.0], device="cuda")

    def tracer(r):                                                 # the plane z = 0, two-sided; every entry of the capacity
        denom = r.dir[2]
        t = -r.origin[2] / denom
        hit = (denom != 0) & (t > 0) & (t <= r.maxdist)
        Pn = r.origin + r.dir * t
        N = nrm[:, None].expand(3, t.shape[0]).contiguous()
        return walk.Found(hit.to(torch.uint8), t.contiguous(), Pn.contiguous(), N, N)

    def contents(seed):
        g = np.random.default_rng(seed)
        P = g.standard_normal((3, n)).astype(np.float32)
        d = g.standard_normal((3, n)).astype(np.float32)
        return P, (P + np.float32(0.01) * d).astype(np.float32), d, g.uniform(0.2, 3.0, n).astype(np.float32)

    import rlshaders_amd as R
    side = torch.cuda.Stream()                                     # (the NULL stream cannot be captured)
    gctx = R.Context(0)
    gctx.use_stream(side)
    q = trace.ProbeQueue(gctx, n, 1)
    Pd = torch.empty(3, n, device="cuda")
    results = []
    w = None
    graph = None

    def whole_walk():
        w.begin()
        for _ in range(TRIALS):
            w.step(tracer(w.rays))

    for seed in (11, 12):
        P, o, d, md = contents(seed)
        Pd.copy_(_dev(P)); q.origin.copy_(_dev(o)); q.dir.copy_(_dev(d)); q.maxdist.copy_(_dev(md))
        torch.cuda.synchronize()
        if graph is None:
            with torch.cuda.stream(side):
                w = walk.ProbeWalk(gctx, q, Pd)
                whole_walk()                                       # (the tracer's first run allocates: not while recording)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                whole_walk()
            torch.cuda.synchronize()
            w.hit_count.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        # the same walk step by step with the host count, and the statement over the same tracer
        wn = walk_np(o, d, md, P, 1)
        while wn.active:
            m = wn.active
            r = type("R", (), dict(origin=_dev(wn.origin), dir=_dev(wn.dir), maxdist=_dev(wn.maxdist)))
            f = tracer(r)
            wn.step(Found(_host(f.hit), _host(f.t), _host(f.P), _host(f.N), _host(f.Ns)))
        assert w.active == 0
        np.testing.assert_array_equal(_host(w.hit_count), wn.count)
        live = np.arange(TRIALS)[:, None] < wn.count[None, :]
        assert np.array_equal(_host(w.hit_P).view(np.uint32)[:, live], wn.hP.view(np.uint32)[:, live])
        results.append(wn.count.copy())
    del graph
    gctx.close()
    assert results[0].any() and not np.array_equal(results[0], results[1])


# ---- 5. the walk's hits through the other hand-offs ------------------------------------------------------------------------------
def test_walked_probes_of_the_skin_node_are_rls_skin_integrate(ctx):
    """trace.skin_node_rays(...).probes walked, then rls_trace_skin_resolve = rls_skin_integrate, as tests/test_gpu_trace_skin.py
    has it with the hits traced on the host: unit sphere, cavity fade, unit radiance and visibility"""
    import test_gpu_trace_skin as S
    from rlshaders_amd import trace
    trace.load()
    spp_n = 2
    b = S.Skin(ctx, O, 37, "sphere", True, False)
    lights = S._mk_lights(S.MIXED3)
    want = b.analytic(lights, spp_n)
    q = b.emit(trace, lights, spp_n)
    cnt, hP, hN, E = walked_hits(ctx, q.probes, dict(P=b.Ph), b.oscene, spp_n)
    out = q.resolve(*S._traced(ctx, q, (1.0, 1.0, 1.0)), cnt, hP, hN, E, use_cavity_fade=True, literal_matrix=False)
    S._same({k: _host(v) for k, v in out.items()}, want, "skin over the walk")
    assert (want["sss"] > 0).mean() > 0.2


def test_walked_hits_through_the_hits_emit(ctx):
    """rls_trace_sss_hits_emit / _resolve on the walk's planes (12 slots a ray) give, slot for slot, the E they give on the list
    traced on the host (one slot a ray: the plane), and the scatter resolve of either is the same bits"""
    import rlshaders_amd as R
    from rlshaders_amd import trace
    n, spp_n = 150, 2
    case, so, _ = scene_pair("plane", n, use_cavity_fade=True)
    s = sampler(ctx, case)
    P = _dev(case["P"])
    q = trace.sss_probe_rays(s, P, spp_n, SEED)
    cnt, hP, hN, _ = walked_hits(ctx, q, case, so, spp_n)
    origin, dirs, maxdist = host_queue(q)
    c1, p1, n1 = (_dev(a) for a in trace_queue(so, origin, dirs, maxdist))
    light = R.make_light(center=(0.5, 0.5, 4.0), radius=1.0, radiance=(2.0, 1.5, 1.0), mis_mode=0)
    results = []
    for c, hp, hn in ((cnt, hP, hN), (c1, p1[:, :1].contiguous(), n1[:, :1].contiguous())):
        hq = trace.sss_hit_rays(s, P, q, c, hp, hn, light, 2, 7, use_cavity_fade=True, trace_diffuse=True)
        vis = torch.ones(3, max(hq.shadow_count, 1), device="cuda")
        Ld = torch.full((3, max(hq.diffuse_count, 1)), 0.25, device="cuda")
        E = hq.resolve(vis, Ld)
        res = q.resolve(c, hp, hn, E, use_cavity_fade=True)
        results.append((hq.hit_count, hq.shadow_count, hq.diffuse_count, _host(hq.hit_element)[:hq.hit_count], _host(E), _host(res)))
    a, b = results
    assert a[:3] == b[:3] and a[0] > n // 2
    np.testing.assert_array_equal(a[3], b[3])                      # slot 0 of ray j is element j under either stride
    cases.assert_same_bits(a[4][:, 0], b[4][:, 0], "E at the first slot")
    assert not a[4][:, 1:].any()
    cases.assert_same_bits(a[5], b[5], "scatter resolve")
    assert (a[5] > 0).any()
