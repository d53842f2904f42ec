"""-m gpu: shadow rays walked on the device (include/rlshaders_amd_shadow_walk.h, rlshaders_amd/shadow_walk.py).

1. Every step = the statement (tests/shadow_walk_util.py, shadow_walk_np) bit for bit -- the device count, ray, origin, dir,
   maxdist, the steps left and T -- under a nearest-hit tracer over the slabs and the sphere, at ray counts around a wavefront and
   the kernels' tile (256 entries, one per lane), at every budget, with direct and indexed opacity (index entries past the table),
   base absent, present and aliasing the visibility, via absent and present, a device count absent, below and above rays; every
   buffer and the exact-size scratch inside sentinel-filled allocations, nothing written at or past the device count.
2. The synthetic streams of the CPU test (shadow_walk_util.rule_streams), one rule of the walk each.
3. End to end on rls_trace_ggx_direct_emit / rls_trace_disney_direct_emit queues: no occluder -- visibility 1 and the analytic
   light loop bit for bit; the slab-and-sphere scene with a table from rls_trace_ggx_opacity -- the walked visibility is
   trace.shadow_visibility over the visited hits bit for bit, and so are the resolves; rays behind the sphere exactly 0 and retired
   there; the shadow queue of trace.sss_hit_rays through via = hit_element.
4. A whole walk recorded into a graph and replayed; EXACT and FAST contexts write the same bytes."""
import numpy as np
import pytest
import torch

import cases
from shadow_walk_util import F, Found, Scene, nearest_tracer, rule_streams, shadow_walk_np
from test_shadow_walk_statement import TABLE, light_rays
from trace_opacity_util import same_bits
from trace_sss_util import same_bits_or_both_nan

pytestmark = pytest.mark.gpu

TILE = 256                                  # kShadowWalkTile = kBlock
SENTINEL = 0xA5
FILL = np.frombuffer(bytes([SENTINEL] * 4), np.float32)[0]
GUARD = 512                                 # bytes of sentinel either side of every buffer
SLABS = [((0.0, 0.0, z), (0.0, 0.0, 1.0)) for z in (0.5, 0.8, 1.1)]
SPHERE = ((-1.5, 0.75, 1.6), 0.45)


@pytest.fixture(scope="module")
def ctx():
    import rlshaders_amd as R
    from rlshaders_amd import build
    build.build_trace_library()
    build.build_shadow_walk_library()
    c = R.Context(0)
    yield c
    c.close()


def _host(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """an allocator for shadow_walk.ShadowWalk: every tensor an inner view of a sentinel-filled buffer"""

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


def device_found(f):
    from rlshaders_amd import shadow_walk
    return shadow_walk.Found(_dev(f.hit), _dev(f.t), _dev(f.P), _dev(f.opacity), None if f.index is None else _dev(f.index))


def assert_same_state(w, wn, what):
    """the device's active list and T = the statement's, bit for bit"""
    m = w.active
    assert m == wn.active, (what, "active", m, wn.active)
    r = w.rays
    np.testing.assert_array_equal(_host(r.ray)[:m].view(np.uint32), wn.ray, str(what))
    np.testing.assert_array_equal(_host(r.trials)[:m], wn.steps, str(what))
    same_bits_or_both_nan(_host(r.origin)[:, :m], wn.origin, (what, "origin"))
    same_bits_or_both_nan(_host(r.dir)[:, :m], wn.dir, (what, "dir"))
    same_bits_or_both_nan(_host(r.maxdist)[:m], wn.maxdist, (what, "maxdist"))
    same_bits_or_both_nan(_host(w.visibility)[:, :wn.rays], wn.T, (what, "T"))


def raw_queue(dirs, maxdist, point, count=None):
    from rlshaders_amd import shadow_walk
    return shadow_walk.RawQueue(_dev(dirs), _dev(maxdist), _dev(np.asarray(point, np.int32)),
                                None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda"))


def walk_both(ctx, queue, O, point, dirs, maxdist, tracer, max_steps, base=None, alias=False, via=None, count=None, steps=None,
              what=""):
    """the device's walk and the statement's side by side over one host tracer (an object over the listed rays, or a list of
    Found, one a step), compared after begin and after every step -> (the device walk, the statement, the active counts)"""
    from rlshaders_amd import shadow_walk
    rays = len(maxdist)
    alloc = Guarded()
    out = alloc((3, rays), torch.float32)
    base_t = None
    if base is not None:
        base_t = out if alias else _dev(base)
        if alias:
            out.copy_(_dev(base))
    w = shadow_walk.ShadowWalk(ctx, queue, _dev(O), base=base_t, via=None if via is None else _dev(np.asarray(via, np.int64)),
                               max_steps=max_steps, out=out, alloc=alloc)
    assert w.scratch.numel() == shadow_walk.scratch_bytes(rays)                  # the exact size, between sentinels
    wn = shadow_walk_np(O, point, dirs, maxdist, max_steps, base=base, via=via, count=count, fill=FILL)
    if alias:
        wn.T[:, wn.walked:] = base[:, wn.walked:]                                # what the caller had there stays
    assert_same_state(w, wn, (what, "begin"))
    # nothing of the first list is written at or past its count
    for plane in (w.rays.ray, w.rays.maxdist, w.rays.trials, w.rays.origin, w.rays.dir) if rays else ():
        assert (_host(plane.reshape(-1, plane.shape[-1])[:, wn.active:].contiguous().view(torch.uint8)) == SENTINEL).all(), what
    counts = []
    for step in range(max_steps if steps is None else steps):
        if wn.active == 0:
            break
        counts.append(wn.active)
        f = tracer[step] if isinstance(tracer, list) else tracer(wn.ray, wn.origin, wn.dir, wn.maxdist)
        w.step(device_found(f), bound=wn.active)
        wn.step(f)
        assert_same_state(w, wn, (what, "step", step))
    alloc.check()
    return w, wn, counts


def scene_rays(rays, seed=7):
    O, point, dirs, maxdist = light_rays((rays + 1) // 2, seed)
    return O, point[:rays], np.ascontiguousarray(dirs[:, :rays]), np.ascontiguousarray(maxdist[:rays])


class past_table(nearest_tracer):
    """the sphere's hits name an entry past the table: the last entry is read"""

    def __call__(self, *a):
        f = super().__call__(*a)
        f.index = np.where(f.index == 3, np.where(np.arange(len(f.index)) % 2 == 0, -1, 0x7FFFFFF0), f.index).astype(np.int32)
        return f


# ---- 1. every step = the statement ---------------------------------------------------------------------------------------------
RAYS = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
BUDGETS = [1, 2, 12, 255]
# opacity, base, via, the device count (relative to rays): every value of each meets every ray count and every budget in turn
OPACITY, BASE, VIA, COUNT = ("direct", "indexed", "past"), ("none", "given", "alias"), (False, True), (None, -5, 0, 7)


@pytest.mark.parametrize("max_steps", BUDGETS)
@pytest.mark.parametrize("rays", RAYS)
def test_every_step_is_the_statement(ctx, rays, max_steps):
    k = RAYS.index(rays) + 2 * BUDGETS.index(max_steps)
    for opacity, base_kind, with_via, dcount in ((OPACITY[k % 3], BASE[(k // 3 + k) % 3], VIA[k % 2], COUNT[k % 4]),
                                                  (OPACITY[(k + 1) % 3], BASE[(k + 1) % 3], VIA[(k + 1) % 2], COUNT[(k + 2) % 4])):
        O, point, dirs, maxdist = scene_rays(rays)
        rng = np.random.default_rng(rays + max_steps)
        count = None if dcount is None else rays + dcount
        base = None if base_kind == "none" else (rng.random((3, rays), F) * F(1.5) - F(0.25)).astype(F)
        via, table_O = None, O
        if with_via:
            via = rng.permutation(O.shape[1])
            table_O = np.empty_like(O)
            table_O[:, via] = O
        scene = Scene(SLABS, [SPHERE])
        tracer = (past_table if opacity == "past" else nearest_tracer)(scene, TABLE, rays, indexed=opacity != "direct")
        what = (rays, max_steps, opacity, base_kind, with_via, dcount)
        _, wn, counts = walk_both(ctx, raw_queue(dirs, maxdist, point, count), table_O, point, dirs, maxdist, tracer, max_steps,
                                  base=base, alias=base_kind == "alias", via=via, count=count, what=what)
        assert wn.active == 0 and wn.walked == (rays if count is None else max(min(rays, count), 0))
        if rays >= TILE - 1 and max_steps >= 12:
            assert 3 <= len(counts) <= 5 and any(3 in v for v in tracer.visited)


# ---- 2. the rules, on the streams of the CPU test -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rule_streams()))
def test_rule_stream(ctx, name):
    begin, founds = rule_streams()[name]
    q = raw_queue(begin["dirs"], begin["maxdist"], begin["point"], begin["count"])
    _, wn, counts = walk_both(ctx, q, begin["O"], begin["point"], begin["dirs"], begin["maxdist"], list(founds), begin["max_steps"],
                              base=begin["base"], count=begin["count"], steps=len(founds), what=name)
    if name == "lanes":                                             # all, one lane a wavefront, one lane in all, none survive
        assert counts == [197, 197, 3, 1] and wn.active == 0
    if name == "budget_255":
        assert counts == [2] * 255 and wn.active == 0


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------
N, SPP_N, SEED = 67, 2, 9157
LIGHT_SPECS = (dict(center=(2.0, 2.0, 3.0), radius=1.25, radiance=(3.0, 2.0, 1.0), mis_mode=0),
               dict(center=(-3.0, 1.0, 2.5), radius=0.5, radiance=(0.5, 4.0, 2.0), mis_mode=1))
E2E_SLABS = [((0.0, 0.0, z), (0.0, 0.0, 1.0)) for z in (1.15, 1.35, 1.55)]
E2E_SPHERE = ((2.0, 2.0, 1.75), 0.3)


@pytest.fixture(scope="module")
def T():
    from rlshaders_amd import build, trace
    build.build_trace_library()
    trace.load()
    return trace


def batch(T, gpu, oracle, node):
    from test_gpu_loop_edges import _lights
    from test_gpu_trace_lights import Batch
    _, lights = _lights(oracle, LIGHT_SPECS)
    return Batch(T, gpu, node, N, oracle), lights


def surface_table(T, gpu):
    """sg->out_opacity of the four surfaces at a shadow ray's point: three tinted slabs, Kt = 0.5, and the sphere, Kt = 0: opaque"""
    shadow = torch.full((4,), T.RLS_RT_SHADOW, dtype=torch.uint8, device="cuda")
    kt = _dev(np.array([[0.2, 0.8, 0.5, 1.0], [0.9, 0.4, 0.5, 1.0], [0.7, 0.6, 1.0, 1.0]], F))
    return T.ggx_opacity(gpu, 4, KtColor=kt, Kt=_dev(np.array([0.5, 0.5, 0.5, 0.0], F)), ray_type=shadow)


def walk_scene(gpu, q, O, scene, table, max_steps=12, via=None, indexed=True):
    """the device's walk of q over the host's nearest-hit tracer -> (the walk, the tracer with its log, the rays retired black by
    a step and found in no later list)"""
    from rlshaders_amd import shadow_walk
    w = shadow_walk.ShadowWalk(gpu, q, O, via=via, max_steps=max_steps)
    tracer = nearest_tracer(scene, _host(table), w.capacity, indexed)
    ended = []
    for _ in range(max_steps):
        m = w.active
        if m == 0:
            break
        r = w.rays
        ray = _host(r.ray)[:m].view(np.uint32)
        f = tracer(ray, _host(r.origin)[:, :m], _host(r.dir)[:, :m], _host(r.maxdist)[:m])
        w.step(device_found(f), bound=m)
        opaque = ray[(f.hit != 0) & (f.index == scene.surfaces - 1)] if indexed else ray[:0]
        after = _host(w.rays.ray)[:w.active].view(np.uint32)
        assert not np.intersect1d(opaque, after).size                # retired at that step
        ended.extend(opaque.tolist())
    assert w.active == 0
    return w, tracer, np.array(ended, np.int64)


@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_no_occluder_is_the_analytic_light_loop(gpu, oracle, T, node):
    from rlshaders_amd import shadow_walk
    b, lights = batch(T, gpu, oracle, node)
    q = b.emit(lights, SPP_N, SEED)
    vis = torch.full((3, q.capacity), -3.0, device="cuda")
    w = shadow_walk.ShadowWalk(gpu, q, b.P, out=vis)
    rays = q.count
    assert rays > N and w.active == int((_host(q.maxdist) > 0).sum())
    h = _host(vis)
    assert (h[:, :rays] == 1).all() and (h[:, rays:] == -3).all()    # nothing at or past the device count
    w.step(shadow_walk.Found(torch.zeros(q.capacity, dtype=torch.uint8, device="cuda"), torch.zeros(q.capacity, device="cuda"),
                             torch.zeros(3, q.capacity, device="cuda"), torch.zeros(3, q.capacity, device="cuda")))
    assert w.active == 0 and (_host(vis)[:, :rays] == 1).all()
    dd, ds = q.resolve(w.visibility)
    want = b.analytic(lights, SPP_N, SEED)
    cases.assert_same_bits(_host(dd), want[0], (node, "direct_diffuse"))
    cases.assert_same_bits(_host(ds), want[1], (node, "direct_specular"))


@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_slabs_and_sphere_walked_is_the_fold_over_the_visited_hits(gpu, oracle, T, node):
    b, lights = batch(T, gpu, oracle, node)
    q = b.emit(lights, SPP_N, SEED)
    rays = q.count
    table = surface_table(T, gpu)
    scene = Scene(E2E_SLABS, [E2E_SPHERE])
    w, tracer, ended = walk_scene(gpu, q, b.P, scene, table)
    count, index, K = tracer.hits()
    assert K >= 3 and count.max() >= 3
    hits = T.ShadowHits(_dev(count), table, K, stride=q.capacity, index=_dev(index.astype(np.int32)))
    folded = T.shadow_visibility(gpu, rays, hits)
    got = _host(w.visibility)[:, :rays]
    cases.assert_same_bits(got, _host(folded), (node, "visibility"))
    # a ray behind the opaque sphere is exactly +0, the others are not black
    assert ended.size > 0 and (got[:, ended].view(np.uint32) == 0).all()
    clear = np.setdiff1d(np.arange(rays), ended)
    assert (got[:, clear] > 0).all() and ((got[:, clear] < 1).any(axis=0)).sum() > rays // 4
    walked, listed = q.resolve(w.visibility), q.resolve(folded)
    for k, name in enumerate(("direct_diffuse", "direct_specular")):
        cases.assert_same_bits(_host(walked[k]), _host(listed[k]), (node, name))
    lit = b.analytic(lights, SPP_N, SEED)
    assert (_host(walked[0]) < lit[0]).any()


def test_hit_queues_shadow_rays_start_at_the_hits_through_via(ctx):
    """the shadow queue of trace.sss_hit_rays: point is the hit's index in the LIST, via = hit_element leads to the hit's
    position in the hit planes; one tinted slab above the plane scene"""
    import rlshaders_amd as R
    from rlshaders_amd import trace
    from test_gpu_walk import sampler, scene_pair, walked_hits
    from trace_opacity_util import fold
    n, spp_n = 60, 2
    case, so, _ = scene_pair("plane", n, use_cavity_fade=True)
    s = sampler(ctx, case)
    P = _dev(case["P"])
    pq = trace.sss_probe_rays(s, P, spp_n, 4242)
    cnt, hP, hN, _ = walked_hits(ctx, pq, case, so, spp_n)
    light = R.make_light(center=(0.5, 0.5, 4.0), radius=1.0, radiance=(2.0, 1.5, 1.0), mis_mode=0)
    hq = trace.sss_hit_rays(s, P, pq, cnt, hP, hN, light, 2, 7, use_cavity_fade=True)
    rays = hq.shadow_count
    assert rays > n
    O = hP.reshape(3, -1)
    sh = hq.shadow
    point, dirs, maxdist = _host(sh["point"]), _host(sh["dir"]), _host(sh["maxdist"])
    via = _host(hq._hit_element)
    scene, table = Scene([((0.0, 0.0, 2.0), (0.0, 0.0, 1.0))]), np.array([[0.25], [0.5], [0.75]], F)
    tracer = nearest_tracer(scene, table, rays)
    cap = hq.shadow_capacity
    pad = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (cap - rays,), a.dtype)], axis=-1)
    # the statement over the whole capacity with the device count = the queue's ray count
    w, wn, counts = walk_both(ctx, hq, _host(O), pad(point), pad(dirs), pad(maxdist), tracer, 4, via=via, count=rays, what="hits")
    assert 1 <= len(counts) <= 2 and counts[0] == int((maxdist > 0).sum())
    start = _host(O)[:, via[point.astype(np.int64)]]
    assert np.isfinite(start).all()
    count, index, K = tracer.hits()
    assert same_bits(_host(w.visibility)[:, :rays], fold(rays, count, table, K, rays, index=index)) and count.any()
    E = hq.resolve(w.visibility)
    assert (_host(E) > 0).any()


# ---- 4. a graph; the math modes -------------------------------------------------------------------------------------------------
def slab_tracer(table):
    """the nearest of the three slabs as torch ops over every entry of the capacity (a tracer a graph can record)"""
    from rlshaders_amd import shadow_walk
    zs = torch.tensor([0.5, 0.8, 1.1], device="cuda")

    def tracer(r):
        t = (zs[:, None] - r.origin[2][None, :]) / r.dir[2][None, :]
        ok = (t > 1e-3) & (t <= r.maxdist[None, :])
        t = torch.where(ok, t, torch.full_like(t, float("inf")))
        tn, k = t.min(dim=0)
        hit = torch.isfinite(tn)
        tn = torch.where(hit, tn, torch.zeros_like(tn))
        Pn = r.origin + r.dir * tn
        return shadow_walk.Found(hit.to(torch.uint8), tn.contiguous(), Pn.contiguous(), table, index=k.to(torch.int32).contiguous())
    return tracer


def test_whole_walk_in_a_graph_replayed_gives_the_same_bytes(ctx):
    import rlshaders_amd as R
    from rlshaders_amd import shadow_walk
    rays, max_steps = TILE + 9, 5
    table = _dev(TABLE[:, :3])
    tracer = slab_tracer(table)
    side = torch.cuda.Stream()                                     # (the NULL stream cannot be captured)
    gctx = R.Context(0)
    gctx.use_stream(side)
    O0, point, d0, md0 = scene_rays(rays, 11)
    q = raw_queue(d0, md0, point)
    Od = _dev(O0)
    w, graph, results = None, None, []

    def whole_walk():
        w.begin()
        for _ in range(max_steps):
            w.step(tracer(w.rays))

    for seed in (11, 12):
        O, point, dirs, maxdist = scene_rays(rays, seed)
        maxdist = (maxdist * np.random.default_rng(seed).uniform(0.1, 1.0, rays)).astype(F)    # many rays end between the slabs
        Od.copy_(_dev(O)); q.dir.copy_(_dev(dirs)); q.maxdist.copy_(_dev(maxdist))
        torch.cuda.synchronize()
        # step by step on the default context, the host reading every count
        ws = shadow_walk.ShadowWalk(ctx, q, Od, max_steps=max_steps)
        steps = 0
        while ws.active:
            ws.step(tracer(ws.rays))
            steps += 1
        want = _host(ws.visibility).copy()
        if graph is None:
            with torch.cuda.stream(side):
                w = shadow_walk.ShadowWalk(gctx, q, Od, max_steps=max_steps)
                whole_walk()                                       # (the tracer's first run allocates: not while recording)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                whole_walk()
            torch.cuda.synchronize()
        w.visibility.fill_(77.0)
        graph.replay()
        torch.cuda.synchronize()
        assert w.active == 0 and 2 <= steps <= 4
        assert np.array_equal(_host(w.visibility).view(np.uint32), want.view(np.uint32))
        results.append(want)
    del graph
    gctx.close()
    assert (results[0] < 1).any() and not np.array_equal(results[0], results[1])


def test_exact_and_fast_contexts_write_the_same_bytes(ctx):
    rays = 3 * TILE + 5
    O, point, dirs, maxdist = scene_rays(rays)
    got = []
    for fast in (False, True):
        ctx.set_math_mode(fast)
        try:
            tracer = nearest_tracer(Scene(SLABS, [SPHERE]), TABLE, rays)
            w, wn, counts = walk_both(ctx, raw_queue(dirs, maxdist, point), O, point, dirs, maxdist, tracer, 12, what=("fast", fast))
        finally:
            ctx.set_math_mode(False)
        got.append((_host(w.visibility).copy(), counts))
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32)) and got[0][1] == got[1][1]
