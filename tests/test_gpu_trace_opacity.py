"""GPU: shadow rays' hits (include/rlshaders_amd_trace.h, rls_trace_ggx_opacity / _disney_opacity / _skin_opacity /
rls_trace_shadow_visibility; rlshaders_amd/trace.py, ggx_opacity / disney_opacity / skin_opacity / ShadowHits /
shadow_visibility).

Every expected bit is the numpy float32 restatement of tests/trace_opacity_util.py -- the three nodes' rules, the stand-in's
clamp, the product as a loop over the hit slot -- or a call that is already held to its reference (the light-loop and node
resolves, rls_*_direct_lighting).  Restatement only: the reference's shader_evaluate cannot run against the stand-in, whose
AiShaderGlobalsApplyOpacity aborts.
  1. the opacity verbs: EXACT and FAST contexts, n at the lane, wave and workgroup edges, parameters uniform, per point, by
     reference (ids past the table) and mixed, ray types absent / all shadow / the bounce tests' mix, hostile values, rlSkin's
     incoming absent, present and aliasing the output, every output inside sentinels;
  2. the fold: direct and indexed, rays around the wave and workgroup edges, max_hits 1, 4 and 255, a padded stride, counts 0, 1,
     max, above max and 255, a wavefront whose last lane alone has hits, index entries past the table, base absent, present and
     aliasing the output, hostile opacities, sentinels;
  3. the fold feeding the light-loop and node resolves; 4. the bounce resolves' shadow points are the verbs' shadow branch;
  5. graph replay."""
import numpy as np
import pytest
import torch

import rlshaders_amd as R
import trace_opacity_util as U
from gpu_util import dev, host
from test_gpu_loop_edges import LIGHTS as LIGHTS8, _lights as _loop_lights
from test_gpu_trace_bounce import DEPTHS, Bounce, _planes, _resolve as _node_resolve
from test_gpu_trace_lights import Batch
from test_gpu_trace_shade import KBLOCK, Node, T  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = F(-7.25)
PAD = 19
SIZES = (1, 5, 67, KBLOCK + 1, 2049)
TABLE = 37
VERBS = ("ggx", "disney", "skin")


def _framed(ctx, n, fill=None):
    """a [3, n] view inside a sentinel-filled buffer (fill: the view's first contents, numpy [3, n])"""
    buf = torch.full((3, n + 2 * PAD), float(SENTINEL), dtype=torch.float32, device=ctx.torch_device)
    view = buf[:, PAD:PAD + n]
    if fill is not None:
        view.copy_(dev(fill))
    return buf, view


def _frame_untouched(buf, n):
    h = host(buf)
    return bool((h[:, :PAD] == SENTINEL).all() and (h[:, PAD + n:] == SENTINEL).all())


def _ids(seed, n):
    """material ids with entries at and past the table's end, and the two 32-bit extremes"""
    ids = np.random.default_rng(seed).integers(0, TABLE + 9, n).astype(np.int64)
    ids[::11] = TABLE
    ids[5::13] = 0xFFFFFFFF
    ids[7::17] = 0x80000000
    return ids.astype(np.uint32).view(np.int32)


def _params(verb, form, n, hostile, seed):
    """(host parameters, ids or None): uniform values, per-point planes, columns by reference, one plane among
    uniform values"""
    m = TABLE if form == "materials" else n
    ids = _ids(seed, n) if form == "materials" else None
    s = lambda k: U.values(seed + k, m, hostile=hostile)
    c = lambda k: U.values(seed + k, 3, m, hostile=hostile)
    if form == "uniform":
        # (KtColor * Kt passes 1 in the last channel; an opacity above 1 and one below 0)
        p = dict(ggx=dict(opacity=0.8, opacity_color=(0.9, 1.3, -0.1), KtColor=(0.2, 0.9, 2.5), Kt=0.5),
                 disney=dict(opacity=(0.7, 1.25, -0.5)), skin=dict(opacity=1.5, opacity_color=(0.4, 0.9, -0.0)))[verb]
    elif form == "mixed":
        p = dict(ggx=dict(opacity=0.8, opacity_color=c(1), KtColor=(0.2, 0.9, 2.5), Kt=s(3)),
                 disney=dict(opacity=c(0)), skin=dict(opacity=s(0), opacity_color=(0.4, 0.9, 1.1)))[verb]
    else:
        p = dict(ggx=dict(opacity=s(0), opacity_color=c(1), KtColor=c(2), Kt=s(3)), disney=dict(opacity=c(0)),
                 skin=dict(opacity=s(0), opacity_color=c(1)))[verb]
    return p, ids


def _reference(verb, n, p, rt, ids, incoming=None):
    kw = dict(ray_type=rt, ids=ids, count=TABLE)
    if verb == "ggx":
        return U.ggx_opacity(n, p["opacity"], p["opacity_color"], p["KtColor"], p["Kt"], **kw)
    if verb == "disney":
        return U.disney_opacity(n, p["opacity"], **kw)
    return U.skin_opacity(n, p["opacity"], p["opacity_color"], incoming=incoming, **kw)


def _call(T, ctx, verb, n, p, rt, ids, out, incoming=None):
    d = {k: dev(v) if isinstance(v, np.ndarray) else v for k, v in p.items()}
    kw = dict(ray_type=None if rt is None else dev(rt), materials=None if ids is None else (dev(ids), TABLE), out=out)
    if verb == "skin":
        kw["incoming"] = incoming
    return getattr(T, verb + "_opacity")(ctx, n, **d, **kw)


# ---- 1. the opacity verbs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("form", ["uniform", "planes", "materials", "mixed"])
@pytest.mark.parametrize("verb", VERBS)
def test_the_opacity_verbs_are_the_restatement_bit_for_bit(gpu, T, verb, form, fast):
    gpu.set_math_mode(fast)
    try:
        for n in SIZES:
            for kind in ("none", "shadow", "mix"):
                for hostile in (False, True):
                    if hostile and form == "uniform":
                        continue
                    seed = 1000 * n + 10 * len(kind) + hostile
                    rt = U.ray_types(seed, n, kind)
                    p, ids = _params(verb, form, n, hostile, seed)
                    for inc in (("none", "plane", "alias") if verb == "skin" else ("none",)):
                        incoming = None if inc == "none" else U.values(seed + 9, 3, n, hostile=hostile)
                        buf, out = _framed(gpu, n, incoming if inc == "alias" else None)
                        inc_dev = None if inc == "none" else out if inc == "alias" else dev(incoming)
                        got = _call(T, gpu, verb, n, p, rt, ids, out, inc_dev)
                        assert got is out
                        want = _reference(verb, n, p, rt, ids, incoming)
                        what = (verb, form, fast, n, kind, hostile, inc)
                        assert U.same_bits(host(out), want), what
                        assert _frame_untouched(buf, n), what
    finally:
        gpu.set_math_mode(False)


def test_the_restatement_takes_every_branch_and_both_clamp_edges():
    """the inputs above reach what they are meant to reach: both branches, both clamp edges, NaN -> 1, -0 kept, an rlGgx shadow
    opacity below 0 and an rlDisney one above 1"""
    n = 2049
    rt = U.ray_types(3, n, "mix")
    sh = U.shadow_mask(rt, n)
    assert sh.any() and (~sh).any() and set(np.unique(rt)) == set(U.RAY_TYPES.tolist())
    assert U.same_bits(U.clamp(np.array([np.nan, -0.0, 0.0, -1.0, 2.0, np.inf, -np.inf, 0.25], F)),
                       np.array([1.0, -0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.25], F))
    p, _ = _params("ggx", "planes", n, True, 5)
    g = U.ggx_opacity(n, p["opacity"], p["opacity_color"], p["KtColor"], p["Kt"], ray_type=rt)
    assert (g[:, sh] < 0).any() and (g[:, sh] > 1).any() and np.isnan(g[:, sh]).any()
    assert ((g[:, ~sh] >= 0) & (g[:, ~sh] <= 1)).all()
    p, _ = _params("disney", "planes", n, True, 6)
    d = U.disney_opacity(n, p["opacity"], ray_type=rt)
    assert (d[:, sh] > 1).any() and (d[:, sh] < 0).any() and ((d[:, ~sh] >= 0) & (d[:, ~sh] <= 1)).all()


def test_the_opacity_verbs_on_a_ray_state(gpu, T):
    """ray_type as a RayState, defaults elsewhere: opaque off a shadow ray, rlGgx's Kt = 0 blocks a shadow ray too"""
    n = 300
    st = T.RayState(*[dev(np.ascontiguousarray(v)) for v in ([U.ray_types(1, n, "mix")] + [np.zeros(n, np.uint8)] * 4)])
    for verb in VERBS:
        assert (host(getattr(T, verb + "_opacity")(gpu, n, ray_type=st)) == 1.0).all(), verb


# ---- 2. the fold ---------------------------------------------------------------------------------------------------------------
RAYS = (1, 63, 64, 65, KBLOCK - 1, KBLOCK, KBLOCK + 1, 3 * 2048 + 5)


def _fold_inputs(seed, rays, max_hits, stride, indexed, hostile):
    count = U.counts(seed, rays, max_hits)
    elements = max_hits * stride
    if indexed:
        opacity = U.values(seed + 1, 3, TABLE, hostile=hostile)
        index = np.random.default_rng(seed + 2).integers(0, TABLE + 5, elements).astype(np.int64)
        index[::9] = TABLE                                       # the first entry past the table, and both 32-bit extremes
        index[4::19] = 0xFFFFFFFF
        index[6::23] = 0x80000000
        index = index.astype(np.uint32).view(np.int32)
    else:
        opacity, index = U.values(seed + 1, 3, elements, hostile=hostile), None
    return count, opacity, index


def _fold(T, ctx, rays, count, opacity, index, max_hits, stride, base, what):
    """the fold with base absent, present, and aliasing the (sentinel-framed) output, against the numpy loop"""
    hits = T.ShadowHits(dev(count), dev(opacity), max_hits, stride=stride, index=None if index is None else dev(index))
    for mode in ("none", "plane", "alias"):
        b = None if mode == "none" else base
        buf, out = _framed(ctx, rays, b if mode == "alias" else None)
        got = T.shadow_visibility(ctx, rays, hits, base=None if b is None else out if mode == "alias" else dev(b), out=out)
        assert got is out
        want = U.fold(rays, count, opacity, max_hits, stride, index=index, base=b)
        assert U.same_bits(host(out), want), (what, mode)
        assert _frame_untouched(buf, rays), (what, mode)
    return want


@pytest.mark.parametrize("indexed", [False, True], ids=["direct", "indexed"])
@pytest.mark.parametrize("max_hits", [1, 4, 255])
def test_the_fold_is_the_numpy_loop_bit_for_bit(gpu, T, max_hits, indexed):
    for rays in (RAYS[:4] if max_hits == 255 else RAYS):
        for stride in (rays, rays + 13):
            for hostile in (False, True):
                seed = 100 * rays + max_hits + hostile
                count, opacity, index = _fold_inputs(seed, rays, max_hits, stride, indexed, hostile)
                base = U.values(seed + 3, 3, rays, hostile=hostile)
                want = _fold(T, gpu, rays, count, opacity, index, max_hits, stride, base, (rays, stride, max_hits, indexed, hostile))
                if hostile and rays >= 63 and max_hits > 1:
                    assert np.isnan(want).any() and np.isinf(want).any() and (want < 0).any() and (want > 1).any()


def test_the_fold_with_hits_on_the_last_lane_of_a_wavefront_alone(gpu, T):
    """one wavefront's k loop runs for its last lane only; its neighbours -- and every other wavefront -- get base, or 1"""
    rays, max_hits = KBLOCK + 1, 4
    for lane in (63, 127, KBLOCK - 1, KBLOCK):
        count = np.zeros(rays, np.uint8)
        count[lane] = 255
        opacity = U.values(lane, 3, max_hits * rays)
        base = U.values(lane + 1, 3, rays)
        want = _fold(T, gpu, rays, count, opacity, None, max_hits, rays, base, ("last lane", lane))
        others = np.arange(rays) != lane
        assert U.same_bits(want[:, others], base[:, others]) and not U.same_bits(want[:, ~others], base[:, ~others])


def test_a_ray_without_hits_reads_no_element(gpu, T):
    """every count 0 over NaN opacities: the visibility is base, or 1, exactly"""
    rays, max_hits = 777, 4
    count = np.zeros(rays, np.uint8)
    opacity = np.full((3, max_hits * rays), np.nan, F)
    hits = T.ShadowHits(dev(count), dev(opacity), max_hits, stride=rays)
    assert (host(T.shadow_visibility(gpu, rays, hits)) == 1.0).all()
    base = U.values(8, 3, rays, hostile=True)
    assert U.same_bits(host(T.shadow_visibility(gpu, rays, hits, base=dev(base))), base)
    assert T.shadow_visibility(gpu, 0, T.ShadowHits(dev(count), dev(opacity), max_hits, stride=rays)).shape == (3, 0)


# ---- 3. the fold into the resolves ---------------------------------------------------------------------------------------------
def _synthetic_hits(T, ctx, rays, seed):
    """hits of `rays` shadow rays on surfaces that carry the three nodes, by reference: a table of TABLE surfaces whose opacities
    come from the verbs at shadow rays' points, counts 0 .. 3, an index per element.  -> (ShadowHits, numpy visibility)"""
    m, max_hits = TABLE, 3
    rt = np.full(m, U.SHADOW, np.uint8)
    u = lambda k, *shape: (np.random.default_rng(seed + k).random(shape, F)).astype(F)
    third = np.arange(m) % 3
    g = T.ggx_opacity(ctx, m, KtColor=dev(u(0, 3, m)), Kt=dev(u(1, m)), ray_type=dev(rt))
    d = T.disney_opacity(ctx, m, opacity=dev(u(2, 3, m)), ray_type=dev(rt))
    s = T.skin_opacity(ctx, m, opacity=dev(u(3, m)), opacity_color=dev(u(4, 3, m)), ray_type=dev(rt))
    table = torch.where(dev(third == 0)[None, :], g, torch.where(dev(third == 1)[None, :], d, s)).contiguous()
    want_table = np.where(third == 0, U.ggx_opacity(m, 1.0, (1.0, 1.0, 1.0), u(0, 3, m), u(1, m), ray_type=rt),
                          np.where(third == 1, U.disney_opacity(m, u(2, 3, m), ray_type=rt),
                                   U.skin_opacity(m, u(3, m), u(4, 3, m), ray_type=rt))).astype(F)
    assert U.same_bits(host(table), want_table)
    rng = np.random.default_rng(seed + 5)
    count = rng.integers(0, max_hits + 1, rays).astype(np.uint8)
    index = rng.integers(0, m, max_hits * rays).astype(np.int32)
    hits = T.ShadowHits(dev(count), table, max_hits, stride=rays, index=dev(index))
    return hits, U.fold(rays, count, want_table, max_hits, rays, index=index), count


@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_the_fold_feeds_the_light_loop_resolve(gpu, oracle, T, node):
    _, lights = _loop_lights(oracle, LIGHTS8[:2])
    n, spp_n = 777, 3
    b = Batch(T, gpu, node, n, oracle)
    q = b.emit(lights, spp_n)
    rays = q.count
    assert rays > n
    hits, want_vis, count = _synthetic_hits(T, gpu, rays, 31)
    vis = T.shadow_visibility(gpu, rays, hits)
    assert U.same_bits(host(vis), want_vis) and (want_vis < 1).any() and (count == 0).any()
    got = [host(t) for t in q.resolve(vis)]
    want = [host(t) for t in q.resolve(dev(want_vis))]
    assert U.same_bits(got[0], want[0]) and U.same_bits(got[1], want[1])
    assert not U.same_bits(got[1], b.analytic(lights, spp_n)[1])                    # the shadows are there
    # no hit on any ray: the analytic light loop, bit for bit
    clear = T.ShadowHits(dev(np.zeros(rays, np.uint8)), hits.opacity, hits.max_hits, stride=rays, index=hits.index)
    got = [host(t) for t in q.resolve(T.shadow_visibility(gpu, rays, clear))]
    ref = b.analytic(lights, spp_n)
    assert U.same_bits(got[0], ref[0]) and U.same_bits(got[1], ref[1])


def test_the_fold_feeds_the_node_resolve(gpu, oracle, T):
    from test_gpu_shade import _lights
    _, lights = _lights(oracle)
    n, spp_n = 777, 3
    b = Node(T, gpu, oracle, "ggx", n)
    nq = b.emit(lights, spp_n)
    planes = _planes(gpu, nq, seed=11)
    rays = nq.shadow.count
    hits, want_vis, _ = _synthetic_hits(T, gpu, rays, 47)
    vis = T.shadow_visibility(gpu, rays, hits)
    got = _node_resolve(nq, [vis] + planes[1:])
    want = _node_resolve(nq, [dev(want_vis)] + planes[1:])
    for k in want:
        assert U.same_bits(got[k], want[k]), k
    clear = T.ShadowHits(dev(np.zeros(rays, np.uint8)), hits.opacity, hits.max_hits, stride=rays, index=hits.index)
    got = _node_resolve(nq, [T.shadow_visibility(gpu, rays, clear)] + planes[1:])
    want = _node_resolve(nq, [torch.ones(3, rays, device=gpu.torch_device)] + planes[1:])
    for k in want:
        assert U.same_bits(got[k], want[k]), k


# ---- 4. the bounce resolve's shadow points ---------------------------------------------------------------------------------------
def test_the_shadow_branch_is_taken_where_the_bounce_resolve_writes_zero(gpu, oracle, T):
    """on a mixed RayState: rls_trace_ggx_bounce_resolve leaves +0 in every plane at exactly the points where ggx_opacity
    returns 1 - KtColor * Kt instead of the clamped opacity"""
    from test_gpu_shade import _lights
    _, lights = _lights(oracle)
    n, spp_n = 700, 2
    b = Bounce(T, gpu, oracle, "ggx", n)
    sth, state = b.state()
    nq = b.bounce(lights, spp_n, state, DEPTHS)
    out = _node_resolve(nq, _planes(gpu, nq, value=(0.7, 0.8, 0.9)))
    # an opacity of 2 clamps to 1 off a shadow ray; KtColor * Kt = 3 gives -2 on one
    o = host(T.ggx_opacity(gpu, n, opacity=2.0, KtColor=(3.0, 3.0, 3.0), Kt=1.0, ray_type=state))
    took_shadow = (o == -2.0).all(axis=0)
    assert ((o == -2.0) | (o == 1.0)).all() and took_shadow.any() and not took_shadow.all()
    assert np.array_equal(took_shadow, (sth[0] & U.SHADOW) != 0)
    # the same points without the shadow bit: what the bit alone changes
    lit = sth.copy()
    lit[0] &= ~np.uint8(U.SHADOW)
    nl = b.bounce(lights, spp_n, T.RayState(*[dev(lit[k]) for k in range(5)]), DEPTHS)
    ref = _node_resolve(nl, _planes(gpu, nl, value=(0.7, 0.8, 0.9)))
    changed, zero = np.zeros(n, bool), np.ones(n, bool)
    for k, v in out.items():
        bits, rbits = np.ascontiguousarray(v).view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32)
        zero &= (bits == 0).all(axis=0)
        changed |= (bits != rbits).any(axis=0)
    assert zero[took_shadow].all()                                   # +0 in every plane of a shadow ray's point
    assert not changed[~took_shadow].any() and changed[took_shadow].any()     # and the bit changes no other point


# ---- 5. graph replay -----------------------------------------------------------------------------------------------------------
def test_the_verbs_and_the_fold_replay_in_a_graph(T):
    m, rays, max_hits = TABLE, 3 * KBLOCK + 7, 4
    gctx = R.Context(0, use_torch_stream=False)          # the context's own stream: the NULL stream cannot be captured
    try:
        rt = dev(np.full(m, U.SHADOW, np.uint8))
        kt, op = U.values(1, 3, m), U.values(2, 3, m)
        count, _, index = _fold_inputs(3, rays, max_hits, rays, True, False)
        base = U.values(4, 3, rays)
        dkt, dop, dcount, dindex, dbase = dev(kt), dev(op), dev(count), dev(index), dev(base)
        tg, td, ts = gctx.empty(3, m), gctx.empty(3, m), gctx.empty(3, m)
        vis = gctx.empty(3, rays)
        hits = T.ShadowHits(dcount, tg, max_hits, stride=rays, index=dindex)
        torch.cuda.synchronize()
        with gctx.capture() as g:
            T.ggx_opacity(gctx, m, KtColor=dkt, Kt=0.5, ray_type=rt, out=tg)
            T.disney_opacity(gctx, m, opacity=dop, ray_type=rt, out=td)
            T.skin_opacity(gctx, m, opacity=0.9, opacity_color=dop, ray_type=rt, incoming=td, out=ts)
            T.shadow_visibility(gctx, rays, hits, base=dbase, out=vis)
        for t in (tg, td, ts, vis):
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        g.launch()
        gctx.synchronize()
        g.close()
        want_g = U.ggx_opacity(m, 1.0, (1.0, 1.0, 1.0), kt, 0.5, ray_type=np.full(m, U.SHADOW, np.uint8))
        want_d = U.disney_opacity(m, op, ray_type=np.full(m, U.SHADOW, np.uint8))
        want_s = U.skin_opacity(m, 0.9, op, ray_type=np.full(m, U.SHADOW, np.uint8), incoming=want_d)
        assert U.same_bits(host(tg), want_g) and U.same_bits(host(td), want_d) and U.same_bits(host(ts), want_s)
        assert U.same_bits(host(vis), U.fold(rays, count, want_g, max_hits, rays, index=index, base=base))
    finally:
        gctx.close()
