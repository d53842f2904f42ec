"""GPU: the caller-traced shading of rlSss's probe hits (rls_trace_sss_hits_emit / _resolve, include/rlshaders_amd_trace.h;
rlshaders_amd.trace.sss_hit_rays / HitQueues.resolve): evalLightSample's light loop and integrateDiffuse's ray at every hit the
scatter resolve counts as shaded.  Checked here:
  1. unit visibility, no diffuse ray: E at the listed hits IS rls_ggx_direct_lighting's direct_diffuse over the flattened hit
     elements (P = hitP, N = wo = hitN, T = hitT, KdColor = Kd = 1, diffuseRoughness 0), bit for bit, EXACT and FAST, and
     rls_trace_ggx_direct_emit / _resolve's at visibility 1;
  2. the list against a numpy restatement of the gate and against the scatter resolve's mean_depth; E == 0 elsewhere;
  3. the shadow queue against the diffuse-carrying rays of rls_trace_ggx_direct_emit, and its invariants;
  4. the diffuse ray, the documented composition in numpy float32 and a float64 bound, non-finite values on absent terms;
  5. end to end through rls_trace_sss_scatter_resolve and rls_trace_skin_resolve;
  6. edges: scan tiles, overflow, exact scratch, no lights, chunks, graph replay, argument checks.

The reference's specular closure never reaches direct_diffuse: on the CPU the oracle's orc_batch_ggx_direct_lighting_two_sums
returns the same direct_diffuse words at diffuseRoughness 0 whatever the roughness, anisotropy, ior, KsColor and Ks are.  The
view does, through Oren-Nayar's side test alone (N . wo > 0, else the term is 0): both sides take wo = hitN."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import rlshaders_amd as R
import trace_sss_util as U
from gpu_util import dev, host
from test_gpu_loop_edges import LIGHTS, _lights
from trace_hits_util import (BSDF, DIFFUSE, LIGHT_MASK, compose_E, gate_np, listed_elements, orthogonal_tangent, queues_host,
                             shadow_keys, synthetic_hits, tangent_np)
from trace_lights_util import compose, near_hit_f64, queue_host

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 6173
INVALID = 1            # RLS_ERR_INVALID_ARGUMENT
N_PTS, SPP_N, MAX_HITS = 67, 2, 3
ONE_LIGHT = dict(center=(1.5, 2.5, 3.5), radius=1.25, radiance=(3.0, 2.0, 0.5), mis_mode=0)


@pytest.fixture(scope="module")
def T():
    from rlshaders_amd import build, trace
    build.build_trace_library()
    trace.load()
    return trace


def _sss(ctx, case, has_dPdu=True):
    return R.SssSampler(ctx, dev(case["N"]), dev(case["T"]), dev(case["albedo"]), dev(case["dist"]), has_dPdu=has_dPdu)


class Hits:
    """one synthetic hit list over N_PTS points (trace_hits_util.synthetic_hits) on the device, with the probe queue the verbs
    take and the flattened elements the references run over"""

    def __init__(self, T, ctx, n=N_PTS, spp_n=SPP_N, max_hits=MAX_HITS, pad=5, seed=3, dense=False, shape=None, src=None):
        """shape(self): edits the host planes (case, cnt, hP, hN, hT) before they go to the device; src: another Hits of the
        same sizes whose host planes are taken as they are (the same hits on another context)"""
        self.T, self.ctx, self.n, self.spp_n, self.max_hits = T, ctx, n, spp_n, max_hits
        self.spp = spp_n * spp_n
        self.stride = n * self.spp + pad
        if src is None:
            self.case, self.cnt, self.hP, self.hN = synthetic_hits(n, self.spp, max_hits, self.stride, seed, dense)
            self.hT = orthogonal_tangent(self.hN.reshape(3, -1), seed + 1).reshape(self.hN.shape)
            if shape is not None:
                shape(self)
        else:
            assert (src.n, src.spp_n, src.max_hits, src.stride) == (n, spp_n, max_hits, self.stride)
            self.case, self.cnt, self.hP, self.hN, self.hT = src.case, src.cnt, src.hP, src.hN, src.hT
        self.s = _sss(ctx, self.case)
        self.P = dev(self.case["P"])
        self.pq = T.sss_probe_rays(self.s, self.P, spp_n, SEED)
        self.d = dict(cnt=dev(self.cnt), hP=dev(self.hP), hN=dev(self.hN), hT=dev(self.hT))

    def emit(self, lights, hit_spp_n, seed=SEED, first=0, hitT="given", **kw):
        d = self.d
        return self.T.sss_hit_rays(self.s, self.P, self.pq, d["cnt"], d["hP"], d["hN"], lights, hit_spp_n, seed,
                                   hitT=d["hT"] if isinstance(hitT, str) else hitT, hit_first_index=first, **kw)

    def elements(self, cavity):
        return listed_elements(gate_np(self.case, self.spp, self.cnt, self.hP, self.hN, self.max_hits, cavity), self.stride)

    def ggx(self, hT=None):
        """the rlGgx closure of the reference over the flattened elements: wo = N = hitN, T = hitT"""
        Nf = dev(np.ascontiguousarray(self.hN.reshape(3, -1)))
        Tf = dev(np.ascontiguousarray((self.hT if hT is None else hT).reshape(3, -1)))
        return R.GgxSampler(self.ctx, Nf, Nf, Tf, specColor=(0.9, 0.5, 0.3), ior=1.45, roughness=0.3), \
            dev(np.ascontiguousarray(self.hP.reshape(3, -1)))

    def direct_diffuse(self, lights, hit_spp_n, seed=SEED, first=0, hT=None):
        """rls_ggx_direct_lighting's direct_diffuse over every element -> [3, max_hits, stride]"""
        g, Pf = self.ggx(hT)
        dd, _ = g.directLighting(Pf, lights, hit_spp_n, seed, KdColor=(1.0, 1.0, 1.0), Kd=1.0, diffuseRoughness=0.0, Ks=0.5,
                                 first_index=first)
        return host(dd).reshape(3, self.max_hits, self.stride)


def _ones(ctx, count):
    return torch.ones(3, max(int(count), 1), dtype=torch.float32, device=ctx.torch_device)


def _at(monkeypatch, g, fn):
    if g is None:
        monkeypatch.delenv("RLS_INTEGRATE_GROUP", raising=False)
    else:
        monkeypatch.setenv("RLS_INTEGRATE_GROUP", str(g))
    try:
        return fn()
    finally:
        monkeypatch.delenv("RLS_INTEGRATE_GROUP", raising=False)


def _assert_E(E, want, elements, what):
    """E [3, max_hits, stride] equals `want` bit for bit at the listed elements and is exactly +0 everywhere else"""
    E, want = E.reshape(3, -1), want.reshape(3, -1)
    cases.assert_same_bits(E[:, elements], want[:, elements], (what, "listed"))
    rest = np.ones(E.shape[1], bool)
    rest[elements] = False
    assert not E[:, rest].view(np.uint32).any(), (what, "an unlisted element is not +0")


def _bytes_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---- 1. unit visibility: the analytic light loop's diffuse AOV at the hits ----------------------------------------------------
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_unit_visibility_is_direct_diffuse_at_the_hits(gpu, oracle, T, fast):
    """eight lights, the mis_modes mixed, one around every hit (cone.valid false), several below many hits' horizons; every
    hit_spp_n in 1..4; then 1 and 2 lights"""
    _, lights = _lights(oracle, LIGHTS)
    gpu.set_math_mode(fast)
    try:
        hits = Hits(T, gpu)
        el = hits.elements(True)
        assert 100 < len(el) < hits.max_hits * hits.n * hits.spp
        for nl, spp_ns in ((8, (1, 2, 3, 4)), (1, (2,)), (2, (3,))):
            for hit_spp_n in spp_ns:
                hq = hits.emit(lights[:nl], hit_spp_n, use_cavity_fade=True)
                assert hq.hit_count == len(el)
                E = host(hq.resolve(_ones(gpu, hq.shadow_count)))
                want = hits.direct_diffuse(lights[:nl], hit_spp_n)
                assert np.any(want.reshape(3, -1)[:, el] != 0)
                _assert_E(E, want, el, (fast, nl, hit_spp_n, "rls_ggx_direct_lighting"))
                # the same bits from the traced rlGgx light loop at visibility 1
                g, Pf = hits.ggx()
                q = T.ggx_shadow_rays(g, T.ggx_shader(g, KdColor=(1.0, 1.0, 1.0), Kd=1.0, diffuseRoughness=0.0, Ks=0.5), Pf,
                                      lights[:nl], hit_spp_n, SEED)
                dd = host(q.resolve(_ones(gpu, q.count))[0]).reshape(want.shape)
                _assert_E(E, dd, el, (fast, nl, hit_spp_n, "rls_trace_ggx_direct_resolve"))
    finally:
        gpu.set_math_mode(False)


def test_unit_visibility_at_every_group_width(gpu, oracle, T, monkeypatch):
    _, lights = _lights(oracle, LIGHTS[:5])
    hits = Hits(T, gpu)
    el = hits.elements(False)
    for hit_spp_n, g in ((2, 1), (2, 4), (4, 16), (4, 64), (3, 64), (4, None)):
        want = _at(monkeypatch, 1, lambda: hits.direct_diffuse(lights, hit_spp_n))
        hq = _at(monkeypatch, g, lambda: hits.emit(lights, hit_spp_n))
        _assert_E(host(hq.resolve(_ones(gpu, hq.shadow_count))), want, el, (hit_spp_n, g))
        if g != 1:                                                   # the queues do not depend on the width
            h1 = queues_host(_at(monkeypatch, 1, lambda: hits.emit(lights, hit_spp_n)))
            hg = queues_host(hq)
            for k in hg[0]:
                assert _bytes_equal(hg[0][k], h1[0][k]), (hit_spp_n, g, k)
            assert np.array_equal(hg[2], h1[2]) and hg[3] == h1[3]


def test_hit_first_index_past_2_36(gpu, oracle, T):
    _, lights = _lights(oracle, LIGHTS[:3])
    hits = Hits(T, gpu)
    el = hits.elements(True)
    first = (1 << 36) + 5
    hq = hits.emit(lights, 2, first=first, use_cavity_fade=True)
    E = host(hq.resolve(_ones(gpu, hq.shadow_count)))
    _assert_E(E, hits.direct_diffuse(lights, 2, first=first), el, "first 2^36 + 5")
    E0 = host(hits.emit(lights, 2, first=5, use_cavity_fade=True).resolve(_ones(gpu, hq.shadow_capacity)))
    assert not np.array_equal(E, E0)                                 # the high bits of the index reach the scrambles


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_no_hitT_is_the_documented_tangent(gpu, oracle, T, fast):
    """hitT = NULL: the frame's tangent is the header's stand-in for the polar frame (the closed AiBuildLocalFramePolar is an
    input of orc_sss_init as of every frame here: there is no tangent to take from it), restated in numpy float32"""
    _, lights = _lights(oracle, LIGHTS[:3])
    gpu.set_math_mode(fast)
    try:
        hits = Hits(T, gpu)
        hT = tangent_np(hits.hN.reshape(3, -1)).reshape(hits.hN.shape)
        a = hits.emit(lights, 3, hitT=None, trace_diffuse=True)
        b = hits.emit(lights, 3, hitT=dev(hT), trace_diffuse=True)
        ha, hb = queues_host(a), queues_host(b)
        assert ha[0]["count"] > 100 and ha[1]["count"] > 100
        for k in ha[0]:
            assert _bytes_equal(ha[0][k], hb[0][k]), ("shadow", k)
        for k in ha[1]:
            assert _bytes_equal(ha[1][k], hb[1][k]), ("diffuse", k)
        given = queues_host(hits.emit(lights, 3, trace_diffuse=True))
        assert not _bytes_equal(ha[1]["dir"], given[1]["dir"])       # (and another tangent gives other rays)
    finally:
        gpu.set_math_mode(False)


# ---- 2. the list --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cavity", [False, True], ids=["nofade", "fade"])
def test_the_list_is_the_scatter_resolves_gate(gpu, oracle, T, cavity):
    _, lights = _lights(oracle, [ONE_LIGHT])
    hits = Hits(T, gpu)
    keep = gate_np(hits.case, hits.spp, hits.cnt, hits.hP, hits.hN, hits.max_hits, cavity)
    el = listed_elements(keep, hits.stride)
    rays = hits.n * hits.spp
    # the inputs reach every branch: duplicates, hits past the radius, counts of 0 and above max_hits, a shut fade
    c = np.minimum(hits.cnt[:rays], hits.max_hits)
    reported = np.arange(hits.max_hits)[:, None] < c[None, :]
    assert (hits.cnt[:rays] == 0).any() and (hits.cnt[:rays] > hits.max_hits).any() and (reported & ~keep).sum() > 50
    if cavity:
        assert len(el) < len(listed_elements(gate_np(hits.case, hits.spp, hits.cnt, hits.hP, hits.hN, hits.max_hits, False),
                                             hits.stride))
    m = 3 * hits.max_hits * hits.stride
    guard = torch.full((m + 64,), -7.0, dtype=torch.float32, device=gpu.torch_device)
    E = guard[32:32 + m].view(3, hits.max_hits, hits.stride)
    hq = hits.emit(lights, 2, use_cavity_fade=cavity)
    _, _, got, count = queues_host(hq)
    np.testing.assert_array_equal(got, el)
    assert count == len(el)
    # per point: listed hits = mean_depth * spp^2 of the scatter resolve on the same hits with a non-zero E
    d = hits.d
    _, depth = hits.pq.resolve(d["cnt"], d["hP"], d["hN"], torch.ones_like(d["hP"]), use_cavity_fade=cavity, want_depth=True)
    per_point = np.bincount((el % hits.stride) // hits.spp, minlength=hits.n)
    np.testing.assert_array_equal(host(depth) * F(hits.spp), per_point.astype(F))
    # E written inside sentinel-filled planes: exactly 0 at every unlisted element, nothing outside the planes
    E = hq.resolve(_ones(gpu, hq.shadow_count), out=E)
    want = hits.direct_diffuse(lights, 2)
    _assert_E(host(E), want, el, ("list", cavity))
    assert torch.all(guard[:32] == -7.0) and torch.all(guard[32 + m:] == -7.0)


# ---- 3. the shadow queue --------------------------------------------------------------------------------------------------------
def assert_shadow_rays_are_the_ggx_emit(T, hits, sh, elements, lights, hit_spp_n, first=0, min_rays=1000):
    """the shadow queue `sh` over the list `elements` holds the diffuse-carrying rays of rls_trace_ggx_direct_emit over the
    flattened elements (hits: a Hits on the context the reference runs on), by (element, light, segment, sample): the same set,
    the same dir, weight_diffuse and maxdist bits"""
    g, Pf = hits.ggx()
    q = T.ggx_shadow_rays(g, T.ggx_shader(g, KdColor=(1.0, 1.0, 1.0), Kd=1.0, diffuseRoughness=0.0, Ks=0.5), Pf, lights,
                          hit_spp_n, SEED, first)
    h = queue_host(q)
    listed = np.zeros(hits.max_hits * hits.stride, bool)
    listed[elements] = True
    m = ((h["kind"] & DIFFUSE) != 0) & listed[h["point"]]
    ref = {k: h[k][..., m] for k in ("dir", "maxdist", "wd", "kind", "point", "sample")}
    ours, theirs = shadow_keys(sh, elements), shadow_keys(ref)
    assert sh["count"] > min_rays
    # the same (element, light, segment, sample) set; ours in list order, theirs in element order
    oa, ob = np.argsort(ours, kind="stable"), np.argsort(theirs, kind="stable")
    np.testing.assert_array_equal(ours[oa], theirs[ob])
    assert np.all(np.diff(ours[oa]) > 0)
    for k in ("dir", "wd", "maxdist"):
        assert _bytes_equal(sh[k][..., oa], ref[k][..., ob]), k


def assert_shadow_queue_invariants(hits, sh, elements, cap, specs, hit_spp, maxdist=True):
    """order, kind, cone and maxdist invariants of the shadow queue `sh` over the list `elements` (capacity `cap`), as
    tests/test_gpu_trace_lights.py holds them for a light loop's queue; specs: the lights' dicts"""
    el = elements
    off, kind = sh["offsets"], sh["kind"]
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and np.all(np.diff(off) <= len(specs) * 2 * hit_spp)
    assert off[cap] == sh["count"] and np.all(off[len(el):] == sh["count"])
    np.testing.assert_array_equal(sh["point"], np.repeat(np.arange(cap), np.diff(off)))
    assert np.all(kind & ~(LIGHT_MASK | BSDF) == DIFFUSE)            # the diffuse term and no other on every ray
    assert np.all(np.diff(((sh["point"] * 8 + (kind & LIGHT_MASK)) * 2 + ((kind & BSDF) != 0)) * 256 + sh["sample"]) > 0)
    assert np.all(sh["sample"] < hit_spp)
    modes = np.array([sp["mis_mode"] for sp in specs])[kind & LIGHT_MASK]
    bs = (kind & BSDF) != 0
    assert not np.any(bs & (modes == 1)) and not np.any(~bs & (modes == 2))
    assert np.all(np.isfinite(sh["maxdist"])) and np.all(sh["maxdist"] > 0) and np.all(sh["wd"] != 0)
    hP, hN = hits.hP.reshape(3, -1)[:, elements[sh["point"]]], hits.hN.reshape(3, -1)[:, elements[sh["point"]]]
    assert np.all((sh["dir"] * hN).sum(axis=0, dtype=F) > 0)         # above the hit's horizon
    for li, sp in enumerate(specs):
        mm = (kind & LIGHT_MASK) == li
        if maxdist and mm.any():
            t, disc, b = near_hit_f64(sp["center"], sp["radius"], hP[:, mm], sh["dir"][:, mm])
            away = disc >= 1e-5 * b * b                              # (within a few ulp of tangency maxdist loses its digits)
            rel = np.abs(sh["maxdist"][mm].astype(np.float64) - t) / t
            assert rel[away].max() <= 4 * 4.097e-5, (li, rel[away].max())   # test_gpu_trace_lights.py's bound


def test_shadow_rays_are_the_diffuse_rays_of_the_ggx_emit(gpu, oracle, T):
    specs = LIGHTS
    _, lights = _lights(oracle, specs)
    hits = Hits(T, gpu)
    hit_spp_n = 3
    el = hits.elements(True)
    hq = hits.emit(lights, hit_spp_n, use_cavity_fade=True)
    sh, _, elements, _ = queues_host(hq)
    np.testing.assert_array_equal(elements, el)
    assert_shadow_rays_are_the_ggx_emit(T, hits, sh, elements, lights, hit_spp_n)
    assert_shadow_queue_invariants(hits, sh, elements, hq.hit_capacity, specs, hit_spp_n * hit_spp_n)
    kind = sh["kind"]
    bs = (kind & BSDF) != 0
    assert bs.any() and (~bs).any()
    assert not np.any((kind & LIGHT_MASK) == 3)                      # the light around every hit


# ---- 4. the diffuse ray ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_diffuse_ray_direction_and_weight(gpu, oracle, T, fast):
    gpu.set_math_mode(fast)
    try:
        hits = Hits(T, gpu)
        first = 901
        hq = hits.emit(None, 1, first=first, trace_diffuse=True)
        _, df, elements, _ = queues_host(hq)
        total = hits.max_hits * hits.stride
        rx, ry = oracle.batch_sample_02(SEED, first, total, 24, 0)
        Nf, Tf = hits.hN.reshape(3, -1), hits.hT.reshape(3, -1)
        want = host(R.SssSampler.sampleDiffuseDirection(gpu, dev(rx), dev(ry), dev(np.ascontiguousarray(Nf)),
                                                        dev(np.ascontiguousarray(Tf))))
        e = elements[df["point"]]
        cases.assert_same_bits(df["dir"], want[:, e], "dir")
        nd = ((Nf[0, e] * df["dir"][0] + Nf[1, e] * df["dir"][1]).astype(F) + Nf[2, e] * df["dir"][2]).astype(F)
        clamp = np.minimum(np.maximum(nd, F(0)), F(1))
        cases.assert_same_bits(df["weight"], clamp, "weight = CLAMP(N . dir, 0, 1)")
        # one ray per listed hit unless the weight is 0, in list order
        nd_all = ((Nf[0, elements] * want[0, elements] + Nf[1, elements] * want[1, elements]).astype(F)
                  + Nf[2, elements] * want[2, elements]).astype(F)
        np.testing.assert_array_equal(df["point"], np.flatnonzero(np.minimum(np.maximum(nd_all, F(0)), F(1)) != 0))
        np.testing.assert_array_equal(np.diff(df["offsets"])[:len(elements)].sum(), df["count"])
        assert df["count"] > 100
    finally:
        gpu.set_math_mode(False)


def assert_documented_composition(gpu, hits, lights, hit_spp_n, seed=17):
    """E_c = direct_c + (radiance_c * weight) * AI_ONEOVERPI in float32 in that order, bit for bit; and within a float64 bound.
    The bound, as tests/trace_lights_util.assert_float64_bound derives shadow_resolve_kernel's: a light's k_l rays cost one
    rounding per product and at most k_l per sum's additions, the light's close three more (the two strategies' sums added, x
    radiance, x 1 / spp), each later light one for its addition: the direct term is within (k + 3 nl) u of the sum of its
    terms' magnitudes, k the hit's rays, u = 2^-24 (no tail here: rlGgx's two are not spent).  The diffuse term has two roundings,
    the final addition one more on everything: |E - exact| <= ((k + 3 nl + 1) M_direct + 3 M_diffuse) u to first order, taken as
    gamma_m = m u / (1 - m u) per count m.  The float64 composition uses the float32 constant AI_ONEOVERPI, as the kernel."""
    rad_l = np.array([[l.radiance[k] for k in range(3)] for l in lights], F)
    hq = hits.emit(lights, hit_spp_n, trace_diffuse=True, use_cavity_fade=True)
    sh, df, elements, _ = queues_host(hq)
    rng = np.random.default_rng(seed)
    vis = (10.0 ** rng.uniform(-8, 0, (3, sh["count"]))).astype(F)
    rad = (rng.random((3, df["count"])) * 10.0 ** rng.uniform(-4, 4, (3, df["count"]))).astype(F)
    # past the rays: NaN that nothing may read; E inside sentinels
    visd = torch.full((3, hq.shadow_capacity + 3), float("nan"), device=gpu.torch_device)
    radd = torch.full((3, hq.hit_capacity + 3), float("nan"), device=gpu.torch_device)
    visd[:, :sh["count"]] = dev(vis)
    radd[:, :df["count"]] = dev(rad)
    E = host(hq.resolve(visd, radd))
    shape = (hits.max_hits, hits.stride)
    want = compose_E(sh, df, elements, shape, vis, rad_l, hit_spp_n * hit_spp_n, rad)
    assert np.isfinite(E).all()
    _assert_E(E, want, elements, "numpy float32 composition")
    e64 = compose_E(sh, df, elements, shape, vis, rad_l, hit_spp_n * hit_spp_n, rad, dtype=np.float64)
    listed = len(elements)
    k = np.diff(sh["offsets"])[:listed].astype(np.float64)
    mdir = compose(dict(sh, wd=np.abs(sh["wd"])), vis, np.abs(rad_l), hit_spp_n * hit_spp_n, dtype=np.float64)[0][:, :listed]
    mdif = np.zeros((3, listed))
    mdif[:, df["point"]] = np.abs(rad.astype(np.float64)) * df["weight"].astype(np.float64)[None, :] * float(U.INV_PI)
    u = 2.0 ** -24
    gamma = lambda m: m * u / (1 - m * u)
    bound = gamma(k + 3 * len(lights) + 1)[None, :] * mdir + gamma(3.0) * mdif + 1e-44
    err = np.abs(E.reshape(3, -1)[:, elements].astype(np.float64) - e64.reshape(3, -1)[:, elements])
    assert np.all(err <= bound), float((err / bound).max())
    return dict(hq=hq, sh=sh, df=df, elements=elements, rng=rng, vis=vis, rad=rad, visd=visd, radd=radd, E=E, shape=shape,
                rad_l=rad_l, listed=listed)


def test_coloured_visibility_and_radiance_follow_the_documented_composition(gpu, oracle, T):
    """assert_documented_composition at hit_spp_n = 2 under the eight lights; then non-finite values"""
    _, lights = _lights(oracle, LIGHTS)
    hits = Hits(T, gpu)
    hit_spp_n = 2
    r = assert_documented_composition(gpu, hits, lights, hit_spp_n)
    hq, sh, df, elements, rng, vis, rad = (r[k] for k in ("hq", "sh", "df", "elements", "rng", "vis", "rad"))
    visd, radd, E, shape, rad_l, listed = (r[k] for k in ("visd", "radd", "E", "shape", "rad_l", "listed"))
    # a non-finite visibility or radiance stays in its hit
    vis2, rad2 = vis.copy(), rad.copy()
    bad_s, bad_d = rng.choice(sh["count"], 9, replace=False), rng.choice(df["count"], 5, replace=False)
    vis2[rng.integers(0, 3, 9), bad_s] = np.array([np.nan, np.inf, -np.inf], F)[np.arange(9) % 3]
    rad2[rng.integers(0, 3, 5), bad_d] = np.array([np.inf, np.nan], F)[np.arange(5) % 2]
    visd[:, :sh["count"]] = dev(vis2)
    radd[:, :df["count"]] = dev(rad2)
    E2 = host(hq.resolve(visd, radd)).reshape(3, -1)
    dirty = np.zeros(listed, bool)
    dirty[sh["point"][bad_s]] = True
    dirty[df["point"][bad_d]] = True
    clean = elements[~dirty]
    assert _bytes_equal(E2[:, clean], E.reshape(3, -1)[:, clean])
    assert not np.isfinite(E2[:, elements[dirty]]).all(axis=0).any()
    U.same_bits_or_both_nan(E2.reshape(3, *shape), compose_E(sh, df, elements, shape, vis2, rad_l, hit_spp_n * hit_spp_n, rad2),
                            "non-finite")


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_end_to_end_through_the_scatter_resolve(gpu, oracle, T, kind):
    """probes through the analytic plane / sphere (orc_scene_trace), one spherical light, unit visibility, no diffuse ray: our E
    into rls_trace_sss_scatter_resolve against the host composition with E from rls_ggx_direct_lighting's direct_diffuse"""
    from test_gpu_trace_sss import _scene_pair, _setting
    n, spp_n, hit_spp_n = N_PTS, SPP_N, 2
    case, kw, has_dPdu = _setting(kind, n)
    so, _ = _scene_pair(use_cavity_fade=True, **kw)
    s = _sss(gpu, case, has_dPdu)
    P = dev(case["P"])
    pq = T.sss_probe_rays(s, P, spp_n, SEED)
    cnt, hP, hN = U.trace_queue(so, host(pq.origin), host(pq.dir), host(pq.maxdist))
    _, lights = _lights(oracle, [dict(ONE_LIGHT, center=(0.8, -0.1, 2.5))])
    hT = orthogonal_tangent(hN.reshape(3, -1), 5).reshape(hN.shape)
    hq = T.sss_hit_rays(s, P, pq, dev(cnt), dev(hP), dev(hN), lights, hit_spp_n, SEED, hitT=dev(hT), use_cavity_fade=True,
                        hit_first_index=77)
    E = hq.resolve(_ones(gpu, hq.shadow_count))
    assert hq.hit_count > n
    got, dgot = pq.resolve(dev(cnt), dev(hP), dev(hN), E, use_cavity_fade=True, want_depth=True)
    Nf = dev(np.ascontiguousarray(hN.reshape(3, -1)))
    g = R.GgxSampler(gpu, Nf, Nf, dev(np.ascontiguousarray(hT.reshape(3, -1))), specColor=(0.9, 0.5, 0.3), ior=1.45, roughness=0.3)
    dd, _ = g.directLighting(dev(np.ascontiguousarray(hP.reshape(3, -1))), lights, hit_spp_n, SEED, KdColor=(1.0, 1.0, 1.0), Kd=1.0,
                             diffuseRoughness=0.0, Ks=0.5, first_index=77)
    Eref = host(dd).reshape(hP.shape)
    assert np.any(Eref != 0)
    want, dwant = U.host_resolve(case, spp_n * spp_n, cnt, hP, hN, Eref, 2, True, False, has_dPdu=has_dPdu)
    cases.assert_same_bits(host(got), want, (kind, "result"))
    cases.assert_same_bits(host(dgot), dwant, (kind, "mean_depth"))
    assert np.any(want != 0)


def test_end_to_end_through_the_skin_resolve(gpu, oracle, T):
    """the rlSkin node on the plane: the sss AOV with E from the hit verbs is the sss AOV with E from rls_ggx_direct_lighting"""
    from test_gpu_trace_skin import Skin, _mk_lights, _resolve, _traced
    n, spp_n, hit_spp_n = N_PTS, SPP_N, 2
    b = Skin(gpu, oracle, n, "plane", cavity=True)
    node_lights = _mk_lights([ONE_LIGHT])
    q = b.emit(T, node_lights, spp_n)
    cnt, hP, hN, _ = b.hits(q)
    p = b.p
    dv = lambda v: dev(v) if isinstance(v, np.ndarray) else v
    s = R.SssSampler(gpu, dev(b.frame[1]), dev(b.frame[2]), dv(p["sss_color"]), dv(p["sss_scatter_dist"]),
                     multiplier=dv(p["sss_dist_multiplier"]))
    _, lights = _lights(oracle, [dict(ONE_LIGHT, center=(0.2, -0.1, 2.5))])
    hT = orthogonal_tangent(hN.reshape(3, -1), 6).reshape(hN.shape)
    hq = T.sss_hit_rays(s, b.P, q.probes, dev(cnt), dev(hP), dev(hN), lights, hit_spp_n, SEED, hitT=dev(hT), use_cavity_fade=True)
    E = host(hq.resolve(_ones(gpu, hq.shadow_count)))
    assert hq.hit_count > n // 2
    Nf = dev(np.ascontiguousarray(hN.reshape(3, -1)))
    g = R.GgxSampler(gpu, Nf, Nf, dev(np.ascontiguousarray(hT.reshape(3, -1))), specColor=(0.9, 0.5, 0.3), ior=1.45, roughness=0.3)
    dd, _ = g.directLighting(dev(np.ascontiguousarray(hP.reshape(3, -1))), lights, hit_spp_n, SEED, KdColor=(1.0, 1.0, 1.0), Kd=1.0,
                             diffuseRoughness=0.0, Ks=0.5)
    Eref = host(dd).reshape(hP.shape)
    traced = _traced(gpu, q, (1.0, 1.0, 1.0))
    got = _resolve(b, q, traced, (cnt, hP, hN, E))
    want = _resolve(b, q, traced, (cnt, hP, hN, Eref))
    U.same_bits_or_both_nan(got["sss"], want["sss"], "sss AOV")
    assert np.any(want["sss"] != 0)


# ---- 6. edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,max_hits", [(2047, 1), (2048, 1), (2049, 1), (1400, 3)])
def test_list_lengths_at_the_scan_tile(gpu, oracle, T, n, max_hits):
    """spp_n = 1 and every ray with max_hits shaded hits: the list is n * max_hits long -- one below, at and one above the
    scan's tile of 2048 entries, and two tiles of rays with a carry -- and every offset is the host's int64 cumsum"""
    _, lights = _lights(oracle, [ONE_LIGHT, dict(LIGHTS[1])])
    hits = Hits(T, gpu, n=n, spp_n=1, max_hits=max_hits, pad=0, dense=True)
    keep = gate_np(hits.case, 1, hits.cnt, hits.hP, hits.hN, max_hits, False)
    el = listed_elements(keep, hits.stride)
    assert len(el) == n * max_hits
    hq = hits.emit(lights, 1, trace_diffuse=True)
    sh, df, elements, count = queues_host(hq)
    np.testing.assert_array_equal(elements, el)
    assert count == len(el)
    per_hit = np.bincount(sh["point"], minlength=hq.hit_capacity)
    np.testing.assert_array_equal(sh["offsets"], np.concatenate([[0], np.cumsum(per_hit, dtype=np.int64)]))
    per_hit_d = np.bincount(df["point"], minlength=hq.hit_capacity)
    np.testing.assert_array_equal(df["offsets"], np.concatenate([[0], np.cumsum(per_hit_d, dtype=np.int64)]))
    assert per_hit.max() <= 4 and per_hit_d.max() == 1 and sh["count"] > n // 4
    E = host(hq.resolve(_ones(gpu, sh["count"]), _ones(gpu, df["count"])))
    rad_l = np.array([[l.radiance[k] for k in range(3)] for l in lights], F)
    want = compose_E(sh, df, elements, (max_hits, hits.stride), np.ones((3, sh["count"]), F), rad_l, 1,
                     np.ones((3, df["count"]), F))
    _assert_E(E, want, el, (n, max_hits))


def test_hit_capacity_one_below_the_shaded_count(gpu, oracle, T):
    _, lights = _lights(oracle, LIGHTS[:3])
    hits = Hits(T, gpu)
    el = hits.elements(True)
    cap = len(el) - 1
    full = hits.emit(lights, 2, trace_diffuse=True, use_cavity_fade=True)
    fs, fd, _, _ = queues_host(full)
    hq = T.HitQueues(gpu, hits.n, hits.spp_n, hits.max_hits, hits.stride, cap, 3, 2, True)
    # sentinels past every capacity: the tensors are views into larger ones
    guard = {}
    for name in ("_hit_element", "_smaxdist", "_skind", "_spoint", "_ssample", "_dpoint"):
        t = getattr(hq, name)
        big = torch.full((t.numel() + 16,), 85, dtype=t.dtype, device=t.device)
        guard[name] = big
        setattr(hq, name, big[:t.numel()])
    hq.q.hit_element = hq._hit_element.data_ptr()
    hq.q.shadow.maxdist, hq.q.shadow.kind = hq._smaxdist.data_ptr(), hq._skind.data_ptr()
    hq.q.shadow.point, hq.q.shadow.sample = hq._spoint.data_ptr(), hq._ssample.data_ptr()
    hq.q.diffuse.point = hq._dpoint.data_ptr()
    hits.emit(lights, 2, trace_diffuse=True, use_cavity_fade=True, queues=hq, hit_capacity=cap)
    sh, df, elements, count = queues_host(hq)
    assert count == len(el) and hq.listed == cap                    # the TRUE count
    np.testing.assert_array_equal(elements, el[:cap])
    for name, big in guard.items():
        assert torch.all(big[-16:] == 85), name
    lo = int(fs["offsets"][cap])
    np.testing.assert_array_equal(sh["offsets"], fs["offsets"][:cap + 1])
    assert sh["count"] == lo and df["count"] == int(fd["offsets"][cap])
    for k in ("dir", "maxdist", "wd", "kind", "point", "sample"):
        assert _bytes_equal(sh[k], fs[k][..., :lo]), k
    E = host(hq.resolve(_ones(gpu, sh["count"]), _ones(gpu, df["count"])))
    Efull = host(full.resolve(_ones(gpu, fs["count"]), _ones(gpu, fd["count"]))).reshape(3, -1).copy()
    Efull[:, el[cap]] = 0                                            # the hit that did not fit is not shaded
    _assert_E(E, Efull.reshape(E.shape), el[:cap], "overflow")
    # capacity 0: the count alone
    h0 = hits.emit(lights, 2, trace_diffuse=True, use_cavity_fade=True, hit_capacity=0)
    assert h0.hit_count == len(el) and h0.shadow_count == 0 and h0.diffuse_count == 0
    assert not host(h0.resolve(_ones(gpu, 1), _ones(gpu, 1))).view(np.uint32).any()


def test_exact_scratch_inside_sentinels(gpu, oracle, T):
    _, lights = _lights(oracle, LIGHTS[:2])
    hits = Hits(T, gpu)
    cap = hits.max_hits * hits.n * hits.spp
    need = T.sss_hits_scratch_bytes(hits.n, hits.spp_n, hits.max_hits, cap, 2, 3)
    big = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=gpu.torch_device)
    hq = T.HitQueues(gpu, hits.n, hits.spp_n, hits.max_hits, hits.stride, cap, 2, 3, True, scratch=big[256:256 + need])
    hits.emit(lights, 3, trace_diffuse=True, queues=hq)
    ref = hits.emit(lights, 3, trace_diffuse=True)
    a, b = queues_host(hq), queues_host(ref)
    for k in a[0]:
        assert _bytes_equal(a[0][k], b[0][k]), k
    assert torch.all(big[:256] == 0xA5) and torch.all(big[256 + need:] == 0xA5)
    x = T.HitQueues_.from_buffer_copy(hq.q)
    x.scratch_bytes = need - 1
    d = hits.d
    h = T._probe_hits(d["cnt"], d["hP"], d["hN"], None, hits.pq.count)
    la, nl = R.closures.light_array(lights)
    st = T.load().rls_trace_sss_hits_emit(gpu.handle, hits.n, C.byref(hits.s.c), R.closures.cvec3(hits.P, hits.n, "P"), hits.spp_n,
                                          C.byref(hits.pq.q), C.byref(h), T.capi.CVec3(None, None, None), 0, la, nl, 3, 1, SEED, 0,
                                          C.byref(x))
    assert st == INVALID and b"scratch" in R.load().rls_last_error()


@pytest.mark.parametrize("diffuse", [False, True], ids=["nodiffuse", "diffuse"])
def test_no_lights(gpu, oracle, T, diffuse):
    hits = Hits(T, gpu)
    el = hits.elements(False)
    hq = hits.emit(None, 2, trace_diffuse=diffuse)
    _, df, elements, count = queues_host(hq)
    np.testing.assert_array_equal(elements, el)
    assert count == len(el)
    rad = np.random.default_rng(2).random((3, max(df["count"], 1))).astype(F)
    E = host(hq.resolve(None, dev(rad) if diffuse else None))
    sh0 = dict(offsets=np.zeros(hq.hit_capacity + 1, np.int64), count=0)
    want = compose_E(sh0, df, elements, (hits.max_hits, hits.stride), None, np.zeros((0, 3), F), 4, rad if diffuse else None)
    _assert_E(E, want, el, ("no lights", diffuse))
    assert diffuse == bool(np.any(E != 0))


def test_two_halves_of_the_rays_equal_one_call(gpu, oracle, T):
    """the rays of the first 33 points, then of the other 34, with hit_first_index advanced by the first half's rays: the hit
    planes are sliced by ray, so element k * stride' + j' of a half is element k * stride + j of the whole at a constant shift
    of j; the samples follow hit_first_index + element"""
    _, lights = _lights(oracle, LIGHTS[:3])
    hits = Hits(T, gpu, pad=0)
    whole = hits.emit(lights, 2, trace_diffuse=True, use_cavity_fade=True, first=1000)
    ws, wdf, wel, _ = queues_host(whole)
    Ew = host(whole.resolve(_ones(gpu, ws["count"]), _ones(gpu, wdf["count"])))
    # a half's own planes of stride = the whole's: its elements are then the whole's, shifted by its first ray
    for a, e in ((0, 33), (33, hits.n)):
        ra, re_ = a * hits.spp, e * hits.spp
        sub = {k: np.ascontiguousarray(v[..., a:e]) for k, v in hits.case.items()}
        s = _sss(gpu, sub)
        P = dev(sub["P"])
        pq = T.sss_probe_rays(s, P, hits.spp_n, SEED)
        shift = lambda v: np.ascontiguousarray(np.concatenate([v[..., ra:], v[..., :ra]], axis=-1))
        cnt, hP, hN, hT = shift(hits.cnt), shift(hits.hP), shift(hits.hN), shift(hits.hT)
        hq = T.sss_hit_rays(s, P, pq, dev(cnt), dev(hP), dev(hN), lights, 2, SEED, hitT=dev(hT), use_cavity_fade=True,
                            trace_diffuse=True, hit_first_index=1000 + ra)
        sh, df, el, _ = queues_host(hq)
        inside = ((wel % hits.stride) >= ra) & ((wel % hits.stride) < re_)
        np.testing.assert_array_equal(el + ra, wel[inside])
        idx = np.flatnonzero(inside)
        lo, hi = int(ws["offsets"][idx[0]]), int(ws["offsets"][idx[-1] + 1])
        for k in ("dir", "maxdist", "wd", "kind", "sample"):
            assert _bytes_equal(sh[k], ws[k][..., lo:hi]), (a, k)
        E = host(hq.resolve(_ones(gpu, sh["count"]), _ones(gpu, df["count"]))).reshape(3, -1)
        assert _bytes_equal(E[:, el], Ew.reshape(3, -1)[:, wel[inside]]), a


def test_emit_and_resolve_in_a_graph(oracle, T):
    _, lights = _lights(oracle, LIGHTS[:3])
    gctx = R.Context(0, use_torch_stream=False)          # the context's own stream: the NULL stream cannot be captured
    try:
        hits = Hits(T, gctx)
        gctx.synchronize()
        torch.cuda.synchronize()
        direct = hits.emit(lights, 2, trace_diffuse=True, use_cavity_fade=True)
        gctx.synchronize()
        ds, dd, del_, dcount = queues_host(direct)
        rng = np.random.default_rng(4)
        vis, rad = dev(rng.random((3, ds["count"])).astype(F)), dev(rng.random((3, dd["count"])).astype(F))
        torch.cuda.synchronize()
        want = direct.resolve(vis, rad)
        gctx.synchronize()
        want = host(want)
        hq = T.HitQueues(gctx, hits.n, hits.spp_n, hits.max_hits, hits.stride, direct.hit_capacity, 3, 2, True)
        out = gctx.empty(3, hits.max_hits, hits.stride)
        torch.cuda.synchronize()
        with gctx.capture() as g:
            hits.emit(lights, 2, trace_diffuse=True, use_cavity_fade=True, queues=hq)
            hq.resolve(vis, rad, out=out, counts=(ds["count"], dd["count"]))
        out.fill_(-1.0)
        hq._hit_count.zero_()
        hq.shadow_offsets.zero_()
        torch.cuda.synchronize()
        g.launch()
        gctx.synchronize()
        g.close()
        qs, qd, qel, qcount = queues_host(hq)
        assert qcount == dcount and np.array_equal(qel, del_)
        for k in ds:
            assert _bytes_equal(qs[k], ds[k]), k
        for k in dd:
            assert _bytes_equal(qd[k], dd[k]), k
        cases.assert_same_bits(host(out), want, "replay")
    finally:
        gctx.close()


def test_argument_checks(gpu, oracle, T):
    lib = T.load()
    _, lights = _lights(oracle, LIGHTS[:2])
    hits = Hits(T, gpu)
    d = hits.d
    n, nl, hit_spp_n = hits.n, 2, 2
    hq = hits.emit(lights, hit_spp_n, trace_diffuse=True)
    gpu.synchronize()
    la = (R._capi.SphereLight * 9)(*(list(lights) + [lights[0]] * 7))
    Pv = R.closures.cvec3(hits.P, n, "P")
    noT = T.capi.CVec3(None, None, None)
    vis, rad = _ones(gpu, hq.shadow_capacity), _ones(gpu, hq.hit_capacity)
    vc, rc = (T.capi.CRgb(*[t[k].data_ptr() for k in range(3)]) for t in (vis, rad))
    E = gpu.empty(3, hits.max_hits, hits.stride)
    Ec = T.capi.Rgb(*[E[k].data_ptr() for k in range(3)])

    def H(**kw):
        h = T._probe_hits(d["cnt"], d["hP"], d["hN"], None, hits.pq.count)
        for k, v in kw.items():
            setattr(h, k, v)
        return h

    def Q(**kw):
        x = T.HitQueues_.from_buffer_copy(hq.q)
        for k, v in kw.items():
            obj, _, field = k.rpartition("__")
            setattr(getattr(x, obj) if obj else x, field, v)
        return x

    def emit(x=None, h=None, lights_n=nl, spp=hit_spp_n, la=la, hitT=noT, diffuse=1, probe_spp=hits.spp_n):
        x = Q() if x is None else x
        h = H() if h is None else h
        return lib.rls_trace_sss_hits_emit(gpu.handle, n, C.byref(hits.s.c), Pv, probe_spp, C.byref(hits.pq.q),
                                           C.byref(h) if h is not False else None, hitT, 0, la, lights_n, spp, diffuse, SEED, 0,
                                           C.byref(x) if x is not False else None)

    def resolve(x=None, h=None, lights_n=nl, spp=hit_spp_n, v=vc, r=rc, o=Ec, diffuse=1):
        x = Q() if x is None else x
        h = H() if h is None else h
        return lib.rls_trace_sss_hits_resolve(gpu.handle, C.byref(h) if h is not False else None, la, lights_n, spp, diffuse,
                                              C.byref(x) if x is not False else None, v, r, o)

    err = lambda: R.load().rls_last_error()
    assert emit() == 0 and resolve() == 0
    gpu.synchronize()
    before = [t.clone() for t in (hq._hit_count, hq._hit_element, hq.shadow_offsets, hq._sdir, hq._swd, hq.diffuse_offsets, E)]
    # NULL planes
    for k in ("count",):
        assert emit(h=H(**{k: None})) == INVALID and b"hits" in err()
    bad = H()
    bad.P.y = None
    assert emit(h=bad) == INVALID
    bad = H()
    bad.N.z = None
    assert emit(h=bad) == INVALID
    assert emit(h=False) == INVALID and resolve(h=False) == INVALID and emit(x=False) == INVALID and resolve(x=False) == INVALID
    for k in ("hit_count", "hit_element", "shadow__offsets", "shadow__maxdist", "shadow__kind", "diffuse__offsets", "scratch"):
        assert emit(Q(**{k: None})) == INVALID, k
    for k in ("hit_count", "hit_element", "shadow__offsets", "shadow__kind", "diffuse__offsets"):
        assert resolve(Q(**{k: None})) == INVALID, k
    x = Q()
    x.shadow.dir.y = None
    assert emit(x) == INVALID
    x = Q()
    x.shadow.weight_diffuse.r = None
    assert emit(x) == INVALID and resolve(x) == INVALID
    x = Q()
    x.diffuse.weight.r = None
    assert emit(x) == INVALID and resolve(x) == INVALID
    assert emit(x, diffuse=0) == 0                                   # the diffuse queue is not read without trace_diffuse
    x = Q()
    x.diffuse.dir.z = None
    assert emit(x) == INVALID
    assert emit(hitT=T.capi.CVec3(d["hT"][0].data_ptr(), None, d["hT"][2].data_ptr())) == INVALID and b"hitT" in err()
    # max_hits, capacities, hit_spp_n, the lights: the sibling verbs' codes and words
    for mh in (0, 13):
        assert emit(h=H(max_hits=mh)) == INVALID and b"max_hits" in err()
        assert resolve(h=H(max_hits=mh)) == INVALID and b"max_hits" in err()
    assert emit(h=H(stride=n * hits.spp - 1)) == INVALID and b"stride" in err()
    cap = hq.hit_capacity
    assert emit(Q(shadow__capacity=cap * nl * 2 * hit_spp_n * hit_spp_n - 1)) == INVALID and b"capacity" in err()
    assert resolve(Q(shadow__capacity=cap * nl * 2 * hit_spp_n * hit_spp_n - 1)) == INVALID and b"capacity" in err()
    assert emit(Q(diffuse__capacity=cap - 1)) == INVALID and b"capacity" in err()
    assert emit(Q(hit_capacity=-1)) == INVALID and b"hit_capacity" in err()
    assert hq.q.scratch_bytes == T.sss_hits_scratch_bytes(n, hits.spp_n, hits.max_hits, cap, nl, hit_spp_n)
    assert emit(Q(scratch_bytes=hq.q.scratch_bytes - 1)) == INVALID and b"scratch" in err()
    for spp in (0, 17):
        assert emit(spp=spp) == INVALID and b"hit_spp_n" in err()
        assert resolve(spp=spp) == INVALID and b"hit_spp_n" in err()
        assert emit(probe_spp=spp) == INVALID and b"spp_n" in err()
    for bad_n in (-1, 9):
        assert emit(lights_n=bad_n) == INVALID and b"n_lights" in err()
        assert resolve(lights_n=bad_n) == INVALID and b"n_lights" in err()
    assert emit(la=None) == INVALID and b"lights" in err()
    wrong = list(lights)
    wrong[1] = R._capi.SphereLight.from_buffer_copy(bytes(lights[1]))
    wrong[1].radius = 0.0
    assert emit(la=(R._capi.SphereLight * 2)(*wrong)) == INVALID and b"radius" in err()
    wrong[1].radius, wrong[1].mis_mode = 1.0, 3
    assert emit(la=(R._capi.SphereLight * 2)(*wrong)) == INVALID and b"mis_mode" in err()
    assert resolve(v=T.capi.CRgb(vis[0].data_ptr(), None, vis[2].data_ptr())) == INVALID and b"visibility" in err()
    assert resolve(r=T.capi.CRgb(None, None, None)) == INVALID and b"radiance" in err()
    assert resolve(r=T.capi.CRgb(None, None, None), diffuse=0) == 0
    assert resolve(o=T.capi.Rgb(E[0].data_ptr(), None, E[2].data_ptr())) == INVALID
    b = C.c_size_t()
    sb = lib.rls_trace_sss_hits_scratch_bytes
    assert sb(n, 2, 3, cap, 2, 2, None) == INVALID
    for args in ((-1, 2, 3, cap, 2, 2), (n, 0, 3, cap, 2, 2), (n, 17, 3, cap, 2, 2), (n, 2, 0, cap, 2, 2), (n, 2, 13, cap, 2, 2),
                 (n, 2, 3, -1, 2, 2), (n, 2, 3, cap, -1, 2), (n, 2, 3, cap, 9, 2), (n, 2, 3, cap, 2, 0), (n, 2, 3, cap, 2, 17)):
        assert sb(*args, C.byref(b)) == INVALID, args
    assert sb(n, 2, 3, cap, 0, 2, C.byref(b)) == 0 and sb(0, 2, 3, 0, 0, 1, C.byref(b)) == 0
    gpu.synchronize()
    # a refused call writes nothing (the valid calls in between rewrote the same values)
    after = (hq._hit_count, hq._hit_element, hq.shadow_offsets, hq._sdir, hq._swd, hq.diffuse_offsets, E)
    assert emit() == 0 and resolve() == 0
    gpu.synchronize()
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t     # (planes past the rays were never written)
    for t, was in zip(after, before):
        assert torch.equal(bits(t), bits(was))
    # n = 0: an empty list, empty queues
    q0 = T.ProbeQueue(gpu, 0, 2)
    h0 = T.HitQueues(gpu, 0, 2, 3, 0, 4, nl, hit_spp_n, True)
    h0._hit_count.fill_(-1)
    h0.shadow_offsets.fill_(-1)
    h0.diffuse_offsets.fill_(-1)
    e = T.ProbeHits_()
    e.max_hits, e.stride = 3, 0
    st = lib.rls_trace_sss_hits_emit(gpu.handle, 0, C.byref(hits.s.c), T.capi.CVec3(None, None, None), 2, C.byref(q0.q), C.byref(e),
                                     noT, 0, la, nl, hit_spp_n, 1, SEED, 0, C.byref(h0.q))
    assert st == 0 and h0.hit_count == 0 and h0.shadow_count == 0 and h0.diffuse_count == 0
    assert not host(h0.shadow_offsets).any() and not host(h0.diffuse_offsets).any()
