"""GPU: the caller-traced rlSkin node (include/rlshaders_amd_trace.h, rls_trace_skin_emit / rls_trace_skin_resolve;
rlshaders_amd/trace.py, skin_node_rays).

The emit fills five queues -- per GGX lobe the light loop's shadow rays and integrateGlossy's rays, then integrateScatter's
probe rays -- and the three hand-down scalars; one resolve composes rls_skin_integrate's AOVs.  Checked here:
  1. the contract, bit for bit: visibility 1 on every shadow ray, one radiance env on every glossy ray and the probe rays
     traced through the analytic plane or sphere with E = light_irradiance(...) give rls_skin_integrate(env, scene, lights) in
     sheen, specular, sss, out, sheenFresnel, specularFresnel and sssWeight: EXACT and FAST, spp_n 1, 2, 3, 7, 16, every
     lane-group width and the host's pick, 0 / 1 / 2 / 8 lights with the three mis_modes mixed, a light below the horizon and
     one around P, uniform parameters, cavity fade and literal_matrix on and off, n = 1, 5, 67, kBlock + 1, first_index past
     2^36, one shared scratch block;
  2. the gates: lobe weights at and below AI_EPSILON, black lobe colours (the light loop still feeds the mean Fresnel, the
     glossy queue is empty), sssWeight below AI_EPSILON (probes with maxdist 0, sss exactly 0, garbage hits ignored);
  3. the queues: the sheen glossy queue is rls_trace_ggx_glossy_emit's for a rlGgx closure with the lobe's parameters (stream
     pair 0); the shadow queues' CSR invariants, order, kind bits, directions inside the cone and maxdist against float64;
  4. non-uniform visibility and radiance against the header's composition in numpy: the light and scatter parts bit for bit,
     the glossy sums within the header's float64 bound carried through the layer products (see _bound);
  5. a non-finite visibility or radiance poisons its point alone; chunked emits reproduce the unchunked queues; a captured graph
     of emit plus resolve replays the same bits."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import cases
import rlshaders_amd as R
import trace_sss_util as U
from gpu_util import dev, host
from test_gpu_loop_edges import LIGHTS as LIGHTS8
from test_gpu_shade import LIGHTS as LIGHTS2

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KBLOCK = int(re.search(r"#define RLS_BLOCK (\d+)", (ROOT / "rlshaders_amd" / "csrc" / "rls_internal.hpp").read_text()).group(1))
KEYS = ("sheen", "specular", "sss", "out", "sheenFresnel", "specularFresnel", "sssWeight")
EPS = np.float32(1e-4)
SEED = 23
F = np.float32


@pytest.fixture(scope="module")
def T():
    from rlshaders_amd import build, trace
    build.build_trace_library()
    trace.load()
    return trace


def _at(monkeypatch, g, fn):
    if g is None:
        monkeypatch.delenv("RLS_INTEGRATE_GROUP", raising=False)
    else:
        monkeypatch.setenv("RLS_INTEGRATE_GROUP", str(g))
    try:
        return fn()
    finally:
        monkeypatch.delenv("RLS_INTEGRATE_GROUP", raising=False)


def _mk_lights(specs):
    return [R.make_light(**s) for s in specs] if specs else None


class Skin:
    """the first n points of cases.skin_mixed on the unit sphere (P = N) or on the plane z = 0, with the scene of
    tests/test_gpu_skin_integrate.py"""

    def __init__(self, gpu, oracle, n, geometry="plane", cavity=False, literal=False, params=None, a=0, full=None,
                 materials=None, case=None):
        """case: the caller's own points on the plane z = 0 instead -- dict(wo, N, T, P [3, n], params), numpy"""
        m = max(a + n, 64) if full is None else full
        c = cases.skin_mixed(cases.SEED_PARITY, m)
        sl = lambda v: np.ascontiguousarray(np.asarray(v)[..., a:a + n])
        p = {k: sl(v) for k, v in c["params"].items()}
        if geometry == "sphere":
            self.kw = dict(geometry="sphere", sphere_radius=1.0, light_dir=(0.0, 0.6, 0.8), use_cavity_fade=cavity,
                           literal_matrix=literal)
            wo, N, Tt = sl(c["wo"]), sl(c["N"]), sl(c["T"])
            P = N.copy()
        else:
            self.kw = dict(geometry="plane", plane_normal=(0.0, 0.0, 1.0), light_dir=(0.0, 0.6, 0.8), use_cavity_fade=cavity,
                           literal_matrix=literal, gate_point=(0.1, 0.0, 0.0), gate_normal=(1.0, 0.0, 0.0))
            P = np.zeros((3, m), F)
            P[:2] = np.stack([oracle.gen_uniform(SEED, 0, m, 40 + j, -0.5, 0.5) for j in range(2)])
            P = sl(P)
            N = np.tile(np.array([[0.0], [0.0], [1.0]], F), (1, n))
            Tt = np.tile(np.array([[1.0], [0.0], [0.0]], F), (1, n))
            wo = cases.frame(cases.SEED_PARITY, m)[0]
            wo[2] = np.abs(wo[2]) + 0.05
            wo = sl((wo / np.linalg.norm(wo, axis=0, keepdims=True)).astype(F))
        if params is not None:
            p = params(p, n) if callable(params) else params
        if case is not None:
            assert geometry == "plane"
            wo, N, Tt, P, p = case["wo"], case["N"], case["T"], case["P"], case["params"]
        self.n, self.gpu, self.oracle, self.cavity, self.literal = n, gpu, oracle, cavity, literal
        self.Ph, self.p = P, p
        self.P = dev(P)
        self.frame = (wo, N, Tt)
        # materials: (ids int32 [n], count): the parameters are per-material columns looked up by id (rls_material_index)
        mat = None if materials is None else (dev(materials[0]), materials[1])
        self.sk = R.SkinShader(gpu, dev(wo), dev(N), dev(Tt), materials=mat,
                               **{k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in p.items()})
        self.scene = R.make_scene(**self.kw)
        self.oscene = oracle.make_scene(**self.kw)

    def analytic(self, lights, spp_n, seed=SEED, first=0, env=(1.0, 1.0, 1.0)):
        out = self.sk.integrate(self.P, self.scene, spp_n, seed, env=env, first_index=first, lights=lights)
        return {k: host(v) for k, v in out.items()}

    def emit(self, T, lights, spp_n, seed=SEED, first=0, queues=None, share=False):
        return T.skin_node_rays(self.sk, self.P, lights, spp_n, seed, first, queues=queues, share_scratch=share)

    def hits(self, q, stride=None):
        """the probe queue traced through the analytic scene on the host -> (count, P, N, E) on the device"""
        pq = q.probes
        o, d, md = host(pq.origin), host(pq.dir), host(pq.maxdist)
        if self.kw["geometry"] == "plane":
            cnt, hP, hN = U.trace_plane_np((0.0, 0.0, 0.0), self.kw["plane_normal"], o, d, md)
        else:
            cnt, hP, hN = U.trace_queue(self.oscene, o, d, md, stride)
        E = U.light_irradiance(self.oscene, hP, hN)
        return cnt, hP, hN, E


def _traced(gpu, q, env, cnt=None):
    cnt = q.counts() if cnt is None else cnt
    ones = lambda k: torch.ones(3, max(cnt[k], 1), dtype=torch.float32, device=gpu.torch_device)
    L = lambda k: (ones(k) * torch.tensor(env, dtype=torch.float32, device=gpu.torch_device)[:, None]).contiguous()
    vis = (ones("sheen_shadow"), ones("specular_shadow")) if q.n_lights > 0 else (None, None)
    return vis[0], vis[1], L("sheen_glossy"), L("specular_glossy")


def _resolve(b, q, traced, hits, **kw):
    cnt, hP, hN, E = hits
    out = q.resolve(*traced, dev(cnt), dev(hP), dev(hN), dev(E), use_cavity_fade=b.cavity, literal_matrix=b.literal, **kw)
    return {k: host(v) for k, v in out.items()}


def _same(got, want, what):
    for k in KEYS:
        U.same_bits_or_both_nan(got[k], want[k], (what, k))


def _contract(T, b, lights, spp_n, first=0, env=(1.0, 1.0, 1.0), share=False, what=None):
    want = b.analytic(lights, spp_n, first=first, env=env)
    q = b.emit(T, lights, spp_n, first=first, share=share)
    got = _resolve(b, q, _traced(b.gpu, q, env), b.hits(q))
    _same(got, want, (what, b.n, spp_n, first, env))
    # the scalars are the emit's own
    for k, t in (("sheenFresnel", q.sheenFresnel), ("specularFresnel", q.specularFresnel), ("sssWeight", q.sssWeight)):
        U.same_bits_or_both_nan(host(t), want[k], (what, "emit", k))
    return q, want


ENVS = ((1.0, 1.0, 1.0), (0.7, 0.8, 0.9))
# a light below the horizon of the plane's points and one around P (its cone is not valid: it draws nothing)
ODD_LIGHTS = (dict(center=(0.2, 0.1, -3.0), radius=0.8, radiance=(1.0, 2.0, 0.5), mis_mode=0),
              dict(center=(0.0, 0.0, 0.0), radius=5.0, radiance=(3.0, 1.0, 1.0), mis_mode=0),
              dict(center=(0.5, 0.5, 4.0), radius=1.0, radiance=(2.0, 1.5, 1.0), mis_mode=2))
MIXED3 = (dict(center=(0.5, 0.5, 4.0), radius=1.0, radiance=(2.0, 1.5, 1.0), mis_mode=0),
          dict(center=(-3.0, 0.0, 1.0), radius=0.7, radiance=(0.2, 0.4, 3.0), mis_mode=2),
          dict(center=(0.0, 3.0, 2.0), radius=0.9, radiance=(1.0, 0.1, 0.1), mis_mode=1))


def _lights8():
    out = []
    for k, s in enumerate(LIGHTS8):
        s = dict(s)
        s["mis_mode"] = k % 3
        out.append(s)
    return out


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("n,spp_n,first", [(1, 16, 0), (5, 7, (1 << 36) + 5), (67, 3, 0), (KBLOCK + 1, 2, (1 << 36) + 5),
                                           (67, 1, 3)])
def test_unit_rays_are_rls_skin_integrate(gpu, oracle, T, n, spp_n, first, fast):
    gpu.set_math_mode(fast)
    try:
        b = Skin(gpu, oracle, n, "plane")
        for env in ENVS:
            q, want = _contract(T, b, _mk_lights(MIXED3), spp_n, first, env, what=("fast", fast))
        if n >= 67:
            assert all(v > 0 for v in q.counts().values()), q.counts()
            assert (want["sss"] > 0).mean() > 0.2
    finally:
        gpu.set_math_mode(False)


def test_unit_rays_on_the_sphere_with_cavity_fade_and_literal_matrix(gpu, oracle, T):
    """EXACT only: trace_sss_util traces the sphere with the oracle's IEEE arithmetic, which is the EXACT integrator's; FAST
    intersects the sphere with the hardware's reciprocal and square root, which no host tracer here reproduces.  FAST runs the
    same fade and matrix cases on the plane below, where the host's trace is the integrator's in either mode."""
    for cavity, literal in ((True, False), (False, True), (True, True)):
        b = Skin(gpu, oracle, 37, "sphere", cavity, literal)
        _contract(T, b, _mk_lights(MIXED3[:2]), 3, 11, ENVS[1], what=("sphere", cavity, literal))


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_unit_rays_on_the_plane_with_cavity_fade_and_literal_matrix(gpu, oracle, T, fast):
    gpu.set_math_mode(fast)
    try:
        for cavity, literal in ((True, False), (False, True), (True, True)):
            b = Skin(gpu, oracle, 67, "plane", cavity, literal)
            q, want = _contract(T, b, _mk_lights(MIXED3[:2]), 3, 11, ENVS[1], what=("plane", cavity, literal))
            assert (want["sss"] > 0).mean() > 0.2
    finally:
        gpu.set_math_mode(False)


def test_unit_rays_at_every_group_width_and_light_count(gpu, oracle, T, monkeypatch):
    b = Skin(gpu, oracle, 131, "plane", cavity=True)
    for specs in (None, MIXED3[:1], LIGHTS2, _lights8(), ODD_LIGHTS):
        lights = _mk_lights(specs)
        for spp_n, g in ((4, 1), (4, 4), (4, 16), (8, 64), (3, 64), (5, None)):
            want = _at(monkeypatch, 1, lambda: b.analytic(lights, spp_n, env=ENVS[1]))
            q = _at(monkeypatch, g, lambda: b.emit(T, lights, spp_n, share=g == 4))
            assert (q.sheen_shadow is None) == (lights is None)
            _same(_resolve(b, q, _traced(gpu, q, ENVS[1]), b.hits(q)), want, (0 if specs is None else len(specs), spp_n, g))


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_unit_rays_uniform_parameters(gpu, oracle, T, fast):
    gpu.set_math_mode(fast)
    try:
        for name, preset in cases.SKIN_PRESETS.items():
            b = Skin(gpu, oracle, 67, "plane", params=dict(preset))
            _contract(T, b, _mk_lights(MIXED3), 3, 0, ENVS[1], what=name)
    finally:
        gpu.set_math_mode(False)


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_unit_rays_parameters_by_reference(gpu, oracle, T, fast):
    """m = 7 materials as per-material columns, a material id per point: the emit kernels, the probe emit and the resolve read
    every parameter through the table; the same points with the columns expanded per point give the same bits"""
    n, m, spp_n = 131, 7, 3
    cols = {k: np.ascontiguousarray(np.asarray(v)[..., :m]) for k, v in cases.skin_mixed(cases.SEED_EDGE, 64)["params"].items()}
    ids = ((oracle.gen_uniform(cases.SEED_PARITY, 0, n, 77) * m).astype(np.uint32) % m).astype(np.int32)
    gpu.set_math_mode(fast)
    try:
        b = Skin(gpu, oracle, n, "plane", cavity=True, params=cols, materials=(ids, m))
        q, want = _contract(T, b, _mk_lights(MIXED3), spp_n, 5, ENVS[1], what="materials")
        e = Skin(gpu, oracle, n, "plane", cavity=True, params={k: np.ascontiguousarray(v[..., ids]) for k, v in cols.items()})
        _same(e.analytic(_mk_lights(MIXED3), spp_n, first=5, env=ENVS[1]), want, "expanded")
        assert len(np.unique(want["sheenFresnel"])) > 3
    finally:
        gpu.set_math_mode(False)


def _gated(p, n):
    k = np.arange(n) % 8
    p = dict(p)
    w = lambda a, m, v: np.where(m, F(v), a).astype(F)
    p["sheen_weight"] = w(w(w(p["sheen_weight"], k == 0, 0.0), k == 1, 1e-4), k == 7, 0.5)
    p["specular_weight"] = w(w(p["specular_weight"], k == 2, 0.0), k == 3, 1e-4)
    p["sheen_color"] = np.where((k == 4)[None, :], F(0.0), p["sheen_color"]).astype(F)
    p["specular_color"] = np.where((k == 5)[None, :], F(0.0), p["specular_color"]).astype(F)
    p["sss_weight"] = w(w(p["sss_weight"], k == 6, 0.0), k == 7, 5e-5)
    return p


@pytest.mark.parametrize("lit", [False, True])
def test_gates(gpu, oracle, T, lit):
    n, spp_n = 160, 4
    b = Skin(gpu, oracle, n, "plane", params=_gated)
    k = np.arange(n) % 8
    lights = _mk_lights(MIXED3) if lit else None
    want = b.analytic(lights, spp_n, env=ENVS[1])
    q = b.emit(T, lights, spp_n)
    off = lambda qq: np.diff(host(qq.offsets))
    # a lobe whose weight is at or below AI_EPSILON has no rays at all; a black colour has no glossy rays
    assert not off(q.sheen_glossy)[(k == 0) | (k == 1) | (k == 4)].any() and off(q.sheen_glossy)[k == 6].all()
    assert not off(q.specular_glossy)[(k == 2) | (k == 3) | (k == 5)].any() and off(q.specular_glossy)[k == 6].all()
    if lit:
        # (a black lobe's terms are all 0: no shadow rays either, though its light loop draws the samples)
        assert not off(q.sheen_shadow)[(k == 0) | (k == 1) | (k == 4)].any() and off(q.sheen_shadow)[k == 6].any()
        assert not off(q.specular_shadow)[(k == 2) | (k == 3) | (k == 5)].any() and off(q.specular_shadow)[k == 6].any()
        # the light loop feeds the mean Fresnel of a black lobe
        assert (host(q.sheenFresnel)[k == 4] != b.p["sheen_weight"][k == 4]).mean() > 0.5
    else:
        assert np.array_equal(host(q.sheenFresnel)[k == 4], b.p["sheen_weight"][k == 4])     # nothing drawn: avg = 1
    assert not host(q.sheenFresnel)[(k == 0) | (k == 1)].any()
    # sssWeight below AI_EPSILON: probes with maxdist 0, and the point's hits are not read
    shut = host(q.sssWeight) < EPS
    assert shut[(k == 6) | (k == 7)].all() and not shut[k == 5].any()
    md = host(q.probes.maxdist).reshape(n, spp_n * spp_n)
    assert not md[shut].any() and md[~shut].all()
    cnt, hP, hN, E = b.hits(q)
    rays = np.repeat(shut, spp_n * spp_n)
    cnt = np.where(rays, np.uint8(255), cnt).astype(np.uint8)
    hP[:, :, rays] = np.nan
    E[:, :, rays] = np.inf
    got = _resolve(b, q, _traced(gpu, q, ENVS[1]), (cnt, hP, hN, E))
    _same(got, want, ("gates", lit))
    assert not got["sss"][:, shut].any() and not got["sheen"][:, (k == 0) | (k == 1)].any()


def test_sheen_glossy_queue_is_the_ggx_glossy_emit_of_the_lobe(gpu, oracle, T):
    n, spp_n = 131, 5
    b = Skin(gpu, oracle, n, "sphere")
    q = b.emit(T, _mk_lights(MIXED3[:1]), spp_n)
    wo, N, Tt = b.frame
    s = R.GgxSampler(gpu, dev(wo), dev(N), dev(Tt), specColor=dev(b.p["sheen_color"]), ior=dev(b.p["sheen_ior"]),
                     roughness=dev(b.p["sheen_roughness"]), anisotropic=0.0)
    g = T.glossy_rays(s, spp_n, SEED)
    open_ = b.p["sheen_weight"] > EPS
    a, e = host(q.sheen_glossy.offsets), host(g.offsets)
    assert np.array_equal(np.diff(a), np.where(open_, np.diff(e), 0))
    keep = np.repeat(open_, np.diff(e))
    for name in ("dir", "weight"):
        U.same_bits_or_both_nan(host(getattr(q.sheen_glossy, name)), host(getattr(g, name))[:, keep], name)
    assert np.array_equal(host(q.sheen_glossy.sample), host(g.sample)[keep])
    assert np.array_equal(host(q.sheen_glossy.point), host(g.point)[keep])


def test_specular_glossy_queue_is_the_oracle_sampler_at_pair_1(gpu, oracle, T, monkeypatch):
    """rls_trace_ggx_glossy_emit draws from pair 0 and cannot reach the specular lobe's pair: the oracle's rlGgx sampler on
    the lobe's parameters at pair 1, per (point, sample)"""
    from test_gpu_trace_shade import _ggx_oracle_queue, _matches, _ray_host
    from trace_util import _queue
    n, spp_n, first = 131, 3, (1 << 36) + 5
    b = Skin(gpu, oracle, n, "sphere")
    q = _at(monkeypatch, 1, lambda: b.emit(T, None, spp_n, first=first))
    _assert_glossy_queues_are_the_oracle_sampler(oracle, b, q, spp_n, first)


def _assert_glossy_queues_are_the_oracle_sampler(oracle, b, q, spp_n, first, seed=SEED):
    """both glossy queues of a skin emit against the oracle's rlGgx sampler on the lobe's parameters at pairs 0 and 1"""
    from test_gpu_trace_shade import _ggx_oracle_queue, _matches, _ray_host
    from trace_util import _queue
    wo, N, Tt = b.frame
    n = b.n
    for lobe, pair in (("sheen", 0), ("specular", 1)):
        case = dict(wo=wo, N=N, T=Tt, KsColor=b.p[lobe + "_color"], ior=b.p[lobe + "_ior"], roughness=b.p[lobe + "_roughness"],
                    anisotropic=np.zeros(n, F))
        dirs, ws, keep, kinds = _ggx_oracle_queue(oracle, case, spp_n, seed, False, pair, first)
        gate = (b.p[lobe + "_weight"] > EPS) & ~np.all(np.abs(b.p[lobe + "_color"]) < EPS, axis=0)
        assert gate.any()
        _matches(_ray_host(getattr(q, lobe + "_glossy")), _queue(dirs, ws, [k & gate for k in keep], kinds), (lobe, pair))


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_probe_queue_is_the_probe_ray_of_the_scaled_distances_at_pair_2(gpu, oracle, T, fast):
    """rls_trace_sss_probe_emit draws from pair 0 and cannot reach pair 2; its per-sample twin rls_sss_probe_ray can be handed
    pair 2's samples: the same bits for sss_scatter_dist x sss_dist_multiplier; and the oracle's getProbeRay (EXACT)"""
    n, spp_n, first = 131, 3, (1 << 36) + 5
    spp = spp_n * spp_n
    b = Skin(gpu, oracle, n, "sphere")
    gpu.set_math_mode(fast)
    try:
        q = b.emit(T, None, spp_n, first=first)
        pq = q.probes
        np.testing.assert_array_equal(host(pq.offsets), np.arange(n + 1, dtype=np.int64) * spp)
        np.testing.assert_array_equal(host(pq.point), np.repeat(np.arange(n), spp))
        np.testing.assert_array_equal(host(pq.sample), np.tile(np.arange(spp), n))
        wo, N, Tt = b.frame
        s = R.SssSampler(gpu, dev(N), dev(Tt), dev(b.p["sss_color"]), dev(b.p["sss_scatter_dist"]),
                         multiplier=dev(b.p["sss_dist_multiplier"]))
        scaled = (b.p["sss_scatter_dist"] * b.p["sss_dist_multiplier"][None, :]).astype(F)
        o = oracle.Sss(n, scaled, b.p["sss_color"], N=N, T=Tt, has_dPdu=True)
        origin, dirs, md = host(pq.origin).reshape(3, n, spp), host(pq.dir).reshape(3, n, spp), host(pq.maxdist).reshape(n, spp)
        assert (host(q.sssWeight) >= EPS).all() and md.all()
        for smp in range(spp):
            rx, ry = oracle.batch_sample_02(SEED, first, n, 2, smp)
            got = s.getProbeRay(dev(rx), dev(ry), P=b.P)
            cases.assert_same_bits(origin[:, :, smp], host(got["origin"]), (smp, "origin"))
            cases.assert_same_bits(dirs[:, :, smp], host(got["dir"]), (smp, "dir"))
            cases.assert_same_bits(md[:, smp], host(got["maxdist"]), (smp, "maxdist"))
            if not fast:
                ref = o.probe(rx, ry)
                cases.assert_tight(cases.summarize(cases.rel_err(origin[:, :, smp], (b.Ph + ref["origin"]).astype(F))), (smp, "o"))
                cases.assert_tight(cases.summarize(cases.rel_err(dirs[:, :, smp], ref["dir"])), (smp, "d"))
                cases.assert_tight(cases.summarize(cases.rel_err(md[:, smp], ref["maxdist"])), (smp, "m"))
    finally:
        gpu.set_math_mode(False)


@pytest.mark.parametrize("max_hits,cavity,literal", [(12, True, False), (5, True, True), (1, False, False)])
def test_synthetic_hit_lists_against_the_host(gpu, oracle, T, max_hits, cavity, literal):
    """hit lists no analytic scene produces (tests/test_gpu_trace_sss.py, _synthetic_hits): up to 15 reported hits a ray, counts
    above max_hits, duplicates, hits beyond maxRadius, zero and non-finite irradiance, a stride past the ray count; the node's
    sss is host_resolve's scatter x sssWeight, the lobes are untouched by the hits"""
    from test_gpu_trace_sss import _synthetic_hits
    n, spp_n = 150, 3
    spp = spp_n * spp_n
    b = Skin(gpu, oracle, n, "sphere", cavity, literal, params=_gated)
    q = b.emit(T, _mk_lights(MIXED3[:1]), spp_n)
    wo, N, Tt = b.frame
    case = dict(P=b.Ph, N=N, T=Tt, albedo=b.p["sss_color"],
                dist=(b.p["sss_scatter_dist"] * b.p["sss_dist_multiplier"][None, :]).astype(F))
    stride = n * spp + 37
    cnt, hP, hN, E = _synthetic_hits(case, spp, max_hits, stride, seed=max_hits)
    tr = _traced(gpu, q, ENVS[1])
    got = _resolve(b, q, tr, (cnt, hP, hN, E))
    scat, depth = U.host_resolve(case, spp, cnt, hP, hN, E, max_hits, cavity, literal)
    sW = host(q.sssWeight)
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.where(sW < EPS, F(0), (scat * sW).astype(F)).astype(F)
    if cases.strict_parity():
        U.same_bits_or_both_nan(got["sss"], want, (max_hits, cavity, literal))
    else:
        assert np.array_equal(np.isnan(got["sss"]), np.isnan(want))
        fin = np.all(np.isfinite(want), axis=0) & np.all(np.isfinite(got["sss"]), axis=0)
        cases.assert_tight(cases.summarize(cases.rel_err(got["sss"][:, fin], want[:, fin])), (max_hits, cavity, literal))
    assert np.isnan(got["sss"]).any() and not got["sss"][:, sW < EPS].any() and (sW < EPS).any()
    # more than one shaded hit a ray on some point (an analytic plane gives one at most): the multi-hit walk ran
    assert float(depth.max()) > (1.0 if max_hits >= 5 else 0.5)
    clean = _resolve(b, q, tr, b.hits(q, stride))
    for k in ("sheen", "specular", "sheenFresnel", "specularFresnel", "sssWeight"):
        U.same_bits_or_both_nan(got[k], clean[k], k)


def test_shadow_queues_order_kind_cone_and_maxdist(gpu, oracle, T):
    n, spp_n = 67, 4
    spp = spp_n * spp_n
    b = Skin(gpu, oracle, n, "plane")
    specs = MIXED3
    q = b.emit(T, _mk_lights(specs), spp_n)
    for sq in (q.sheen_shadow, q.specular_shadow):
        off = host(sq.offsets)
        cnt = int(off[n])
        assert off[0] == 0 and (np.diff(off) >= 0).all() and cnt <= sq.capacity and cnt > 0
        kind, pt, smp = host(sq.kind), host(sq.point).astype(np.int64), host(sq.sample).astype(np.int64)
        assert np.array_equal(pt, np.repeat(np.arange(n), np.diff(off)))
        light = (kind & T.RLS_SHADOW_LIGHT_MASK).astype(np.int64)
        bsdf = ((kind & T.RLS_SHADOW_BSDF) != 0).astype(np.int64)
        assert ((kind & T.RLS_SHADOW_SPECULAR) != 0).all() and not (kind & T.RLS_SHADOW_DIFFUSE).any()
        assert light.max() < len(specs)
        # the stated order: the key (point, light, sample, strategy) strictly ascends
        key = ((pt * 8 + light) * spp + smp) * 2 + bsdf
        assert (np.diff(key) > 0).all()
        mode = np.array([s["mis_mode"] for s in specs])[light]
        assert not ((mode == 1) & (bsdf == 1)).any() and not ((mode == 2) & (bsdf == 0)).any()
        ws = host(sq.weight_specular)
        assert (ws != 0).any(axis=0).all() and np.isfinite(ws).all()
        # the direction is inside the light's cone (light samples to rounding), maxdist the near intersection, in float64
        d = host(sq.dir).astype(np.float64)
        Pp = b.Ph[:, pt].astype(np.float64)
        C = np.array([s["center"] for s in specs], np.float64)[light].T
        rad = np.array([s["radius"] for s in specs], np.float64)[light]
        v = C - Pp
        bq = (v * d).sum(0)
        disc = np.maximum(0.0, bq * bq - ((v * v).sum(0) - rad * rad) * (d * d).sum(0))
        assert (disc > -1e-9).all() and (bq > 0).all()
        cosmax = np.sqrt(1.0 - rad * rad / (v * v).sum(0))
        assert ((bq / np.sqrt((v * v).sum(0)) / np.sqrt((d * d).sum(0))) >= cosmax - 1e-5).all()
        want = ((v * v).sum(0) - rad * rad) / (bq + np.sqrt(disc))
        # float32: disc = b^2 - c2 |dir|^2 is a difference of two rounded products, off by up to 3 x 2^-24 b^2 (+ c2's own
        # rounding of |d|^2 - r^2, 2 x 2^-24 |d|^2), so its root by min(e / (2 sqrt(disc)), sqrt(e)); then the sum, the root and
        # the quotient round once each
        u = 2.0 ** -24
        e = 3 * u * bq * bq + 2 * u * (v * v).sum(0) * (d * d).sum(0)
        droot = np.minimum(e / (2 * np.maximum(np.sqrt(disc), 1e-300)), np.sqrt(e))
        tol = want * (droot / (bq + np.sqrt(disc)) + 6 * u)
        assert (np.abs(host(sq.maxdist) - want) <= tol).all(), float((np.abs(host(sq.maxdist) - want) / tol).max())


def _bound(k, inv, terms):
    """The header's bound on one glossy sum S about a reference radiance: |S - inv sum L w| <= 3 (k + 3) 2^-24 inv sum |L||w|
    for a point with k rays.  Carried through the layer: lobe = lit + S (one rounding, 2^-24 |lobe|), AOV = lobe * W (one
    rounding), and for the specular lobe W = specular_weight * (1 - sheenFresnel) formed in float32 (two roundings, 2 x 2^-24
    relative): the float64 composition from the float32 lit, S-terms and scalars differs from the kernel's AOV by at most
    |W| (bound_S + 4 x 2^-24 (|lit| + inv sum |L||w|)) -- four roundings after S, each relative to a magnitude that
    |lit| + inv sum |L||w| bounds (to first order; the factor (1 + 2^-23) covers the second)."""
    u = 2.0 ** -24
    return (3.0 * (k + 3) * u * inv * terms), 4.0 * u


def _documented_composition(b, q, specs, spp_n, vis, rad, hits, got):
    """the header's composition on the host, for the resolve `got` of q under the visibilities vis and radiances rad (dicts by
    queue name, numpy [3, count]) and the hits (count, P, N, E): the scatter part and out bit for bit, the lobes within the bound
    of _bound about the float32 light part -> (lit {lobe: [3, n]}, gate, W), what the lobes are composed of"""
    n, spp = b.n, spp_n * spp_n
    inv32 = F(1) / F(spp)
    hc, hP, hN, E = hits
    sF, pF, sW = host(q.sheenFresnel), host(q.specularFresnel), host(q.sssWeight)
    # light part, float32 in queue order
    lit = {}
    for name, sq in (("sheen", q.sheen_shadow), ("specular", q.specular_shadow)):
        off, kind, ws = host(sq.offsets), host(sq.kind), host(sq.weight_specular)
        v = vis[name + "_shadow"]
        out = np.zeros((3, n), F)
        for i in range(n):
            for l, s in enumerate(specs):
                acc = np.zeros(3, F)
                for r in range(off[i], off[i + 1]):
                    if (kind[r] & 7) == l:
                        acc = (acc + (v[:, r] * ws[:, r]).astype(F)).astype(F)
                out[:, i] = (out[:, i] + ((np.asarray(s["radiance"], F) * acc).astype(F) * inv32).astype(F)).astype(F)
        lit[name] = out
    # scatter part through the existing host composition, bit for bit
    case = dict(P=b.Ph, N=b.frame[1], T=b.frame[2], albedo=np.broadcast_to(np.asarray(b.p["sss_color"], F).reshape(3, -1), (3, n)).copy(),
                dist=(np.asarray(b.p["sss_scatter_dist"], F).reshape(3, -1) * np.asarray(b.p["sss_dist_multiplier"], F)).astype(F)
                * np.ones((3, n), F))
    scat, _ = U.host_resolve(case, spp, hc, hP, hN, E, hP.shape[1], b.cavity, b.literal)
    sss = np.where(sW < EPS, F(0), (scat * sW).astype(F)).astype(F)
    U.same_bits_or_both_nan(got["sss"], sss, "sss")
    W = {"sheen": np.asarray(b.p["sheen_weight"], F) * np.ones(n, F),
         "specular": (np.asarray(b.p["specular_weight"], F) * (F(1) - sF)).astype(F)}
    gate = {"sheen": np.asarray(b.p["sheen_weight"], F) * np.ones(n, F) > EPS,
            "specular": np.asarray(b.p["specular_weight"], F) * np.ones(n, F) > EPS}
    for name in ("sheen", "specular"):
        gq = getattr(q, name + "_glossy")
        off, w = host(gq.offsets), host(gq.weight).astype(np.float64)
        L = rad[name + "_glossy"].astype(np.float64)
        for i in range(n):
            r = slice(off[i], off[i + 1])
            S = (L[:, r] * w[:, r]).sum(1) / spp
            mag = (np.abs(L[:, r]) * np.abs(w[:, r])).sum(1) / spp
            bS, u4 = _bound(off[i + 1] - off[i], 1.0, mag)
            want = (lit[name][:, i].astype(np.float64) + S) * W[name][i] if gate[name][i] else np.zeros(3)
            tol = abs(float(W[name][i])) * (bS + u4 * (np.abs(lit[name][:, i]) + mag)) * (1 + 2.0 ** -23)
            assert (np.abs(got[name][:, i] - want) <= tol).all(), (name, i, got[name][:, i], want, tol)
    U.same_bits_or_both_nan(got["out"], ((got["sheen"] + got["specular"]).astype(F) + got["sss"]).astype(F), "out")
    return lit, gate, W


def test_random_visibility_and_radiance_follow_the_documented_composition(gpu, oracle, T):
    n, spp_n = 67, 4
    spp = spp_n * spp_n
    inv32 = F(1) / F(spp)
    b = Skin(gpu, oracle, n, "plane", cavity=True)
    specs = MIXED3
    q = b.emit(T, _mk_lights(specs), spp_n)
    cnt = q.counts()
    rng = np.random.default_rng(5)
    vis = {k: rng.random((3, cnt[k])).astype(F) for k in ("sheen_shadow", "specular_shadow")}
    rad = {k: (rng.random((3, cnt[k])) * 10.0 ** rng.uniform(-4, 4, (3, cnt[k]))).astype(F) for k in ("sheen_glossy", "specular_glossy")}
    hc, hP, hN, E = b.hits(q)
    E = (E * rng.random(E.shape).astype(F)).astype(F)
    got = _resolve(b, q, (dev(vis["sheen_shadow"]), dev(vis["specular_shadow"]), dev(rad["sheen_glossy"]),
                          dev(rad["specular_glossy"])), (hc, hP, hN, E))
    lit, gate, W = _documented_composition(b, q, specs, spp_n, vis, rad, (hc, hP, hN, E), got)
    # with the glossy radiance 0 the lobes are the light part alone, bit for bit
    zero = {k: np.zeros_like(v) for k, v in rad.items()}
    got0 = _resolve(b, q, (dev(vis["sheen_shadow"]), dev(vis["specular_shadow"]), dev(zero["sheen_glossy"]),
                           dev(zero["specular_glossy"])), (hc, hP, hN, E))
    for name in ("sheen", "specular"):
        want = np.where(gate[name], ((lit[name] + F(0)).astype(F) * W[name]).astype(F), (F(0) * W[name]).astype(F))
        U.same_bits_or_both_nan(got0[name], want.astype(F), name + " light part")


def test_a_non_finite_ray_poisons_only_its_point(gpu, oracle, T):
    n, spp_n = 67, 3
    b = Skin(gpu, oracle, n, "plane")
    q = b.emit(T, _mk_lights(MIXED3), spp_n)
    hits = b.hits(q)
    tr = _traced(gpu, q, ENVS[1])
    clean = _resolve(b, q, tr, hits)
    vis, _, Ls, Lp = [t.clone() for t in tr[:1]] + [None] + [t.clone() for t in tr[2:]]
    i_v, i_s, i_p = 5, 20, 40
    off = lambda qq, i: int(qq.offsets[i].item())
    assert off(q.sheen_shadow, i_v + 1) > off(q.sheen_shadow, i_v)
    vis[1, off(q.sheen_shadow, i_v)] = float("nan")
    Ls[0, off(q.sheen_glossy, i_s)] = float("inf")
    Lp[2, off(q.specular_glossy, i_p)] = float("-inf")
    got = _resolve(b, q, (vis, tr[1], Ls, Lp), hits)
    others = np.ones(n, bool)
    others[[i_v, i_s, i_p]] = False
    for k in ("sheen", "specular", "sss", "out"):
        U.same_bits_or_both_nan(got[k][:, others], clean[k][:, others], k)
    assert not np.isfinite(got["sheen"][1, i_v]) and not np.isfinite(got["sheen"][0, i_s])
    assert not np.isfinite(got["specular"][2, i_p])
    U.same_bits_or_both_nan(got["specular"][:, i_v], clean["specular"][:, i_v], "the other lobe")


def test_chunked_emits_reproduce_the_unchunked_queues(gpu, oracle, T):
    n, spp_n, first = 150, 3, (1 << 36) + 5
    lights = _mk_lights(MIXED3)
    whole = Skin(gpu, oracle, n, "plane", full=n).emit(T, lights, spp_n, first=first)
    parts = []
    for a, m in ((0, 67), (67, 83)):
        parts.append(Skin(gpu, oracle, m, "plane", a=a, full=n).emit(T, lights, spp_n, first=first + a))
    for name in ("sheen_shadow", "specular_shadow", "sheen_glossy", "specular_glossy"):
        for plane in ("dir", "weight_specular" if "shadow" in name else "weight"):
            cat = np.concatenate([host(getattr(getattr(p, name), plane)) for p in parts], axis=1)
            U.same_bits_or_both_nan(host(getattr(getattr(whole, name), plane)), cat, (name, plane))
    for plane in ("origin", "dir"):
        cat = np.concatenate([host(getattr(p.probes, plane)) for p in parts], axis=1)
        U.same_bits_or_both_nan(host(getattr(whole.probes, plane)), cat, plane)
    for k in ("sheenFresnel", "specularFresnel", "sssWeight"):
        U.same_bits_or_both_nan(host(getattr(whole, k)), np.concatenate([host(getattr(p, k)) for p in parts]), k)


def test_graph_replay_of_emit_and_resolve(gpu, oracle, T):
    n, spp_n = 67, 3
    gctx = R.Context(0, use_torch_stream=False)          # the context's own stream: the NULL stream cannot be captured
    try:
        b = Skin(gctx, oracle, n, "plane")
        lights = _mk_lights(MIXED3)
        torch.cuda.synchronize()
        q = b.emit(T, lights, spp_n, share=True)
        gctx.synchronize()
        cnt = q.counts()
        tr = _traced(gctx, q, ENVS[1], cnt)
        hits = tuple(dev(h) for h in b.hits(q))
        torch.cuda.synchronize()
        want = q.resolve(*tr, *hits)
        gctx.synchronize()
        want = {k: host(v) for k, v in want.items()}
        out = {k: gctx.empty(3, n) for k in ("sheen", "specular", "sss", "out")}
        out.update({k: gctx.empty(n) for k in ("sheenFresnel", "specularFresnel", "sssWeight")})
        torch.cuda.synchronize()
        with gctx.capture() as graph:
            b.emit(T, lights, spp_n, queues=q)
            q.resolve(*tr, *hits, out=out, counts=cnt)
        for t in out.values():
            t.zero_()
        for t in (q.sheenFresnel, q.specularFresnel, q.sssWeight, q.sheen_glossy.offsets, q.probes.maxdist):
            t.zero_()
        torch.cuda.synchronize()
        graph.launch()
        gctx.synchronize()
        _same({k: host(v) for k, v in out.items()}, want, "replay")
    finally:
        gctx.close() if hasattr(gctx, "close") else None

