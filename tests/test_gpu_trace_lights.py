"""GPU: the caller-traced light loops (include/rlshaders_amd_trace.h, rls_shadow_queue; rlshaders_amd/trace.py).

The emits put one shadow ray per term-carrying sample of rls_ggx_direct_lighting's / rls_disney_direct_lighting's two-sample
MIS estimator into a compacted queue; the resolves reduce the visibility the caller traced.  Checked here:
  1. with visibility 1 the resolve IS the analytic call, bit for bit, EXACT and FAST (and the oracle's two-sums form);
  2. single rays: weights, directions and maxdist one by one;
  3. an arbitrary coloured visibility against the documented composition in numpy float32, and a float64 bound;
  4. occlusion of one of two lights, a visibility of 0, the queue's invariants;
  5. edges: batch sizes, the per-point slot maximum, non-finite visibilities, argument checks, graph replay.
EXACT gates are max == 0 (cases.assert_same_bits; cases.assert_tight against the oracle)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import rlshaders_amd as R
from gpu_util import dev, disney_oracle, disney_sampler, ggx_oracle, ggx_sampler, host
from test_gpu_loop_edges import LIGHTS, _lights, _sl, _slab, make_case
from trace_lights_util import BSDF, DIFFUSE, LIGHT_MASK, SPECULAR, assert_float64_bound, compose, cone, cone_hit, near_hit_f64, queue_host, segment
from trace_util import disney_inputs, ggx_inputs

pytestmark = pytest.mark.gpu

SEED = 9157
INVALID = 1            # RLS_ERR_INVALID_ARGUMENT
NODES = ("ggx", "disney")


@pytest.fixture(scope="module")
def T():
    from rlshaders_amd import build, trace
    build.build_trace_library()
    trace.load()
    return trace


class Batch:
    """one node's closure over the slab of shading points, with what both the analytic call and the emit take"""

    def __init__(self, T, ctx, node, n, oracle=None, c=None, materials=None, shader=None, seed=cases.SEED_PARITY):
        self.T, self.ctx, self.node, self.n = T, ctx, node, n
        self.c = c if c is not None else make_case(node + "_direct", oracle, n, seed)
        c = self.c
        if "P" not in c:
            c["P"] = _slab(n, seed)
        self.P = dev(c["P"])
        if node == "ggx":
            if materials is not None:
                self.s = R.GgxSampler(ctx, dev(c["wo"]), dev(c["N"]), dev(c["T"]), specColor=dev(c["KsColor"]), ior=dev(c["ior"]),
                                      roughness=dev(c["roughness"]), anisotropic=dev(c["anisotropic"]), materials=materials)
            else:
                self.s = ggx_sampler(ctx, c)
            self.sh = shader if shader is not None else dict(KdColor=dev(c["kdc"]), Kd=dev(c["kd"]),
                                                             diffuseRoughness=dev(c["kdr"]), Ks=dev(c["ks"]))
        else:
            if materials is not None:
                sc = {k: dev(c[k]) for k in R._capi.DISNEY_SCALARS if k in c}
                self.s = R.DisneySampler(ctx, dev(c["wo"]), dev(c["N"]), dev(c["T"]), base_color=dev(c["base_color"]),
                                         materials=materials, **sc)
            else:
                self.s = disney_sampler(ctx, c)
            self.sh = None

    def analytic(self, lights, spp_n, seed=SEED, first=0):
        if self.node == "ggx":
            dd, ds = self.s.directLighting(self.P, lights, spp_n, seed, first_index=first, **self.sh)
        else:
            dd, ds = self.s.directLighting(self.P, lights, spp_n, seed, first_index=first)
        return host(dd), host(ds)

    def emit(self, lights, spp_n, seed=SEED, first=0, queue=None):
        if self.node == "ggx":
            return self.T.ggx_shadow_rays(self.s, self.T.ggx_shader(self.s, **self.sh), self.P, lights, spp_n, seed, first, queue)
        return self.T.disney_shadow_rays(self.s, self.P, lights, spp_n, seed, first, queue)

    def tail(self):
        """rlGgx: (KdColor * Kd [3, n], Ks [n]) in float32, as the kernels form them"""
        if self.node != "ggx":
            return None
        c = self.c
        return (c["kdc"] * c["kd"][None, :]).astype(np.float32), c["ks"].astype(np.float32)


def _ones(ctx, q):
    return torch.ones(3, max(q.count, 1), dtype=torch.float32, device=ctx.torch_device)


def _resolve(q, vis):
    dd, ds = q.resolve(vis)
    return host(dd), host(ds)


def _same(got, want, what):
    cases.assert_same_bits(got[0], want[0], (what, "direct_diffuse"))
    cases.assert_same_bits(got[1], want[1], (what, "direct_specular"))


def _rad(lights):
    return np.array([[l.radiance[k] for k in range(3)] for l in lights], np.float32)


def _at(monkeypatch, g, fn):
    if g is None:
        monkeypatch.delenv("RLS_INTEGRATE_GROUP", raising=False)
    else:
        monkeypatch.setenv("RLS_INTEGRATE_GROUP", str(g))
    try:
        return fn()
    finally:
        monkeypatch.delenv("RLS_INTEGRATE_GROUP", raising=False)


# ---- 1. visibility 1: the analytic light loops, bit for bit ----------------------------------------------------------------
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("node", NODES)
def test_unit_visibility_is_the_analytic_loop_at_every_spp_n(gpu, oracle, T, node, fast):
    """eight lights, the three mis_modes mixed, one light around every point (cone.valid false), one below the slab"""
    _, lights = _lights(oracle, LIGHTS)
    gpu.set_math_mode(fast)
    try:
        for spp_n in range(1, 17):
            n = 700 if spp_n <= 6 else 203 if spp_n <= 11 else 77
            b = Batch(T, gpu, node, n, oracle)
            q = b.emit(lights, spp_n)
            _same(_resolve(q, _ones(gpu, q)), b.analytic(lights, spp_n), (node, spp_n, fast))
    finally:
        gpu.set_math_mode(False)


@pytest.mark.parametrize("node", NODES)
def test_unit_visibility_at_every_light_count_and_group_width(gpu, oracle, T, monkeypatch, node):
    lo, lights = _lights(oracle, LIGHTS)
    b = Batch(T, gpu, node, 333, oracle)
    for nl in range(1, 9):
        for spp_n, g in ((2, 1), (2, 4), (4, 16), (8, 64), (5, None), (3, 64)):
            want = _at(monkeypatch, 1, lambda: b.analytic(lights[:nl], spp_n))
            q = _at(monkeypatch, g, lambda: b.emit(lights[:nl], spp_n))
            h = queue_host(q)
            _same(_resolve(q, _ones(gpu, q)), want, (node, nl, spp_n, g))
            if g != 1:                                              # the queue itself does not depend on the width
                q1 = _at(monkeypatch, 1, lambda: b.emit(lights[:nl], spp_n))
                h1 = queue_host(q1)
                for k in h:
                    assert np.array_equal(np.ascontiguousarray(h[k]).view(np.uint8), np.ascontiguousarray(h1[k]).view(np.uint8)), (node, nl, g, k)


@pytest.mark.parametrize("node", NODES)
def test_unit_visibility_is_the_oracle_two_sums_form(gpu, oracle, T, monkeypatch, node):
    """Directly against the oracle at spp_n 1, 3 and 4, one lane per point, EXACT, eight lights.  Every other combination
    of the anchor (spp_n, G, light count, FAST) reaches the oracle through the analytic kernel: the tests above hold the
    resolve to rls_*_direct_lighting bit for bit, and tests/test_gpu_loop_edges.py holds that kernel to the oracle's two-sums
    form at every spp_n, G and light count."""
    lo, lights = _lights(oracle, LIGHTS)
    n = 257
    b = Batch(T, gpu, node, n, oracle)
    c = b.c
    for spp_n in (1, 3, 4):
        if node == "ggx":
            ref = ggx_oracle(oracle, c).direct_lighting(c["P"], lo, spp_n, SEED, Kd_color=c["kdc"], Kd=c["kd"],
                                                        Kd_roughness=c["kdr"], Ks=c["ks"])
        else:
            ref = disney_oracle(oracle, c).direct_lighting(c["P"], lo, spp_n, SEED)
        q = _at(monkeypatch, 1, lambda: b.emit(lights, spp_n))
        got = _resolve(q, _ones(gpu, q))
        for k, name in enumerate(("direct_diffuse", "direct_specular")):
            cases.assert_tight(cases.summarize(cases.rel_err(got[k], ref[k])), (node, spp_n, name))


@pytest.mark.parametrize("node", NODES)
def test_unit_visibility_uniform_parameters_and_by_reference(gpu, oracle, T, node):
    _, lights = _lights(oracle, LIGHTS[:3])
    n, spp_n = 1001, 3
    for kind in ("uniform", "materials"):
        if node == "ggx":
            c, _, mat = ggx_inputs(kind, n)
            if mat is None:
                sh = dict(KdColor=(0.7, 0.5, 0.2), Kd=0.8, diffuseRoughness=0.3, Ks=0.6)
            else:
                m = mat[1]
                u = lambda j: dev(oracle.gen_uniform(cases.SEED_PARITY, 0, m, 900 + j))
                sh = dict(KdColor=dev(np.stack([oracle.gen_uniform(cases.SEED_PARITY, 0, m, 910 + j) for j in range(3)])),
                          Kd=u(0), diffuseRoughness=u(1), Ks=u(2))
            b = Batch(T, gpu, node, n, c=dict(c), materials=mat, shader=sh)
        else:
            c, mat = disney_inputs(kind, n)
            b = Batch(T, gpu, node, n, c=dict(c), materials=mat)
        q = b.emit(lights, spp_n)
        _same(_resolve(q, _ones(gpu, q)), b.analytic(lights, spp_n), (node, kind))


def test_sample_diffuse_off(gpu, oracle, T):
    """AiColorIsSmall(KdColor * Kd): no diffuse term is drawn, none is queued, direct_diffuse is radiance * 0"""
    _, lights = _lights(oracle, LIGHTS[:3])
    n, spp_n = 500, 3
    c = make_case("ggx_direct", oracle, n)
    c["kd"] = np.where(np.arange(n) % 2 == 0, np.float32(1e-6), c["kd"]).astype(np.float32)
    b = Batch(T, gpu, "ggx", n, c=c)
    q = b.emit(lights, spp_n)
    h = queue_host(q)
    off_pts = np.arange(n) % 2 == 0
    assert not np.any((h["kind"] & DIFFUSE != 0) & off_pts[h["point"]])
    assert np.any(h["kind"] & DIFFUSE != 0)
    _same(_resolve(q, _ones(gpu, q)), b.analytic(lights, spp_n), "sampleDiffuse off")


@pytest.mark.parametrize("node", NODES)
def test_first_index_past_2_32_and_chunks(gpu, oracle, T, node):
    """a batch walked in chunks: the chunks' queues concatenate to the unchunked queue, their resolves to its resolve"""
    _, lights = _lights(oracle, LIGHTS[:4])
    n, spp_n, first = 3000, 3, (1 << 32) - 1200
    full_b = Batch(T, gpu, node, n, oracle)
    full = full_b.emit(lights, spp_n, first=first)
    hf = queue_host(full)
    vis = torch.rand(3, max(hf["count"], 1), generator=torch.Generator().manual_seed(3)).cuda()
    rf = _resolve(full, vis)
    _same(_resolve(full, _ones(gpu, full)), full_b.analytic(lights, spp_n, first=first), (node, "first_index past 2^32"))
    base = _resolve(Batch(T, gpu, node, n, oracle).emit(lights, spp_n, first=0), vis)
    assert not np.array_equal(base[1], rf[1])                      # the index reaches the scrambles
    for a, e in ((0, 1111), (1111, 1200), (1200, 1201), (1201, n)):
        bc = Batch(T, gpu, node, e - a, c=_sl(full_b.c, a, e))
        qc = bc.emit(lights, spp_n, first=first + a)
        hc = queue_host(qc)
        lo, hi = int(hf["offsets"][a]), int(hf["offsets"][e])
        np.testing.assert_array_equal(hc["offsets"], hf["offsets"][a:e + 1] - lo)
        for k in ("dir", "maxdist", "ws", "wd", "kind", "sample"):
            assert np.array_equal(np.ascontiguousarray(hc[k]).view(np.uint8),
                                  np.ascontiguousarray(hf[k][..., lo:hi]).view(np.uint8)), (node, a, e, k)
        np.testing.assert_array_equal(hc["point"] + a, hf["point"][lo:hi])
        got = _resolve(qc, vis[:, lo:max(hi, lo + 1)].contiguous())
        _same(got, (rf[0][:, a:e], rf[1][:, a:e]), (node, a, e, "resolve"))


# ---- 2. single rays ------------------------------------------------------------------------------------------------------------
ONE = dict(center=(1.5, 2.5, 3.5), radius=1.25, radiance=(3.0, 2.0, 0.5))


@pytest.mark.parametrize("node", NODES)
def test_single_weights_against_the_analytic_loop(gpu, oracle, T, node):
    """spp_n = 1, one light, LIGHT_ONLY then BSDF_ONLY: each AOV is one weight times radiance / 1"""
    n = 4096
    b = Batch(T, gpu, node, n, oracle)
    tail = b.tail()
    for mode in (1, 2):
        _, lights = _lights(oracle, [dict(ONE, mis_mode=mode)])
        rad = _rad(lights)[0]
        q = b.emit(lights, 1)
        h = queue_host(q)
        dd, ds = b.analytic(lights, 1)
        cnt = np.diff(h["offsets"])
        assert cnt.max() <= (1 if mode == 1 else 2) and h["count"] > 20
        assert np.all(((h["kind"] & BSDF) != 0) == (mode == 2))
        wS, wD = np.zeros((3, n), np.float32), np.zeros((3, n), np.float32)
        s = h["kind"] & SPECULAR != 0
        d = h["kind"] & DIFFUSE != 0
        wS[:, h["point"][s]] = h["ws"][:, s]
        wD[:, h["point"][d]] = h["wd"][:, d]
        want_s = (rad[:, None] * wS) * np.float32(1.0)
        want_d = (rad[:, None] * wD) * np.float32(1.0)
        if tail is not None:
            want_d, want_s = want_d * tail[0], want_s * tail[1][None, :]
        cases.assert_same_bits(want_s, ds, (node, mode, "specular weights"))
        cases.assert_same_bits(want_d, dd, (node, mode, "diffuse weights"))
        # a term without its bit is an exact zero in the queue's plane
        assert np.all(h["ws"][:, ~s] == 0) and np.all(h["wd"][:, ~d] == 0)


def bsdf_directions_against_the_oracle(oracle, node, c, h, nl, spp_n, seed=SEED, first=0):
    """the BSDF-strategy rays of the queue h (queue_host) of the points c under nl lights, per (light, segment, sample) against
    the oracle's samplers -> {(light, segment): rays checked}"""
    n = c["wo"].shape[1]
    seg, l = segment(h["kind"]), h["kind"] & LIGHT_MASK
    checked = {}
    for li in range(nl):
        for s in range(spp_n * spp_n):
            if node == "ggx":
                jobs = [(2, 3 * li + 1, lambda rx, ry: ggx_oracle(oracle, c).sample_eval_pdf(rx, ry)[0])]
            else:
                od = disney_oracle(oracle, c)
                jobs = [(1, 3 * li + 1, lambda rx, ry: od.sample(0x08, rx, ry)), (2, 3 * li + 2, lambda rx, ry: od.sample(0x10, rx, ry))]
            for sg, pair, fn in jobs:
                rx, ry = oracle.batch_sample_02(seed, first, n, pair, s)
                want = fn(rx, ry)
                m = (seg == sg) & (l == li) & (h["sample"] == s)
                checked[(li, sg)] = checked.get((li, sg), 0) + int(m.sum())
                if m.any():
                    cases.assert_tight(cases.summarize(cases.rel_err(h["dir"][:, m], want[:, h["point"][m]])), (node, li, sg, s))
    return checked


@pytest.mark.parametrize("node", NODES)
def test_bsdf_directions_are_the_oracle_samplers(gpu, oracle, T, node):
    """BSDF-strategy rays: the direction of (point, light, segment, sample) is the oracle sampler's on the numbers
    orc_batch_sample_02 draws for the light's streams 6 l + 2 .. 6 l + 5 (dimension pairs 3 l + 1, 3 l + 2).
    The gate is cases.assert_tight, as in tests/test_gpu_trace_edges.py: max == 0 (bit equality) where the host libm is the
    one the kernels restate (cases.strict_parity), elsewhere at most one point of a batch beyond 1e-5.  rlGgx's diffuse-lobe
    directions (segment 1) have no oracle sampler of their own; the single-weight test and the anchor cover them."""
    lo, lights = _lights(oracle, [dict(LIGHTS[0], mis_mode=2), dict(LIGHTS[6], mis_mode=0)])
    n, spp_n = 2048, 3
    b = Batch(T, gpu, node, n, oracle)
    h = queue_host(b.emit(lights, spp_n))
    checked = bsdf_directions_against_the_oracle(oracle, node, b.c, h, 2, spp_n)
    # every (light, segment) that has an oracle sampler was checked, on a share of the points that hit the light
    assert set(checked) == {(li, sg) for li in range(2) for sg in ((2,) if node == "ggx" else (1, 2))}
    assert all(v >= 20 for v in checked.values()), checked


@pytest.mark.parametrize("node", NODES)
def test_light_directions_and_maxdist(gpu, oracle, T, node):
    """light-strategy rays: unit, above the horizon, inside the cone (cone_hit restated on the host).  Every ray's maxdist
    against the near root in float64 from the emitted float32 direction."""
    specs = [dict(LIGHTS[0], mis_mode=0), dict(LIGHTS[2], mis_mode=2), dict(LIGHTS[6], mis_mode=1)]
    _, lights = _lights(oracle, specs)
    n, spp_n = 4096, 4
    b = Batch(T, gpu, node, n, oracle)
    h = queue_host(b.emit(lights, spp_n))
    P, N = b.c["P"], b.c["N"]
    assert h["count"] > n
    worst, near = 0.0, 0
    for li, sp in enumerate(specs):
        m = (h["kind"] & LIGHT_MASK) == li
        pts, dirs = h["point"][m], h["dir"][:, m]
        light = m & (h["kind"] & BSDF == 0)
        dl, pl = h["dir"][:, light], h["point"][light]
        if sp["mis_mode"] == 2:
            assert not light.any()
        else:
            assert light.any()
        assert np.all(np.abs(np.linalg.norm(dl.astype(np.float64), axis=0) - 1.0) < 4e-7)
        assert np.all((dl * N[:, pl]).sum(axis=0, dtype=np.float32) > 0)
        t, disc, bb = near_hit_f64(sp["center"], sp["radius"], P[:, pts], dirs)
        d, c2 = cone(sp["center"], sp["radius"], P[:, pl])
        inside = cone_hit(d, c2, dl)
        # within a few ulp of tangency the float32 test may go either way (and maxdist loses its digits): excluded below
        tangent = disc < 1e-5 * bb * bb
        assert np.all(inside | tangent[h["kind"][m] & BSDF == 0])
        near += int(tangent.sum())
        rel = np.abs(h["maxdist"][m].astype(np.float64) - t) / t
        worst = max(worst, float(rel[~tangent].max()))
    print(f"maxdist: worst relative error {worst:.3e}, rays near tangency {near} of {h['count']}")
    assert near <= 1e-3 * h["count"], (near, h["count"])
    # Measured on these inputs on the MI355X, away from tangency (disc >= 1e-5 b^2: 11 of 74 655 rlGgx rays and 11 of 74 313
    # rlDisney rays excluded, 1.5e-4 of them): largest relative error 4.097e-5 for both nodes; the kernel's formula restated in
    # numpy float32 on 2e5 directions per light gives 4.05e-5.  (The cancellation in b^2 - c2 |dir|^2 costs up to 1e5 x 2^-24
    # of disc, half of that of its root, which is >= 3.2e-3 of b + the root.)  The margin is four times the measured value.
    assert worst <= 4 * 4.097e-5, worst


# ---- 3. an arbitrary visibility ------------------------------------------------------------------------------------------------
def _visibility(cnt, seed=11):
    rng = np.random.default_rng(seed)
    v = rng.random((3, max(cnt, 1)), dtype=np.float32)
    sel = rng.random(max(cnt, 1))
    v[:, sel < 0.2] = 0.0
    v[:, sel > 0.8] = 1.0
    return v


@pytest.mark.parametrize("node", NODES)
def test_coloured_visibility_is_the_documented_composition(gpu, oracle, T, node):
    _, lights = _lights(oracle, LIGHTS)
    n, spp_n = 1500, 4
    b = Batch(T, gpu, node, n, oracle)
    q = b.emit(lights, spp_n)
    h = queue_host(q)
    vis = _visibility(h["count"])
    got = _resolve(q, dev(vis))
    want = compose(h, vis, _rad(lights), spp_n * spp_n, tail=b.tail())
    _same(got, want, (node, "numpy float32 composition"))
    assert_float64_bound(h, vis, _rad(lights), spp_n * spp_n, got, b.tail(), node)


# ---- 4. occlusion ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("node", NODES)
def test_a_half_space_in_front_of_one_light(gpu, oracle, T, node):
    """two lights on either side of the slab in x; the half-space x > 5 blocks every ray to light 1 and none to light 0"""
    specs = [dict(center=(-4.0, 2.0, 3.0), radius=1.0, radiance=(3.0, 2.0, 1.0), mis_mode=0),
             dict(center=(9.0, 2.0, 3.0), radius=1.0, radiance=(1.0, 4.0, 2.0), mis_mode=0)]
    _, lights = _lights(oracle, specs)
    n, spp_n = 2000, 4
    b = Batch(T, gpu, node, n, oracle)
    q = b.emit(lights, spp_n)
    h = queue_host(q)
    # the "tracer": the ray P + t dir, 0 < t < maxdist, crosses x = 5
    P = b.c["P"][:, h["point"]]
    end = P[0] + h["maxdist"] * h["dir"][0]
    blocked = (P[0] < 5.0) & (end > 5.0)
    l = h["kind"] & LIGHT_MASK
    assert np.array_equal(blocked, l == 1) and blocked.any() and (~blocked).any()
    vis = np.where(blocked, np.float32(0.0), np.float32(1.0))[None, :].repeat(3, axis=0)
    got = _resolve(q, dev(vis))
    want = b.analytic(lights[:1], spp_n)
    for a in range(2):                                              # by value: the blocked light adds +0
        np.testing.assert_array_equal(got[a], want[a])
    zero = _resolve(q, torch.zeros(3, max(h["count"], 1), device=gpu.torch_device))
    assert np.all(zero[0] == 0) and np.all(zero[1] == 0)


@pytest.mark.parametrize("node", NODES)
def test_queue_invariants(gpu, oracle, T, node):
    _, lights = _lights(oracle, LIGHTS)
    n, spp_n = 1024, 3
    spp = spp_n * spp_n
    b = Batch(T, gpu, node, n, oracle)
    h = queue_host(b.emit(lights, spp_n))
    off, kind = h["offsets"], h["kind"]
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and np.all(np.diff(off) <= len(lights) * 3 * spp) and off[n] == h["count"]
    np.testing.assert_array_equal(h["point"], np.repeat(np.arange(n), np.diff(off)))
    assert np.all(kind & (SPECULAR | DIFFUSE) != 0)                              # no ray with every term bit clear
    assert np.all(kind & ~(LIGHT_MASK | BSDF | SPECULAR | DIFFUSE) == 0)
    bs = kind & BSDF != 0
    assert np.all(np.isin(kind[bs] & (SPECULAR | DIFFUSE), (SPECULAR, DIFFUSE)))   # a BSDF ray carries one lobe
    order = ((h["point"] * 8 + (kind & LIGHT_MASK)) * 3 + segment(kind)) * 256 + h["sample"]
    assert np.all(np.diff(order) > 0)
    assert np.all(h["sample"] < spp)
    modes = np.array([sp["mis_mode"] for sp in LIGHTS])[kind & LIGHT_MASK]
    assert not np.any(bs & (modes == 1)) and not np.any(~bs & (modes == 2))
    assert not np.any((kind & LIGHT_MASK) == 3)                                   # the light around every point
    assert np.all(np.isfinite(h["maxdist"])) and np.all(h["maxdist"] > 0)
    s, d = kind & SPECULAR != 0, kind & DIFFUSE != 0
    assert np.all(np.any(h["ws"][:, s] != 0, axis=0)) and np.all(np.any(h["wd"][:, d] != 0, axis=0))


# ---- 5. edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("node", NODES)
@pytest.mark.parametrize("n,nl,spp_n", [(1, 2, 4), (257, 3, 2), (1025, 1, 1), (5, 8, 16)])
def test_batch_sizes_and_the_slot_maximum(gpu, oracle, T, node, n, nl, spp_n):
    _, lights = _lights(oracle, LIGHTS[:nl])
    b = Batch(T, gpu, node, n, oracle)
    q = b.emit(lights, spp_n)
    h = queue_host(q)
    _same(_resolve(q, _ones(gpu, q)), b.analytic(lights, spp_n), (node, n, nl, spp_n))
    vis = _visibility(h["count"], seed=n)
    _same(_resolve(q, dev(vis)), compose(h, vis, _rad(lights), spp_n * spp_n, tail=b.tail()), (node, n, nl, spp_n, "coloured"))


@pytest.mark.parametrize("node", NODES)
def test_a_non_finite_visibility_stays_in_its_point(gpu, oracle, T, node):
    _, lights = _lights(oracle, LIGHTS[:3])
    n, spp_n = 777, 3
    b = Batch(T, gpu, node, n, oracle)
    q = b.emit(lights, spp_n)
    h = queue_host(q)
    cnt = h["count"]
    vis = np.full((3, q.capacity), np.nan, np.float32)              # past the rays: NaN that no point may read
    vis[:, :cnt] = _visibility(cnt)
    clean = _resolve(q, dev(vis))
    rng = np.random.default_rng(5)
    hit = rng.choice(cnt, max(3, cnt // 60), replace=False)
    vis[rng.integers(0, 3, hit.size), hit] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(hit.size) % 3]
    got = _resolve(q, dev(vis))
    _same(got, compose(h, vis, _rad(lights), spp_n * spp_n, tail=b.tail()), (node, "non-finite"))
    dirty = np.zeros(n, bool)
    dirty[h["point"][~np.isfinite(vis[:, :cnt]).all(axis=0)]] = True
    assert dirty.any() and not dirty.all()
    for a in range(2):
        assert np.array_equal(got[a][:, ~dirty].view(np.uint32), clean[a][:, ~dirty].view(np.uint32)), node
    assert not np.isfinite(got[0][:, dirty]).all() or not np.isfinite(got[1][:, dirty]).all()


def _last_error():
    return R.load().rls_last_error()


@pytest.mark.parametrize("node", NODES)
def test_argument_checks(gpu, oracle, T, node):
    lib = T.load()
    _, lights = _lights(oracle, LIGHTS[:2])
    n, spp_n, nl = 300, 2, 2
    b = Batch(T, gpu, node, n, oracle)
    la = (R._capi.SphereLight * 9)(*(list(lights) + [lights[0]] * 7))
    q = T.ShadowQueue(gpu, n, nl, spp_n, disney=node == "disney")
    sh = T.ggx_shader(b.s, **b.sh) if node == "ggx" else None
    Pv = R.closures.cvec3(b.P, n, "P")
    out = gpu.empty(3, n), gpu.empty(3, n)
    vis = torch.ones(3, q.capacity, device=gpu.torch_device)
    vc = T.capi.CRgb(*[vis[k].data_ptr() for k in range(3)])
    oc = [T.capi.Rgb(*[o[k].data_ptr() for k in range(3)]) for o in out]

    def emit(qq, lights_n=nl, spp=spp_n, nn=n, la=la):
        if node == "ggx":
            return lib.rls_trace_ggx_direct_emit(gpu.handle, nn, C.byref(b.s.c), C.byref(sh), Pv, la, lights_n, spp, SEED, 0,
                                                 C.byref(qq) if qq is not None else None)
        return lib.rls_trace_disney_direct_emit(gpu.handle, nn, C.byref(b.s.c), Pv, la, lights_n, spp, SEED, 0,
                                                C.byref(qq) if qq is not None else None)

    def resolve(qq, lights_n=nl, spp=spp_n, v=vc, o=oc):
        if node == "ggx":
            return lib.rls_trace_ggx_direct_resolve(gpu.handle, n, C.byref(b.s.c), C.byref(sh), la, lights_n, spp,
                                                    C.byref(qq) if qq is not None else None, v, o[0], o[1])
        return lib.rls_trace_disney_direct_resolve(gpu.handle, n, la, lights_n, spp, C.byref(qq) if qq is not None else None,
                                                   v, o[0], o[1])

    assert emit(q.q) == 0 and resolve(q.q) == 0
    gpu.synchronize()
    planes = (q.offsets, q._dir, q._maxdist, q._ws, q._wd, q._kind, q._point, q._sample)
    before = [t.clone() for t in planes]
    outs = [o.clone() for o in out]

    def bad(**kw):
        x = T.ShadowQueue_.from_buffer_copy(q.q)
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    assert emit(bad(capacity=n * nl * 3 * spp_n * spp_n - 1)) == INVALID and b"capacity" in _last_error()
    assert emit(bad(scratch_bytes=T.shadow_scratch_bytes(n, nl, spp_n) - 1)) == INVALID and b"scratch" in _last_error()
    assert emit(q.q, lights_n=0) == INVALID and b"n_lights" in _last_error()
    assert emit(q.q, lights_n=9) == INVALID and b"n_lights" in _last_error()
    assert emit(q.q, la=None) == INVALID
    for spp in (0, 17):
        assert emit(q.q, spp=spp) == INVALID and resolve(q.q, spp=spp) == INVALID
    for field in ("offsets", "scratch", "maxdist", "kind"):
        assert emit(bad(**{field: None})) == INVALID, field
    for field in ("dir", "weight_specular"):
        x = bad()
        getattr(x, field).__setattr__("xyz"[1] if field == "dir" else "g", None)
        assert emit(x) == INVALID, field
    x = bad()
    x.weight_diffuse.r = None
    assert emit(x) == INVALID and resolve(x) == INVALID
    x = bad()
    x.weight_diffuse.b = None
    assert emit(x) == (0 if node == "ggx" else INVALID)             # rlGgx writes weight_diffuse.r only
    assert emit(None) == INVALID and resolve(None) == INVALID
    wrong = list(lights)
    wrong[1] = R._capi.SphereLight.from_buffer_copy(bytes(lights[1]))
    wrong[1].radius = 0.0
    assert emit(q.q, la=(R._capi.SphereLight * 2)(*wrong)) == INVALID and b"radius" in _last_error()
    wrong[1].radius, wrong[1].mis_mode = 1.0, 3
    assert emit(q.q, la=(R._capi.SphereLight * 2)(*wrong)) == INVALID and b"mis_mode" in _last_error()
    assert resolve(q.q, lights_n=0) == INVALID and resolve(q.q, lights_n=9) == INVALID
    assert resolve(bad(kind=None)) == INVALID and resolve(bad(offsets=None)) == INVALID
    assert resolve(q.q, v=T.capi.CRgb(vis[0].data_ptr(), None, vis[2].data_ptr())) == INVALID
    assert resolve(q.q, o=[oc[0], T.capi.Rgb()]) == INVALID
    assert emit(bad(point=None, sample=None)) == 0                   # the optional planes
    gpu.synchronize()
    # a refused call writes nothing (the last, valid emit rewrote the same queue)
    for t, was in zip(planes, before):
        assert torch.equal(t, was)
    for o, was in zip(out, outs):
        assert torch.equal(o, was)
    bytes_ = C.c_size_t()
    assert lib.rls_trace_shadow_scratch_bytes(n, 0, 2, C.byref(bytes_)) == INVALID
    assert lib.rls_trace_shadow_scratch_bytes(n, 9, 2, C.byref(bytes_)) == INVALID
    assert lib.rls_trace_shadow_scratch_bytes(n, 1, 17, C.byref(bytes_)) == INVALID
    assert lib.rls_trace_shadow_scratch_bytes(-1, 1, 2, C.byref(bytes_)) == INVALID
    # n = 0: an empty queue
    q0 = T.ShadowQueue(gpu, 0, nl, spp_n, disney=node == "disney")
    q0.offsets.fill_(-1)
    assert emit(q0.q, nn=0) == 0 and q0.count == 0
    with pytest.raises(ValueError):
        q.lights = (la, nl)
        q.sampler, q.shader = b.s, sh
        q.resolve(torch.ones(3, 1, device=gpu.torch_device))


@pytest.mark.parametrize("node", NODES)
def test_emit_and_resolve_in_a_graph(oracle, T, node):
    _, lights = _lights(oracle, LIGHTS[:3])
    n, spp_n = 3000, 3
    gctx = R.Context(0, use_torch_stream=False)          # the context's own stream: the NULL stream cannot be captured
    try:
        b = Batch(T, gctx, node, n, oracle)
        torch.cuda.synchronize()
        direct = b.emit(lights, spp_n)
        gctx.synchronize()
        hd = queue_host(direct)
        vis = dev(_visibility(hd["count"]))
        q = T.ShadowQueue(gctx, n, len(lights), spp_n, disney=node == "disney")
        out = gctx.empty(3, n), gctx.empty(3, n)
        torch.cuda.synchronize()
        want = direct.resolve(vis)
        gctx.synchronize()                               # (the context's own stream: torch's copies do not wait for it)
        want = host(want[0]), host(want[1])
        with gctx.capture() as g:
            b.emit(lights, spp_n, queue=q)
            q.resolve(vis, out=out, count=hd["count"])
        for o in out:
            o.zero_()
        q.offsets.zero_()
        torch.cuda.synchronize()
        g.launch()
        gctx.synchronize()
        g.close()
        hq = queue_host(q)
        for k in hd:
            assert np.array_equal(np.ascontiguousarray(hq[k]).view(np.uint8), np.ascontiguousarray(hd[k]).view(np.uint8)), k
        _same((host(out[0]), host(out[1])), want, (node, "replay"))
    finally:
        gctx.close()
