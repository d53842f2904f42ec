"""GPU: the n^2-spp loop kernels (rls_loops.hpp; launched from integrate.hip, lights.hip, scatter.hip, shade.hip) at
their edges, held to the oracle: every spp_n 1..16 at every lane-group width, the LDS queues of the packed rare branches
and evaluations driven to all of their 4 x 64 slots, one to eight lights, several rounds of the grid-stride loop, the
automatic group width, the words beside the output planes and a first_index range that crosses 2^32.

Gates: cases.assert_tight for one lane per point against the oracle, cases.assert_same_bits for every other comparison
of EXACT results; FAST mode under the gates of test_gpu_fast_mode.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import rlshaders_amd as R
from gpu_util import dev, disney_oracle, disney_sampler, ggx_oracle, ggx_sampler, host
from rlshaders_amd.closures import plane, rgb
from test_gpu_scatter import _sphere_case

pytestmark = pytest.mark.gpu

ENV = (0.7, 0.8, 0.9)
GROUPS = (4, 16, 64)
SKIN_SCENE = dict(geometry="sphere", sphere_radius=1.0, light_dir=(0.0, 0.6, 0.8), use_cavity_fade=True)
SSS_SCENE = dict(geometry="sphere", sphere_center=(0.3, -0.2, 0.1), sphere_radius=0.35, light_dir=(0.0, 0.6, 0.8),
                 light_color=(1.5, 1.0, 0.25), use_cavity_fade=True)
# eight lights over the slab of shading points (_slab): the three estimator modes mixed; light 3 holds every point of the
# slab inside it (invalid cone: black), light 4 lies below the slab (below the horizon of most frames)
LIGHTS = (dict(center=(2.0, 2.0, 3.0), radius=1.25, radiance=(3.0, 2.0, 1.0), mis_mode=0),
          dict(center=(-3.0, 1.0, 2.5), radius=0.5, radiance=(0.5, 4.0, 2.0), mis_mode=1),
          dict(center=(0.5, -2.5, 6.0), radius=2.0, radiance=(1.0, 1.0, 6.0), mis_mode=2),
          dict(center=(2.0, 2.0, 0.5), radius=4.0, radiance=(1.0, 1.0, 1.0), mis_mode=0),
          dict(center=(2.0, 2.0, -5.0), radius=0.5, radiance=(2.0, 2.0, 2.0), mis_mode=2),
          dict(center=(6.0, -1.0, 1.5), radius=0.8, radiance=(0.3, 0.6, 0.9), mis_mode=1),
          dict(center=(1.0, 5.0, 4.0), radius=1.0, radiance=(5.0, 1.0, 1.0), mis_mode=0),
          dict(center=(-1.0, -1.0, 8.0), radius=3.0, radiance=(0.7, 0.7, 0.2), mis_mode=2))
LIT = ("ggx_direct", "disney_direct", "ggx_shade", "disney_shade", "skin")
KINDS = ("ggx_integrate", "ggx_refract", "ggx_refract_untraced", "disney_integrate", "disney_streamed") + LIT + ("sss",)
FORCED_G1 = ("ggx_refract_untraced", "disney_streamed")       # the product runs these with one lane per point


def _threads(oracle):
    return min(16, oracle.hardware_threads())


def _slab(n, seed=cases.SEED_PARITY):
    return (cases.xi(seed, n, 3) * np.array([[4.0], [4.0], [1.0]], np.float32)).astype(np.float32)


def _lights(oracle, specs):
    lo = [oracle.make_light(**kw) for kw in specs]
    return lo, [R._capi.SphereLight.from_buffer_copy(bytes(l)) for l in lo]


def _sl(v, a, b):
    if isinstance(v, np.ndarray):
        return np.ascontiguousarray(v[..., a:b])
    if isinstance(v, dict):
        return {k: _sl(x, a, b) for k, x in v.items()}
    return v


def make_case(kind, oracle, n, seed=cases.SEED_PARITY):
    """the inputs of one batch of `kind`: numpy planes (and the shader parameters the entry point takes)"""
    u = lambda j: oracle.gen_uniform(seed, 0, n, oracle.S_PARAM0 + 20 + j)
    if kind.startswith("ggx"):
        c = cases.ggx_mixed(seed, n)
        c.update(P=_slab(n, seed), kdc=np.stack([u(j) for j in range(3)]), ktc=np.stack([u(3 + j) for j in range(3)]),
                 kd=u(6), kdr=u(7), ks=u(8), kt=u(9))
    elif kind.startswith("disney"):
        c = dict(cases.disney_mixed(seed, n), P=_slab(n, seed))
    elif kind == "skin":
        c = cases.skin_mixed(seed, n)
        c["P"] = c["N"]
    else:
        c = _sphere_case(oracle, n, 0.35, (0.3, -0.2, 0.1))
    return c


def run_ref(kind, oracle, c, spp_n, seed, first, lights):
    """the oracle's result: dict of numpy planes"""
    nt = _threads(oracle)
    if kind.startswith("ggx"):
        og = ggx_oracle(oracle, c, nthreads=nt)
        sh = dict(Kd_color=c["kdc"], Kd=c["kd"], Kd_roughness=c["kdr"], Ks=c["ks"])
        if kind == "ggx_integrate":
            return dict(zip(("sum", "avg"), og.integrate(spp_n, seed, first_index=first)))
        if kind in ("ggx_refract", "ggx_refract_untraced"):
            return dict(zip(("result", "tir"), og.integrate_refract(spp_n, seed, traced=kind == "ggx_refract", env=ENV,
                                                                    first_index=first)))
        if kind == "ggx_direct":
            return dict(zip(("dd", "ds"), og.direct_lighting(c["P"], lights, spp_n, seed, first_index=first, **sh)))
        return og.shade(c["P"], lights, spp_n, seed, Kt_color=c["ktc"], Kt=c["kt"], env=ENV, traced=True, first_index=first,
                        **sh)
    if kind.startswith("disney"):
        od = disney_oracle(oracle, c, nthreads=nt)
        if kind in ("disney_integrate", "disney_streamed"):
            return od.integrate(spp_n, seed, streamed=kind == "disney_streamed", first_index=first)
        if kind == "disney_direct":
            return dict(zip(("dd", "ds"), od.direct_lighting(c["P"], lights, spp_n, seed, first_index=first)))
        return od.shade(c["P"], lights, spp_n, seed, env=ENV, first_index=first)
    if kind == "skin":
        return oracle.skin_integrate(c["wo"], c["N"], c["T"], c["params"], c["P"], oracle.make_scene(**SKIN_SCENE), spp_n, seed,
                                     env=ENV, first_index=first, nthreads=nt, lights=lights)
    o = oracle.Sss(c["P"].shape[1], c["dist"], c["albedo"], N=c["N"], T=c["T"], nthreads=nt)
    return dict(zip(("result", "depth"), oracle.integrate_scatter(o, c["P"], oracle.make_scene(**SSS_SCENE), spp_n, seed,
                                                                  first_index=first)))


def run_dev(kind, ctx, c, spp_n, seed, first, lights, alloc=None):
    """the device's result: dict of numpy planes.  alloc(shape) -> the float32 tensor an output plane is written to"""
    n = c["P"].shape[1]
    alloc = alloc or ctx.empty
    A3, A1 = (lambda: alloc((3, n))), (lambda: alloc((n,)))
    if kind.startswith("ggx"):
        s = ggx_sampler(ctx, c)
        sh = dict(KdColor=dev(c["kdc"]), Kd=dev(c["kd"]), diffuseRoughness=dev(c["kdr"]), Ks=dev(c["ks"]))
        if kind == "ggx_integrate":
            out = s.integrate(spp_n, seed, out=(A3(), A1()), first_index=first)
            keys = ("sum", "avg")
        elif kind in ("ggx_refract", "ggx_refract_untraced"):
            out = (A3(), A1())
            e = (C.c_float * 3)(*ENV)
            R._capi.check(ctx.lib.rls_ggx_integrate_refract(ctx.handle, n, C.byref(s.c), 1 if kind == "ggx_refract" else 0, e,
                                                            spp_n, seed, first, rgb(out[0], n, "result"),
                                                            plane(out[1], n, "tir")))
            keys = ("result", "tir")
        elif kind == "ggx_direct":
            out = s.directLighting(dev(c["P"]), lights, spp_n, seed, out=(A3(), A3()), first_index=first, **sh)
            keys = ("dd", "ds")
        else:
            o = {k: A3() for k in s.SHADE_AOVS + ("out",)}
            o = s.shade(dev(c["P"]), lights, spp_n, seed, KtColor=dev(c["ktc"]), Kt=dev(c["kt"]), env=ENV, traced=True,
                        out=o, first_index=first, **sh)
            return {k: host(v) for k, v in o.items()}
        return {k: host(v) for k, v in zip(keys, out)}
    if kind.startswith("disney"):
        d = disney_sampler(ctx, c)
        if kind in ("disney_integrate", "disney_streamed"):
            o = {"diffuse_sum": A3(), "diffuse_count": A1(), "specular_sum": A3(), "specular_count": A1()}
            if kind == "disney_streamed":
                m = 2 * spp_n * spp_n * n
                o.update(wi=alloc((3, m)), f=alloc((3, m)), pdf=alloc((m,)))
            o = d.integrate(spp_n, seed, streamed=kind == "disney_streamed", out=o, first_index=first)
        elif kind == "disney_direct":
            o = dict(zip(("dd", "ds"), d.directLighting(dev(c["P"]), lights, spp_n, seed, out=(A3(), A3()), first_index=first)))
        else:
            o = d.shade(dev(c["P"]), lights, spp_n, seed, env=ENV, out={k: A3() for k in d.SHADE_AOVS + ("out",)},
                        first_index=first)
        return {k: host(v) for k, v in o.items()}
    if kind == "skin":
        sk = R.SkinShader(ctx, dev(c["wo"]), dev(c["N"]), dev(c["T"]), **{k: dev(v) for k, v in c["params"].items()})
        o = {k: A3() for k in ("sheen", "specular", "sss", "out")}
        o.update({k: A1() for k in ("sheenFresnel", "specularFresnel", "sssWeight")})
        o = sk.integrate(dev(c["P"]), R.make_scene(**SKIN_SCENE), spp_n, seed, env=ENV, out=o, first_index=first,
                         lights=lights)
        return {k: host(v) for k, v in o.items()}
    s = R.SssSampler(ctx, dev(c["N"]), dev(c["T"]), dev(c["albedo"]), dev(c["dist"]))
    res, depth = s.integrateScatter(dev(c["P"]), R.make_scene(**SSS_SCENE), spp_n, seed, want_depth=True, out=A3(),
                                    first_index=first)
    return {"result": host(res), "depth": host(depth)}


class Batch:
    """one batch of one loop entry point, with the lights it takes (LIGHTS[:nl])"""

    def __init__(self, kind, oracle, n, nl=2, case=None):
        self.kind, self.oracle, self.n = kind, oracle, n
        self.case = case if case is not None else make_case(kind, oracle, n)
        self.lo, self.lg = _lights(oracle, LIGHTS[:nl]) if kind in LIT else (None, None)

    def ref(self, spp_n, seed, first=0, a=0, b=None, nl=None):
        """the oracle on points [a, b) of the batch"""
        b = self.n if b is None else b
        lo = self.lo if nl is None else self.lo[:nl]
        return run_ref(self.kind, self.oracle, _sl(self.case, a, b), spp_n, seed, first + a, lo)

    def dev(self, ctx, spp_n, seed, first=0, alloc=None, nl=None, case=None):
        lg = self.lg if nl is None or self.lg is None else (self.lg[:nl] or None)
        return run_dev(self.kind, ctx, self.case if case is None else case, spp_n, seed, first, lg, alloc)


def _at(monkeypatch, g, fn):
    """fn() with RLS_INTEGRATE_GROUP = g (None: unset, the host picks the width)"""
    if g is None:
        monkeypatch.delenv("RLS_INTEGRATE_GROUP", raising=False)
    else:
        monkeypatch.setenv("RLS_INTEGRATE_GROUP", str(g))
    try:
        return fn()
    finally:
        monkeypatch.delenv("RLS_INTEGRATE_GROUP", raising=False)


def _tight(got, ref, what):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k in ref:
        cases.assert_tight(cases.summarize(cases.rel_err(got[k], ref[k])), (what, k))


def _same(a, b, what):
    for k in b:
        cases.assert_same_bits(a[k], b[k], (what, k))


def _auto_group(ctx, n, spp):
    """pick_group (rls_loops.hpp) restated: the width the host gives a batch of n points with spp samples"""
    want = ctx.device_info()["compute_units"] * 4 * 4 * 64
    g = 1
    while g < 64 and n * g < want and g * 4 <= spp:
        g *= 4
    return g


# ---- A. every spp_n 1..16 at every group width ---------------------------------------------------------------------
def _ragged_n(spp):
    return min(4099, max(259, 65536 // spp + 3))


@pytest.mark.parametrize("spp_n", range(1, 17))
@pytest.mark.parametrize("kind", KINDS)
def test_every_spp_n_at_every_group_width(gpu, oracle, monkeypatch, kind, spp_n):
    """ragged batches, mixed closures, two lights where the entry point takes lights: G = 1 bit-equal to the oracle; 4, 16,
    64 lanes per point (G > spp included) and the host's own choice give the same bits.  Sample counts 1..256 leave the
    last pass of K = 4 samples x G lanes partly empty at every width but the few that divide."""
    spp = spp_n * spp_n
    n, seed, first = _ragged_n(spp), 1000 + spp_n, 12345 + spp_n
    b = Batch(kind, oracle, n)
    base = _at(monkeypatch, 1, lambda: b.dev(gpu, spp_n, seed, first))
    _tight(base, b.ref(spp_n, seed, first), (kind, spp_n))
    if kind in ("ggx_refract", "ggx_refract_untraced"):
        assert base["tir"].min() >= 0 and base["tir"].max() <= 1
    for g in GROUPS + (None,):
        # FORCED_G1: the setting is ignored (traced-free refraction, sample-major streamed planes) -- still the same bits
        _same(_at(monkeypatch, g, lambda: b.dev(gpu, spp_n, seed, first)), base, (kind, spp_n, g))


@pytest.mark.parametrize("spp_n", [5, 16])
def test_chunked_streaming_at_ragged_chunks(gpu, oracle, monkeypatch, spp_n):
    """rls_disney_integrate_chunked with a chunk size that does not divide n: the sums are the unchunked streamed call's,
    every chunk's sample planes are the unchunked planes' columns of its points"""
    spp = spp_n * spp_n
    n, seed, first, cp = _ragged_n(spp), 71, (1 << 32) - 100, 97 if spp_n == 16 else 601
    b = Batch("disney_streamed", oracle, n)
    whole = _at(monkeypatch, 16, lambda: b.dev(gpu, spp_n, seed, first))        # streamed: G = 1 whatever is asked
    _tight(whole, b.ref(spp_n, seed, first), ("streamed", spp_n))
    d = disney_sampler(gpu, b.case)
    got = {k: np.full_like(whole[k], np.nan) for k in ("wi", "f", "pdf")}
    seen = []

    def consume(p0, count, chunk):
        torch.cuda.synchronize()
        seen.append((p0, count))
        for k in got:
            a = host(chunk[k])[..., : 2 * spp * count]
            a = a.reshape(a.shape[:-1] + (2 * spp, count))
            got[k].reshape(got[k].shape[:-1] + (2 * spp, n))[..., p0:p0 + count] = a

    sums, _ = _at(monkeypatch, 64, lambda: d.integrateChunked(spp_n, seed, cp, consume=consume, first_index=first))
    assert n % cp != 0 and seen == [(p, min(cp, n - p)) for p in range(0, n, cp)]
    _same({k: host(v) for k, v in sums.items()}, {k: whole[k] for k in sums}, ("chunked sums", spp_n))
    _same(got, {k: whole[k] for k in got}, ("chunked planes", spp_n))


# ---- B. the LDS queues full ------------------------------------------------------------------------------------------
def _upright(n, roughness):
    """unperturbed frames (N = z, T = x), views along the normal: theta = 0, every visible-normal sample takes the
    uniform-slope fallback; the shading points at the origin, under the centre of the light"""
    N = np.tile(np.array([[0.0], [0.0], [1.0]], np.float32), (1, n))
    T = np.tile(np.array([[1.0], [0.0], [0.0]], np.float32), (1, n))
    return N.copy(), N, T, np.zeros((3, n), np.float32), np.full(n, roughness, np.float32)


SAT_LIGHT = dict(center=(0.0, 0.0, 1.0), radius=0.9999, radiance=(1.0, 2.0, 3.0), mis_mode=0)   # an 89.2-degree half angle


def _view_near_normal(c, alpha_x, alpha_y):
    """vndf_view's test from the inputs, in float64: the stretched view within 1e-4 of the normal (nearNormal)"""
    wo, N, T = (np.asarray(c[k], np.float64) for k in ("wo", "N", "T"))
    B = np.cross(N.T, T.T).T
    v = np.stack([(wo * T).sum(0) * alpha_x, (wo * B).sum(0) * alpha_y, (wo * N).sum(0)])
    return v[2] / np.linalg.norm(v, axis=0) > 1.0 - 1e-5


def _cone(P, light):
    d = np.asarray(light["center"], np.float64)[:, None] - P.astype(np.float64)
    dist = np.linalg.norm(d, axis=0)
    return d / dist, np.arcsin(np.minimum(1.0, light["radius"] / dist)), dist > light["radius"]


def _full_passes(flags, g):
    """flags [spp, n] (n a multiple of 64 / g): the fraction of (wavefront, pass of 4 samples x g lanes) whose 256 queue
    slots are all asked for -- one wavefront holds 64 / g points"""
    spp, n = flags.shape
    per = 4 * g
    f = flags[: spp // per * per].reshape(spp // per, per, n // (64 // g), 64 // g)
    return float(f.all(axis=(1, 3)).mean())


@pytest.mark.parametrize("kind", ["ggx_integrate", "ggx_refract", "disney_integrate", "ggx_direct", "disney_direct"])
def test_saturated_queues(gpu, oracle, monkeypatch, kind):
    """every lane queues at every sample: views along the normal (the uniform-slope fallback of visible-normal sampling in
    rlGgx glossy, refraction and the rlDisney specular lobe, with clearcoat = 1 sending samples to the clearcoat lobe) and,
    for the light loops, one light that fills most of the upper hemisphere above unperturbed frames at low roughness
    (every light sample above the horizon, nearly every BSDF sample on the light).  spp_n = 16: a pass of G = 64 lanes holds
    the 256 samples.  Reduced mode at G = 1 bit-equal to the oracle, 4 / 16 / 64 the same bits."""
    n, spp_n, seed = 1024, 16, 5
    spp = spp_n * spp_n
    # low roughness where BSDF samples are to hit the light; elsewhere rough enough that every sample's weight depends on
    # its microfacet normal (at 0.05 the refraction weight of a view along the normal is 1 for every sample)
    wo, N, T, P, rough = _upright(n, 0.05 if kind in LIT else 0.5)
    base = make_case(kind, oracle, n, cases.SEED_EDGE)
    if kind.startswith("ggx"):
        c = dict(base, wo=wo, N=N, T=T, P=P, roughness=rough, anisotropic=np.zeros(n, np.float32))
        alpha = np.float64(rough[0]) ** 2
    else:
        c = dict(base, wo=wo, N=N, T=T, P=P, roughness=rough, anisotropic=np.zeros(n, np.float32),
                 clearcoat=np.ones(n, np.float32), clearcoat_gloss=np.ones(n, np.float32))
        alpha = max(np.float64(rough[0]) ** 2, 1e-3)
    # the fallback queue: every point's every visible-normal sample
    assert _view_near_normal(c, alpha, alpha).all()
    b = Batch(kind, oracle, n, nl=0, case=c)
    if kind in LIT:
        b.lo, b.lg = _lights(oracle, [SAT_LIGHT])
        axis, half, valid = _cone(P, SAT_LIGHT)
        # the light-sample queue: the whole cone above the horizon at every point
        assert valid.all() and (np.arccos(np.clip(axis[2], -1, 1)) + half < np.radians(89.5)).all()
        # the hit queue: the oracle's own BSDF samples (dimension pair 3 l + 1: GGX specular, rlDisney diffuse)
        og = ggx_oracle(oracle, c) if kind == "ggx_direct" else None
        od = disney_oracle(oracle, c) if kind == "disney_direct" else None
        hits = np.zeros((spp, n), bool)
        for s in range(spp):
            rx, ry = oracle.batch_sample_02(seed, 0, n, 1, s)
            L = og.sample(rx, ry)[0] if og is not None else od.sample(oracle.RAY_DIFFUSE, rx, ry)
            L = L.astype(np.float64)
            ang = np.arccos(np.clip((L * axis).sum(0) / np.maximum(np.linalg.norm(L, axis=0), 1e-30), -1, 1))
            hits[s] = (L[2] > 0) & (ang < half - 1e-3)
        print(kind, "BSDF samples on the light", hits.mean(), "full passes G=1", _full_passes(hits, 1),
              "G=64", _full_passes(hits, 64))
        assert hits.mean() > 0.995 and _full_passes(hits, 1) > 0.5 and _full_passes(hits, 64) > 0.5
    got = _at(monkeypatch, 1, lambda: b.dev(gpu, spp_n, seed))
    _tight(got, b.ref(spp_n, seed), ("saturated", kind))
    for k, v in got.items():
        assert np.isfinite(v).all() and (k == "tir" or (v != 0).any()), (kind, k)    # no TIR looking along the normal
    for g in GROUPS:
        _same(_at(monkeypatch, g, lambda: b.dev(gpu, spp_n, seed)), got, ("saturated", kind, g))


# ---- C. one to eight lights ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LIT)
def test_light_counts_one_to_eight(gpu, oracle, monkeypatch, kind):
    """lights 0..7 each draw their own hash streams (kScrambleStream + 6 l + k; rlSkin's stream + 4 l per lobe) ahead of the
    whole nodes' kShadeStream = 3 RLS_MAX_LIGHTS: every count against the oracle, the direct AOVs growing as lights are
    appended (every light adds a non-negative term), and the whole nodes without lights keep every other AOV"""
    n, spp_n, seed, first = 2053, 3, 17, 1 << 34
    b = Batch(kind, oracle, n, nl=8)
    direct = {"ggx_direct": ("dd", "ds"), "disney_direct": ("dd", "ds"), "skin": ("specular", "sheen")}.get(
        kind, ("direct_diffuse", "direct_specular"))
    prev = None
    for nl in range(1, 9):
        got = _at(monkeypatch, 1, lambda: b.dev(gpu, spp_n, seed, first, nl=nl))
        _tight(got, b.ref(spp_n, seed, first, nl=nl), (kind, nl))
        if prev is not None and kind != "skin":
            for k in direct:
                assert (got[k] >= prev[k]).all(), (kind, nl, k)
        prev = got
    assert (prev[direct[1]] > 0).mean() > 0.1
    _same(_at(monkeypatch, 16, lambda: b.dev(gpu, spp_n, seed, first, nl=8)), prev, (kind, "8 lights G=16"))
    if kind in ("ggx_shade", "disney_shade"):
        dark = _at(monkeypatch, 1, lambda: b.dev(gpu, spp_n, seed, first, nl=0))
        for k in dark:
            if k.startswith("direct"):
                assert not dark[k].any(), k
            elif k != "out":
                cases.assert_same_bits(dark[k], prev[k], (kind, "no lights", k))


# ---- D. several rounds of the grid-stride loop -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_block_per_cu():
    """a context whose grids are capped at one workgroup per CU (RLS_BLOCKS_PER_CU, read at context creation)"""
    mp = pytest.MonkeyPatch()
    mp.setenv("RLS_BLOCKS_PER_CU", "1")
    try:
        ctx = R.Context(0)
    finally:
        mp.undo()
    yield ctx
    ctx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_several_grid_rounds(gpu, oracle, monkeypatch, one_block_per_cu, kind):
    """one workgroup per CU: a round of the loop covers compute_units x 256 / G points, and n is sized so that G = 1 runs
    three and a half rounds (G = 64 runs 224): every dead lane clamped to point n - 1, the per-round indices and hash
    streams.  The same bits as the default context at every G; the oracle on windows across G = 1's round boundaries and
    at the tail."""
    ctx = one_block_per_cu
    cu = ctx.device_info()["compute_units"]
    rnd = cu * 256
    n, spp_n, seed, first = 3 * rnd + rnd // 2 + 37, 2, 23, 777
    b = Batch(kind, oracle, n)
    base = None
    for g in (1,) + GROUPS:
        got = _at(monkeypatch, g, lambda: b.dev(ctx, spp_n, seed, first))
        _same(got, _at(monkeypatch, g, lambda: b.dev(gpu, spp_n, seed, first)), (kind, "rounds vs default", g))
        if base is None:
            base = got
        else:
            _same(got, base, (kind, "rounds", g))
    m = 2 * spp_n * spp_n
    for a in [k * rnd - 70 for k in (1, 2, 3)] + [n - 141]:
        bb = min(n, a + 141)
        ref = b.ref(spp_n, seed, first, a, bb)
        win = {}
        for k, v in base.items():
            if v.shape[-1] == n:
                win[k] = v[..., a:bb]
            else:                                                    # streamed planes: [.., 2 spp, n] sample-major
                win[k] = v.reshape(v.shape[:-1] + (m, n))[..., a:bb].reshape(v.shape[:-1] + (m * (bb - a),))
        _tight(win, ref, (kind, "window", a))


# ---- E. automatic width, the words beside the planes, first_index across 2^32 ------------------------------------------
@pytest.mark.parametrize("kind", ["ggx_integrate", "ggx_refract", "disney_integrate", "ggx_direct", "disney_shade", "skin",
                                  "sss"])
def test_automatic_width_gives_the_one_lane_bits(gpu, oracle, monkeypatch, kind):
    """RLS_INTEGRATE_GROUP unset: batches for which pick_group chooses 4, 16 and 64 lanes per point give the G = 1 bits"""
    seen = set()
    for n, spp_n in ((1001, 2), (1001, 4), (1001, 8), (333, 16)):
        g = _auto_group(gpu, n, spp_n * spp_n)
        seen.add(g)
        b = Batch(kind, oracle, n)
        one = _at(monkeypatch, 1, lambda: b.dev(gpu, spp_n, 3, 9))
        _same(_at(monkeypatch, None, lambda: b.dev(gpu, spp_n, 3, 9)), one, (kind, n, spp_n, "auto", g))
    assert seen == {4, 16, 64}, seen


SENTINEL = 0x7FC0DEAD            # a quiet NaN with a payload: no kernel writes it


@pytest.mark.parametrize("kind", KINDS)
def test_output_planes_leave_the_words_beside_them(gpu, oracle, monkeypatch, kind):
    """every output plane a view inside a larger buffer filled with a sentinel: the words before and after each row are
    untouched, the view holds the bits of the plain call"""
    n, spp_n, seed, pad = 1001, 3, 11, 67
    b = Batch(kind, oracle, n)
    for g in (1, 64):
        plain = _at(monkeypatch, g, lambda: b.dev(gpu, spp_n, seed))
        bufs = []

        def alloc(shape):
            rows = shape[:-1]
            buf = torch.full(rows + (shape[-1] + 2 * pad,), SENTINEL, dtype=torch.int32, device="cuda")
            bufs.append((buf, shape[-1]))
            return buf.view(torch.float32)[..., pad:pad + shape[-1]]

        got = _at(monkeypatch, g, lambda: b.dev(gpu, spp_n, seed, alloc=alloc))
        _same(got, plain, (kind, g, "in a padded buffer"))
        for buf, w in bufs:
            h = host(buf)
            assert (h[..., :pad] == SENTINEL).all() and (h[..., pad + w:] == SENTINEL).all(), (kind, g, h.shape)


@pytest.mark.parametrize("kind", KINDS)
def test_first_index_across_two_to_the_32(gpu, oracle, monkeypatch, kind):
    """points 2^32 - n/2 .. 2^32 + n/2 - 1 in one batch: the low word of the point index wraps inside it.  Against the
    oracle, and against two shards split at the wrap"""
    n, spp_n, seed = 2048, 3, 8
    first = (1 << 32) - n // 2
    b = Batch(kind, oracle, n)
    for g in (1, 16):
        whole = _at(monkeypatch, g, lambda: b.dev(gpu, spp_n, seed, first))
        if g == 1:
            _tight(whole, b.ref(spp_n, seed, first), (kind, "across 2^32"))
        h = n // 2
        lo = _at(monkeypatch, g, lambda: b.dev(gpu, spp_n, seed, first, case=_sl(b.case, 0, h)))
        hi = _at(monkeypatch, g, lambda: b.dev(gpu, spp_n, seed, 1 << 32, case=_sl(b.case, h, n)))
        for k in whole:
            if k in ("wi", "f", "pdf"):
                m = 2 * spp_n * spp_n
                sh = whole[k].shape[:-1]
                joined = np.concatenate([lo[k].reshape(sh + (m, h)), hi[k].reshape(sh + (m, n - h))], axis=-1).reshape(
                    whole[k].shape)
            else:
                joined = np.concatenate([lo[k], hi[k]], axis=-1)
            cases.assert_same_bits(joined, whole[k], (kind, g, "shards at 2^32", k))


# ---- F. FAST mode at the edges ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fast():
    ctx = R.Context(0)
    ctx.set_math_mode(True)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("spp_n", [1, 7, 16])
@pytest.mark.parametrize("kind", ["ggx_direct", "disney_direct", "ggx_shade", "disney_shade", "skin"])
def test_fast_mode_at_the_edges(fast, oracle, kind, spp_n):
    """the FAST instantiations of the same templates at spp_n 1, 7, 16 and eight lights, under test_gpu_fast_mode.py's
    gates: finite, batch means within 5e-3, 90 % of the points within 1e-3 (2e-3 for the whole nodes)"""
    n, seed = 4096 if spp_n < 16 else 1024, 29
    b = Batch(kind, oracle, n, nl=8)
    got, ref = b.dev(fast, spp_n, seed), b.ref(spp_n, seed)
    q90 = 2e-3 if kind.endswith("shade") else 1e-3
    for k in ref:
        a, r = got[k].astype(np.float64), ref[k].astype(np.float64)
        assert np.isfinite(a).all(), (kind, k)
        if kind == "skin" and k in ("sheenFresnel", "specularFresnel", "sssWeight"):
            st = cases.summarize(cases.rel_err(got[k], ref[k]))
            assert st["nonfinite"] == 0 and st["median"] <= 1e-5 and st["p99"] <= 1e-3, (k, st)
            continue
        assert abs(a.mean() / r.mean() - 1) < 5e-3, (kind, k, a.mean(), r.mean())
        if kind != "skin":
            assert np.quantile(cases.rel_err(got[k], ref[k]), 0.9) <= q90, (kind, k)
