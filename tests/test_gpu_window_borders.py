"""GPU: every window guard of the EXACT arithmetic crossed through a public verb, against the oracle.

The windowed primitives of csrc/rls_libm.hpp (rcp32_w, rcp32_hi, div32_m, div32_y, div32_const_w, the unguarded square roots,
exp32_in_range) are correct only inside stated operand windows, and each caller in csrc/rls_device.hpp / csrc/rls_loops.hpp
guarantees its window by construction or with a compare.  tests/test_gpu_libm_primitives.py holds the primitives to IEEE
inside the windows; here the CALLERS are driven to both sides of every border: batches of a few thousand points with border
values interleaved among ordinary ones (wavefronts mix both kinds), and for material parameters the same values as UNIFORM
parameters, one small launch each (the hoisted path keeps the reciprocals in scalar registers).  Comparison: the same NaN
pattern, and the same bits elsewhere under cases.strict_parity() (tests/test_gpu_hostile_inputs.py, _same).

Call sites of windowed primitives and the test that crosses their border (functions of csrc/rls_device.hpp unless said):

| site                                                                  | primitive              | crossed by |
|---|---|---|
| normalize (R_RCPW of the length)                                      | rcp32_w                | test_normalize_of_scaled_vectors |
| normalize_h (R_RCPH: half vector, microfacet normal)                  | rcp32_w                | test_normalize_of_scaled_vectors |
| spherical_direction (R_SQRT1M(cos^2))                                 | sqrt32_1m              | test_smith_g1_at_grazing_directions (N.wo = 0, +-tiny: cos^2 underflows), test_normalize_of_scaled_vectors (clamped cosines of +-1) |
| vndf_view_from: G1 = R_TWO_OVER(1 + R_SQRT1P(B^2)), invB = R_RCPW(B)  | rcp32_w, sqrt32_1p     | test_smith_g1_at_grazing_directions (views at and beside the horizon: B up to 2.3e7), test_uniform_slope_borders (near-normal: B = 0) |
| vndf_view_from: yG1 (G1 >= 2^-14) and div32_y(2 rx, G1, yG1)          | rcp32_w, div32_y       | test_gpu_disney_config3.py::test_loop_reciprocals_at_their_window_borders (grazing views) |
| ratio_to_one_minus (2^-60 <= rx < 1)                                  | div32_m                | test_uniform_slope_borders |
| slope_y_ratio (u <= 1)                                                | div32_m                | test_second_slope_borders |
| vndf_slope_closed: R_RCPG(A^2 - 1), the fallback threshold            | rcp32_hi               | test_closed_form_slope_beside_its_poles |
| vndf_slope_closed: R_SQRTH1P(slope.x^2)                               | sqrt32_1p              | test_closed_form_slope_beside_its_poles (slopes from 0 to inf) |
| ggx_material: R_SQRT1M(anisotropic * 0.9), R_RCPHI(max(ior, 1e-4))    | sqrt32_1m, rcp32_hi    | test_ggx_material_borders |
| ggx_from_material / ggx_G1: R_RCP(cos^2), R_TWO_OVER(1 + R_SQRT1P())  | rcp32, rcp32_w, sqrt32_1p | test_smith_g1_at_grazing_directions |
| disney_make_scalars: R_SQRT1M(anisotropic * 0.9)                      | sqrt32_1m              | test_disney_one_sample_verbs_at_the_reciprocal_borders |
| disney_prepare_material (yax, yay, yW, y1mW) and D_GTR2Aniso          | rcp32_w, div32_y       | test_disney_one_sample_verbs_at_the_reciprocal_borders; the n^2-spp loops: test_gpu_disney_config3.py::test_loop_reciprocals_at_their_window_borders |
| disney_gtr1_microfacet / slow_eval: R_SQRT1M(ry) at a2 == 1, R_SQRT1M(cos^2) | sqrt32_1m       | test_disney_one_sample_verbs_at_the_reciprocal_borders (roughness beside 1, one-sample verbs and integrate) |
| slow_eval: ratio_to_one_minus(q) of the loops                         | div32_m                | test_disney_one_sample_verbs_at_the_reciprocal_borders (integrate: q from the in-kernel sampler, 0 included) |
| rls_loops.hpp, disney_spec_push: div32_y(num, den, yW / y1mW)         | div32_y                | test_gpu_disney_config3.py::test_loop_reciprocals_at_their_window_borders |
| nd_make, nd_pdf, nd_profile, nd_pdf_profile_t (ydm, ycw, q = -r / d, exp32_in_range_3, R_EXP_IN_RANGE, R_DIVCW(q, 3)) | rcp32_w, div32_y, exp32_in_range, div32_const_w | test_gpu_sss_skin.py::test_nd_profile_across_the_reciprocal_window |
| cone_make: R_RCPW(sqrt(dist^2))                                       | rcp32_w                | test_light_cone_at_extreme_distances |
"""
import os

import numpy as np
import pytest

import cases
import libm_probe_util as U
import rlshaders_amd as R
import rr_wg_util
from gpu_util import dev, disney_oracle, disney_sampler, ggx_oracle, ggx_sampler, host

pytestmark = pytest.mark.gpu
F = np.float32
N = 1 << 12
GGX_NAMES = ("wi", "f", "pdf", "fresnel", "wt", "weight")


def _same(got, ref, what):
    got, ref = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    assert np.array_equal(nan_g, nan_r), (what, "NaN pattern", int((nan_g != nan_r).sum()))
    ok = ~nan_r
    diff = got.view(np.uint32)[ok] != ref.view(np.uint32)[ok]
    if cases.strict_parity():
        assert not diff.any(), (what, int(diff.sum()), "of", int(ok.sum()), got[ok][diff][:4], ref[ok][diff][:4])
    else:       # the host libm is not the build the device follows: one point of a batch may differ (cases.assert_tight)
        assert int(diff.sum()) <= 3 * cases.flag_slack(), (what, int(diff.sum()))


def _with_group(g, fn):
    """the n^2-spp loops with g lanes per point; 1 adds in the reference's order (tests/test_gpu_disney_config3.py)"""
    os.environ["RLS_INTEGRATE_GROUP"] = str(g)
    try:
        return fn()
    finally:
        del os.environ["RLS_INTEGRATE_GROUP"]


def _spread(n, values, every=3):
    """-> (mask of the lanes that take a border value, the value each of them takes): every `every`-th lane, cycling"""
    k = np.arange(n)
    m = (k % every) == 0
    v = np.asarray(values, dtype=np.float32)
    return m, v[(k[m] // every) % v.size]


def _ggx_sampling_verbs(gpu, oracle, c, x, what, expect_nan=False):
    """rls_ggx_microfacet, rls_ggx_sample and rls_ggx_reflect_refract (the streamed launch of the companion kernel)"""
    og, s = ggx_oracle(oracle, c), ggx_sampler(gpu, c)
    ref = og.microfacet(x[0], x[1])
    assert bool(np.isnan(ref).any()) == expect_nan, (what, "the values beyond the guard reach the outputs")
    _same(host(s.microfacet(dev(x[0]), dev(x[1]))), ref, f"{what} microfacet")
    for nm, a, b in zip(("wi", "fresnel"), s.evalSample(dev(x[0]), dev(x[1])), og.sample(x[0], x[1])):
        _same(host(a), b, f"{what} sample {nm}")
    for nm, a, b in zip(GGX_NAMES, s.reflectRefract(*(dev(x[k]) for k in range(4))), og.reflect_refract(*x[:4])):
        _same(host(a), b, f"{what} reflect_refract {nm}")


def test_uniform_slope_borders(gpu, oracle):
    """ratio_to_one_minus: near-normal points (wo = N, roughness 0.1: both samples take the uniform slope) whose rx sits on
    either side of 2^-60 and of 1"""
    rx = [0.0, 2.0 ** -149, 2.0 ** -126, U.step(U.pow2(-60), -1), 2.0 ** -60, U.step(U.pow2(-60), 1), 0.5, 1.0 - 2.0 ** -24, 1.0,
          U.step(F(1.0), 1), 2.0, -(2.0 ** -60)]
    c, x = rr_wg_util.mixed(N)
    m, v = _spread(N, rx)
    rr_wg_util._near_normal(c, m)
    x[0][m] = v
    x[2][m] = np.roll(v, 5)
    _ggx_sampling_verbs(gpu, oracle, c, x, "uniform slope", expect_nan=True)       # rx > 1: the square root of a negative ratio


def test_second_slope_borders(gpu, oracle):
    """slope_y_ratio: quiet points (closed-form slopes, no fallback) whose ry makes u = 2 |ry - 1/2| 0, tiny, 1 and beyond"""
    ry = [0.0, 2.0 ** -149, U.step(F(0.5), -1), 0.5, U.step(F(0.5), 1), 1.0 - 2.0 ** -24, 1.0, U.step(F(1.0), 1), -(2.0 ** -24), 2.0]
    c, x = rr_wg_util.mixed(N)
    m, v = _spread(N, ry)
    rr_wg_util._quiet(c, x, m)
    x[1][m] = v
    x[3][m] = np.roll(v, 3)
    _ggx_sampling_verbs(gpu, oracle, c, x, "second slope")


def test_closed_form_slope_beside_its_poles(gpu, oracle):
    """R_RCPG(A^2 - 1) and the |A^2 - 1| < 1e-4 fallback: quiet points with rx = G1 (1 + k 2^-24), |k| <= 64 (A beside 1),
    rx = k 2^-30, k <= 64 (A beside -1), and rx = 1e30 (A^2 overflows)"""
    c, x = rr_wg_util.mixed(N)
    m = (np.arange(N) % 2) == 0
    rr_wg_util._quiet(c, x, m)
    g1 = rr_wg_util._view(c)[3]                                  # float64 (tests/twin64.py's arithmetic)
    idx = np.flatnonzero(m)
    k = (np.arange(idx.size) % 129) - 64
    beside_one = (g1[idx] * (1.0 + k * 2.0 ** -24)).astype(np.float32)
    beside_minus_one = ((np.arange(idx.size) % 65) * 2.0 ** -30).astype(np.float32)
    third = np.arange(idx.size) % 3
    v = np.where(third == 0, beside_one, np.where(third == 1, beside_minus_one, F(1e30))).astype(np.float32)
    x[0][idx] = v
    x[2][idx] = np.roll(v, 1)
    # the batch holds A on both sides of each pole and inside the fallback band (float64 restatement)
    A = 2.0 * x[0][idx].astype(np.float64) / g1[idx] - 1.0
    band = np.abs(A * A - 1.0) < 1e-4
    assert band.any() and (~band).any() and (A[third == 0] > 1).any() and (A[third == 0] < 1).any()
    _ggx_sampling_verbs(gpu, oracle, c, x, "closed form", expect_nan=True)         # rx = 1e30: inf - inf


SCALES = (-80, -75, -74, -64, -63, 62, 63, 64)


def _scaled(v, m, e):
    out = v.copy()
    out[:, m] = (v[:, m] * np.ldexp(F(1.0), e)[None, :]).astype(np.float32)
    return out


def test_normalize_of_scaled_vectors(gpu, oracle):
    """normalize / normalize_h: the view (and the incident direction, the frame of the probe) scaled by 2^k, so that squared
    lengths underflow to 0, are subnormal, or overflow to infinity"""
    k = np.arange(N)
    m = (k % 3) == 0
    e = np.asarray(SCALES)[(k[m] // 3) % len(SCALES)]
    c = cases.ggx_mixed(cases.SEED_EDGE, N)
    x = cases.xi(cases.SEED_EDGE, N, 4)
    wi_unit = ggx_oracle(oracle, c).sample(x[0], x[1])[0]
    c["wo"] = _scaled(c["wo"], m, e)
    og, s = ggx_oracle(oracle, c), ggx_sampler(gpu, c)
    for nm, a, b in zip(("wi", "fresnel"), s.evalSample(dev(x[0]), dev(x[1])), og.sample(x[0], x[1])):
        _same(host(a), b, f"scaled view: ggx sample {nm}")
    for wi, tag in ((wi_unit, "unit wi"), (_scaled(wi_unit, m, e), "scaled wi")):
        _same(host(s.evalBrdf(dev(wi))), og.eval(wi), f"scaled view, {tag}: ggx eval")
    d = cases.disney_mixed(cases.SEED_EDGE, N)
    d["wo"] = _scaled(d["wo"], m, e)
    od, ds = disney_oracle(oracle, d), disney_sampler(gpu, d)
    for lobe in (R.RLS_RAY_DIFFUSE, R.RLS_RAY_GLOSSY):
        ds.setSampleType(lobe)
        for nm, a, b in zip(("wi", "f", "pdf"), ds.sampleEvalPdf(dev(x[0]), dev(x[1])), od.sample_eval_pdf(lobe, x[0], x[1])):
            _same(host(a), b, f"scaled view: disney {lobe} {nm}")
    p = cases.sss_mixed(cases.SEED_EDGE, N)
    Ns, Ts = _scaled(p["N"], m, e), _scaled(p["T"], m, np.roll(e, 1))
    ref = oracle.Sss(N, p["dist"], p["albedo"], N=Ns, T=Ts, nthreads=4).probe(x[0], x[1])
    got = R.SssSampler(gpu, dev(Ns), dev(Ts), dev(p["albedo"]), dev(p["dist"])).getProbeRay(dev(x[0]), dev(x[1]))
    for key in ("r", "origin", "dir", "maxdist", "pdf", "profile"):
        _same(host(got[key]), ref[key], f"scaled frame: sss probe {key}")


IOR = [1e-5, U.step(F(1e-4), -1), 1e-4, U.step(F(1e-4), 1), U.step(U.pow2(126), -1), 2.0 ** 126, U.step(U.pow2(126), 1), 3e38]
ANISO = [1.0, U.step(F(1.0) / F(0.9), -1), F(1.0) / F(0.9), U.step(F(1.0) / F(0.9), 1), 1.2]
ROUGH = [2.0 ** -63, 2.0 ** -75, 1e19, 2.0 ** 63, 2.0 ** 64]


def _ggx_material_verbs(gpu, oracle, c_dev, c_ref, x, exiting, what):
    og, s = ggx_oracle(oracle, c_ref, exiting=exiting), ggx_sampler(gpu, c_dev, exiting=exiting)
    for nm, a, b in zip(("wi", "f", "pdf", "fresnel"), s.sampleEvalPdf(dev(x[0]), dev(x[1])), og.sample_eval_pdf(x[0], x[1])):
        _same(host(a), b, f"{what} sample_eval_pdf {nm}")
    for nm, a, b in zip(GGX_NAMES, s.reflectRefract(*(dev(x[k]) for k in range(4))), og.reflect_refract(*x[:4])):
        _same(host(a), b, f"{what} reflect_refract {nm}")


def test_ggx_material_borders(gpu, oracle):
    """ggx_material: max(ior, 1e-4) and its reciprocal up to and beyond 2^126 (rcp32_hi's only test), sqrtf(1 - 0.9 anisotropic)
    where the radicand is tiny, zero and negative, roughness whose square under- and overflows; streamed and uniform"""
    c = cases.ggx_mixed(cases.SEED_EDGE, N)
    x = cases.xi(cases.SEED_EDGE, N, 4)
    exiting = (np.arange(N) % 2).astype(np.uint8)
    k = np.arange(N)
    for key, vals, lane in (("ior", IOR, 0), ("anisotropic", ANISO, 1), ("roughness", ROUGH, 2)):
        m = (k % 4) == lane
        c[key] = c[key].copy()
        c[key][m] = np.asarray(vals, dtype=np.float32)[(k[m] // 4) % len(vals)]
    _ggx_material_verbs(gpu, oracle, c, c, x, exiting, "streamed material")
    n = 256
    base = dict(ior=1.5, roughness=0.4, anisotropic=0.3)
    geo = {kk: c[kk][..., :n].copy() for kk in ("wo", "N", "T")}
    xs = np.ascontiguousarray(x[:, :n])
    for key, vals in (("ior", IOR), ("anisotropic", ANISO), ("roughness", ROUGH)):
        for v in vals:
            p = dict(base, **{key: float(F(v))})
            c_dev = dict(geo, KsColor=(0.9, 0.8, 0.7), **p)
            c_ref = dict(geo, KsColor=(0.9, 0.8, 0.7), **{kk: np.full(n, vv, np.float32) for kk, vv in p.items()})
            _ggx_material_verbs(gpu, oracle, c_dev, c_ref, xs, exiting[:n].copy(), f"uniform {key} = {v!r}")


COSINES = [0.0, 2.0 ** -75, -(2.0 ** -75), 2.0 ** -64, U.step(U.pow2(-63), -1), 2.0 ** -63, U.step(U.pow2(-63), 1), 1e-20]


def test_smith_g1_at_grazing_directions(gpu, oracle):
    """G1's R_RCP(cos^2) and R_TWO_OVER: N . wi, then N . wo, exactly 0, +-2^-75, 2^-64, beside 2^-63 (cos^2 beside 2^-126, the
    border of rcp32) and 1e-20.  The frame of those lanes is axis aligned, so the dot product IS the third component."""
    c = cases.ggx_mixed(cases.SEED_EDGE, N)
    x = cases.xi(cases.SEED_EDGE, N, 2)
    wi = ggx_oracle(oracle, c).sample(x[0], x[1])[0]
    k = np.arange(N)
    graze = np.zeros((3, N), np.float32)
    graze[0] = 1.0
    for which, lane in (("wi", 0), ("wo", 1)):
        m = (k % 4) == lane
        cosv = np.asarray(COSINES, dtype=np.float32)[(k[m] // 4) % len(COSINES)]
        both = (k % 4) < 2
        c["N"][:, both] = np.array([[0.0], [0.0], [1.0]], np.float32)
        c["T"][:, both] = np.array([[1.0], [0.0], [0.0]], np.float32)
        g = graze[:, m].copy()
        g[2] = cosv
        other = np.array([[0.3], [0.4], [np.sqrt(0.75)]], np.float32)
        if which == "wi":
            wi[:, m] = g
            c["wo"][:, m] = other
        else:
            c["wo"][:, m] = g
            wi[:, m] = other
    og, s = ggx_oracle(oracle, c), ggx_sampler(gpu, c)
    _same(host(s.evalBrdf(dev(wi))), og.eval(wi), "grazing: ggx eval")
    _same(host(s.evalPdf(dev(wi))), og.pdf(wi), "grazing: ggx pdf")
    # the grazing VIEWS through the sampling verbs too: the stretched view at the horizon (tanf of an angle beside pi / 2)
    for nm, a, b in zip(("wi", "fresnel"), s.evalSample(dev(x[0]), dev(x[1])), og.sample(x[0], x[1])):
        _same(host(a), b, f"grazing: ggx sample {nm}")


def _clearcoat_complement_border():
    """the smallest clearcoat parameter p whose lobe-weight complement 1 - 1 / (0.25 p + 1) reaches 2^-14 in fp32"""
    def w2(p):
        return F(1.0) - F(1.0) / (F(p) * F(0.25) + F(1.0))
    lo, hi = U.ubits(F(1e-4)), U.ubits(F(1e-3))
    assert w2(U.from_bits(np.uint32(lo))[0]) < U.pow2(-14) <= w2(U.from_bits(np.uint32(hi))[0])
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if w2(U.from_bits(np.uint32(mid))[0]) >= U.pow2(-14):
            hi = mid
        else:
            lo = mid
    return U.from_bits(np.uint32(hi))[0]


def _around3(v):
    return [U.step(F(v), -1), F(v), U.step(F(v), 1)]


def test_disney_one_sample_verbs_at_the_reciprocal_borders(gpu, oracle):
    """D_GTR2Aniso's reciprocals and the lobe weights in rls_disney_eval / _pdf / _sample_eval_pdf (the existing border test
    drives integrate only): alpha = roughness^2 beside 2^14 at anisotropic 0; clearcoat beside the values that make the lobe
    weight 1 / (0.25 clearcoat + 1), and its complement, exactly 2^-14 (4 x 16383 and ~2.44e-4 -- and 16383 itself, the value
    that would do it without the node's factor 0.25); roughness beside 1 (a2 == 1 selects sqrtf(1 - ry)); anisotropic beside
    1 / 0.9; half vectors whose tangent component is exactly +0 and -0.  Streamed, then uniform."""
    pc = _clearcoat_complement_border()
    rough = _around3(128.0) + _around3(1.0)
    coat = _around3(16383.0) + _around3(4 * 16383.0) + _around3(pc) + _around3(pc / 4)
    d = cases.disney_mixed(cases.SEED_EDGE, N)
    x = cases.xi(cases.SEED_EDGE, N, 2)
    k = np.arange(N)
    for key in ("roughness", "clearcoat", "anisotropic", "wo", "N", "T"):
        d[key] = d[key].copy()
    m = (k % 4) == 0
    d["roughness"][m] = np.asarray(rough, np.float32)[(k[m] // 4) % len(rough)]
    d["anisotropic"][m] = 0.0
    m = (k % 4) == 1
    d["clearcoat"][m] = np.asarray(coat, np.float32)[(k[m] // 4) % len(coat)]
    m = (k % 4) == 2
    d["anisotropic"][m] = np.asarray(ANISO, np.float32)[(k[m] // 4) % len(ANISO)]
    wi = {lobe: disney_oracle(oracle, d).sample(lobe, x[0], x[1]) for lobe in (R.RLS_RAY_DIFFUSE, R.RLS_RAY_GLOSSY)}
    # h . U exactly +0 / -0: an axis-aligned frame, view and incident direction in the plane x = 0; U = (-1, -0, -0) turns
    # the three products of the dot into -0
    m = (k % 8) == 3
    neg = m & ((k // 8) % 2 == 1)
    d["N"][:, m] = np.array([[0.0], [0.0], [1.0]], np.float32)
    d["T"][:, m] = np.array([[1.0], [0.0], [0.0]], np.float32)
    d["T"][:, neg] = np.array([[-1.0], [-0.0], [-0.0]], np.float32)
    d["wo"][:, m] = np.array([[0.0], [0.6], [0.8]], np.float32)
    for lobe in wi:
        wi[lobe][:, m] = np.array([[0.0], [0.28], [0.96]], np.float32)
    od, ds = disney_oracle(oracle, d), disney_sampler(gpu, d)
    for lobe in (R.RLS_RAY_DIFFUSE, R.RLS_RAY_GLOSSY):
        ds.setSampleType(lobe)
        _same(host(ds.evalBrdf(dev(wi[lobe]))), od.eval(lobe, wi[lobe]), f"disney {lobe} eval")
        _same(host(ds.evalPdf(dev(wi[lobe]))), od.pdf(lobe, wi[lobe]), f"disney {lobe} pdf")
        for nm, a, b in zip(("wi", "f", "pdf"), ds.sampleEvalPdf(dev(x[0]), dev(x[1])), od.sample_eval_pdf(lobe, x[0], x[1])):
            _same(host(a), b, f"disney {lobe} sample_eval_pdf {nm}")
    # the loops' slow_eval on the same materials (a2 == 1, ratio_to_one_minus of the in-kernel sampler's numbers)
    ref = od.integrate(2, 31)
    got = _with_group(1, lambda: ds.integrate(2, 31))
    for key in ref:
        _same(host(got[key]), ref[key], f"disney integrate {key}")
    # uniform parameters: one small launch per value
    n = 256
    geo = {kk: d[kk][..., :n].copy() for kk in ("wo", "N", "T")}
    ordinary = {name: 0.1 + 0.07 * j for j, name in enumerate(oracle.DISNEY_SCALARS)}
    xs = np.ascontiguousarray(x[:, :n])
    wis = np.ascontiguousarray(wi[R.RLS_RAY_GLOSSY][:, :n])
    for key, vals in (("roughness", rough), ("clearcoat", coat), ("anisotropic", ANISO)):
        for v in vals:
            p = dict(ordinary, **{key: float(F(v))})
            if key == "roughness":
                p["anisotropic"] = 0.0
            cu = dict(geo, base_color=(0.8, 0.6, 0.3), **p)
            cr = dict(geo, base_color=(0.8, 0.6, 0.3), **{kk: np.full(n, vv, np.float32) for kk, vv in p.items()})
            ou, du = disney_oracle(oracle, cr), disney_sampler(gpu, cu)
            du.setSampleType(R.RLS_RAY_GLOSSY)
            what = f"uniform {key} = {v!r}"
            _same(host(du.evalBrdf(dev(wis))), ou.eval(R.RLS_RAY_GLOSSY, wis), f"{what} eval")
            _same(host(du.evalPdf(dev(wis))), ou.pdf(R.RLS_RAY_GLOSSY, wis), f"{what} pdf")
            for nm, a, b in zip(("wi", "f", "pdf"), du.sampleEvalPdf(dev(xs[0]), dev(xs[1])),
                                ou.sample_eval_pdf(R.RLS_RAY_GLOSSY, xs[0], xs[1])):
                _same(host(a), b, f"{what} sample_eval_pdf {nm}")


def test_light_cone_at_extreme_distances(gpu, oracle):
    """cone_make's R_RCPW(sqrtf(dist^2)): shading positions whose squared distance to the light underflows to 0, is subnormal,
    or overflows"""
    n = 1 << 10
    c = cases.ggx_mixed(cases.SEED_EDGE, n)
    k = np.arange(n)
    m = (k % 3) == 0
    e = np.asarray(SCALES)[(k[m] // 3) % len(SCALES)]
    center = np.zeros(3, np.float32)                             # at the origin: |P - center|^2 is |P|^2, whatever its magnitude
    P = (c["N"] * F(3.0)).astype(np.float32)
    P[:, m] = (c["N"][:, m] * np.ldexp(F(1.0), e)[None, :]).astype(np.float32)
    lo = [oracle.make_light(center=tuple(center), radius=1.0, radiance=(2.0, 1.5, 1.0))]
    lg = [R._capi.SphereLight.from_buffer_copy(bytes(l)) for l in lo]
    kw = dict(Kd=0.5, Ks=0.5)
    ref = ggx_oracle(oracle, c).direct_lighting(P, lo, 2, 9, Kd_color=(0.8, 0.7, 0.6), Kd_roughness=0.3, **kw)
    got = _with_group(1, lambda: ggx_sampler(gpu, c).directLighting(dev(P), lg, 2, 9, KdColor=(0.8, 0.7, 0.6),
                                                                    diffuseRoughness=0.3, **kw))
    for nm, a, b in zip(("diffuse", "specular"), got, ref):
        _same(host(a), b, f"light cone {nm}")
