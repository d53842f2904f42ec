"""GPU: the caller-traced rlSss integrator (rls_trace_sss_probe_emit / rls_trace_sss_scatter_resolve,
rlshaders_amd.trace.sss_probe_rays / ProbeQueue.resolve).

The emit queues integrateScatter's probe rays (getProbeRay, src/rlSss.h:224-228) densely, point-major; the caller walks them
through the object and reports hits; the resolve combines the hits as the integrator does (src/rlSss.h:245-279).  Checked
here: the queue against the oracle's probe rays on the integrator's samples and against rls_sss_probe_ray; with the probe
rays traced on the host through the analytic scene (orc_scene_trace) and the analytic light's irradiance, the resolve IS
rls_sss_integrate_scatter's result and mean_depth, bit for bit; hit lists no analytic scene makes, against a host composition
of the oracle's profile, fade and MIS pdf; large batches, first_index past 2^32, graph capture, FAST mode."""
import numpy as np
import pytest
import torch

import cases
import oracle_lib as O
from trace_sss_util import (MAX_HITS, host_resolve, light_irradiance, plane_case, same_bits_or_both_nan, sphere_case,
                            trace_plane_np, trace_queue)

pytestmark = pytest.mark.gpu

SEED = 4242


@pytest.fixture(scope="module")
def ctx():
    import rlshaders_amd as R
    from rlshaders_amd import build
    build.build_trace_library()
    c = R.Context(0)
    yield c
    c.close()


def _trace():
    from rlshaders_amd import trace
    return trace


def _host(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if isinstance(a, np.ndarray) else a


def _sampler(ctx, case, has_dPdu=True, materials=None):
    import rlshaders_amd as R
    if materials is not None:
        ids, cols = materials
        return R.SssSampler(ctx, _dev(case["N"]), _dev(case["T"]), _dev(cols["albedo"]), _dev(cols["dist"]),
                            has_dPdu=has_dPdu, materials=(_dev(ids), cols["albedo"].shape[1]))
    return R.SssSampler(ctx, _dev(case["N"]), _dev(case["T"]), _dev(case["albedo"]), _dev(case["dist"]), has_dPdu=has_dPdu)


def _scene_pair(**kw):
    import rlshaders_amd as R
    so = O.make_scene(**kw)
    return so, R._capi.SssScene.from_buffer_copy(bytes(so))


SPHERE = dict(geometry="sphere", sphere_center=(0.3, -0.2, 0.1), sphere_radius=0.35, light_dir=(0.0, 0.6, 0.8),
              light_color=(1.5, 1.0, 0.25))


def _setting(kind, n):
    """(case, scene kwargs, has_dPdu) of one analytic setting"""
    if kind.startswith("plane"):
        case, nrm = plane_case(n)
        kw = dict(geometry="plane", plane_point=(0.5, -1.0, 0.25), plane_normal=tuple(nrm), light_dir=tuple(nrm),
                  light_color=(1.0, 0.5, 2.0))
        if kind == "plane_gate":
            kw.update(gate_point=(0.5, -1.0, 0.25), gate_normal=(1.0, 0.0, 0.0))
        return case, kw, True
    case = sphere_case(n, bend=0.3 if kind == "sphere_bent" else 0.0)
    kw = dict(SPHERE)
    if kind == "sphere_gate":
        kw.update(gate_point=(0.3, -0.2, 0.1), gate_normal=(0.0, 0.0, 1.0))
    return case, kw, kind != "sphere_polar"


def _traced_hits(scene, q):
    """the queue traced on the host through the analytic scene -> device tensors (count, P, N, E)"""
    cnt, hP, hN = trace_queue(scene, _host(q.origin), _host(q.dir), _host(q.maxdist))
    E = light_irradiance(scene, hP, hN)
    return _dev(cnt), _dev(hP), _dev(hN), _dev(E)


# ---- 1. the queue -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,spp_n", [("sphere", 4), ("sphere_polar", 3), ("plane", 2), ("sphere_bent", 5)])
def test_emit_matches_the_oracle_and_the_probe_call(ctx, kind, spp_n):
    T = _trace()
    n, spp, first = 777, spp_n * spp_n, 12345
    case, _, has_dPdu = _setting(kind, n)
    s = _sampler(ctx, case, has_dPdu)
    q = T.sss_probe_rays(s, _dev(case["P"]), spp_n, SEED, first_index=first)
    assert q.count == n * spp
    np.testing.assert_array_equal(_host(q.offsets), np.arange(n + 1, dtype=np.int64) * spp)
    np.testing.assert_array_equal(_host(q.point), np.repeat(np.arange(n), spp))
    np.testing.assert_array_equal(_host(q.sample), np.tile(np.arange(spp), n))
    origin = _host(q.origin).reshape(3, n, spp)
    dirs = _host(q.dir).reshape(3, n, spp)
    maxdist = _host(q.maxdist).reshape(n, spp)
    o = O.Sss(n, case["dist"], case["albedo"], N=case["N"], T=case["T"], has_dPdu=has_dPdu)
    for smp in range(spp):
        rx, ry = O.batch_sample_02(SEED, first, n, 0, smp)
        ref = o.probe(rx, ry)
        cases.assert_tight(cases.summarize(cases.rel_err(origin[:, :, smp], (case["P"] + ref["origin"]).astype(np.float32))),
                           (kind, smp, "origin"))
        cases.assert_tight(cases.summarize(cases.rel_err(dirs[:, :, smp], ref["dir"])), (kind, smp, "dir"))
        cases.assert_tight(cases.summarize(cases.rel_err(maxdist[:, smp], ref["maxdist"])), (kind, smp, "maxdist"))
        # the device's own getProbeRay on the same (rx, ry) and P: the same bits
        got = s.getProbeRay(_dev(rx), _dev(ry), P=_dev(case["P"]))
        cases.assert_same_bits(origin[:, :, smp], _host(got["origin"]), (kind, smp, "origin vs rls_sss_probe_ray"))
        cases.assert_same_bits(dirs[:, :, smp], _host(got["dir"]), (kind, smp, "dir vs rls_sss_probe_ray"))
        cases.assert_same_bits(maxdist[:, smp], _host(got["maxdist"]), (kind, smp, "maxdist vs rls_sss_probe_ray"))


def test_fast_emit_matches_the_fast_probe_call(ctx):
    T = _trace()
    n, spp_n = 1000, 3
    case, _, _ = _setting("sphere", n)
    ctx.set_math_mode(True)
    try:
        s = _sampler(ctx, case)
        q = T.sss_probe_rays(s, _dev(case["P"]), spp_n, SEED)
        for smp in range(spp_n * spp_n):
            rx, ry = O.batch_sample_02(SEED, 0, n, 0, smp)
            got = s.getProbeRay(_dev(rx), _dev(ry), P=_dev(case["P"]))
            for k in ("origin", "dir"):
                cases.assert_same_bits(_host(getattr(q, k)).reshape(3, n, -1)[:, :, smp], _host(got[k]), (smp, k))
            cases.assert_same_bits(_host(q.maxdist).reshape(n, -1)[:, smp], _host(got["maxdist"]), (smp, "maxdist"))
    finally:
        ctx.set_math_mode(False)


# ---- 2. end to end against the integrator -----------------------------------------------------------------------------------
@pytest.mark.parametrize("literal", [False, True], ids=["projection", "literal"])
@pytest.mark.parametrize("cavity", [False, True], ids=["nofade", "fade"])
@pytest.mark.parametrize("kind", ["sphere", "sphere_gate", "sphere_polar", "plane", "plane_gate"])
def test_traced_scene_is_the_integrator_bit_for_bit(ctx, kind, cavity, literal):
    T = _trace()
    n, spp_n = 400, 4
    case, kw, has_dPdu = _setting(kind, n)
    so, sg = _scene_pair(use_cavity_fade=cavity, literal_matrix=literal, **kw)
    s = _sampler(ctx, case, has_dPdu)
    P = _dev(case["P"])
    q = T.sss_probe_rays(s, P, spp_n, SEED)
    cnt, hP, hN, E = _traced_hits(so, q)
    got, dgot = q.resolve(cnt, hP, hN, E, use_cavity_fade=cavity, literal_matrix=literal, want_depth=True)
    ref, dref = s.integrateScatter(P, sg, spp_n, SEED, want_depth=True)
    cases.assert_same_bits(_host(got), _host(ref), (kind, cavity, literal, "result"))
    cases.assert_same_bits(_host(dgot), _host(dref), (kind, cavity, literal, "mean_depth"))
    assert float(_host(dref).mean()) > 0.2
    o = O.Sss(n, case["dist"], case["albedo"], N=case["N"], T=case["T"], has_dPdu=has_dPdu)
    oref, odref = O.integrate_scatter(o, case["P"], so, spp_n, SEED)
    cases.assert_tight(cases.summarize(cases.rel_err(_host(got), oref)), (kind, "vs oracle"))
    np.testing.assert_array_equal(_host(dgot), odref)


@pytest.mark.parametrize("spp_n", list(range(1, 17)))
def test_every_spp_n(ctx, spp_n):
    T = _trace()
    n = 96 if spp_n <= 8 else 24
    case, kw, _ = _setting("sphere", n)
    so, sg = _scene_pair(use_cavity_fade=True, **kw)
    s = _sampler(ctx, case)
    P = _dev(case["P"])
    q = T.sss_probe_rays(s, P, spp_n, SEED, first_index=77)
    cnt, hP, hN, E = _traced_hits(so, q)
    got, dgot = q.resolve(cnt, hP, hN, E, use_cavity_fade=True, want_depth=True)
    ref, dref = s.integrateScatter(P, sg, spp_n, SEED, want_depth=True, first_index=77)
    cases.assert_same_bits(_host(got), _host(ref), (spp_n, "result"))
    cases.assert_same_bits(_host(dgot), _host(dref), (spp_n, "mean_depth"))


def test_parameters_by_reference(ctx):
    T = _trace()
    n, spp_n, m = 500, 3, 7
    case, kw, _ = _setting("sphere", n)
    cols = dict(dist=np.stack([O.gen_uniform(5, 0, m, O.S_PARAM0 + j, 0.02, 0.3) for j in range(3)]),
                albedo=np.stack([O.gen_uniform(5, 0, m, O.S_KS_R + j) for j in range(3)]))
    ids = ((O.gen_uniform(cases.SEED_PARITY, 0, n, 77) * m).astype(np.uint32) % m).astype(np.int32)
    so, sg = _scene_pair(use_cavity_fade=True, **kw)
    s = _sampler(ctx, case, materials=(ids, cols))
    P = _dev(case["P"])
    q = T.sss_probe_rays(s, P, spp_n, SEED)
    cnt, hP, hN, E = _traced_hits(so, q)
    got, dgot = q.resolve(cnt, hP, hN, E, use_cavity_fade=True, want_depth=True)
    ref, dref = s.integrateScatter(P, sg, spp_n, SEED, want_depth=True)
    cases.assert_same_bits(_host(got), _host(ref), "materials: result")
    cases.assert_same_bits(_host(dgot), _host(dref), "materials: mean_depth")


# ---- 3. hit lists no analytic scene produces ---------------------------------------------------------------------------------
def _synthetic_hits(case, spp, max_hits, stride, seed):
    """up to 15 reported hits per ray (counts above max_hits included), scattered around the shading point (some beyond
    maxRadius), duplicates within AI_EPSILON, zero, NaN and Inf irradiance"""
    rng = np.random.default_rng(seed)
    f = np.float32
    n = case["P"].shape[1]
    rays = n * spp
    pt = np.arange(rays) // spp
    cnt = np.zeros(stride, np.uint8)
    cnt[:rays] = rng.integers(0, 16, rays)
    maxR = 3 * case["dist"].max(axis=0)[pt]
    off = rng.normal(size=(3, MAX_HITS, rays)) * (0.6 * maxR)
    hP = np.zeros((3, MAX_HITS, stride), f)
    hP[:, :, :rays] = case["P"][:, None, pt] + off
    dup = rng.random((MAX_HITS, rays)) < 0.15                              # within AI_EPSILON of the hit before
    for k in range(1, MAX_HITS):
        hP[:, k, :rays] = np.where(dup[k], hP[:, k - 1, :rays] + f(3e-5), hP[:, k, :rays])
    hP = hP[:, :max_hits].copy()
    N0 = rng.normal(size=(3, max_hits, stride)).astype(f)
    hN = (N0 / np.linalg.norm(N0, axis=0)).astype(f)
    E = rng.random((3, max_hits, stride)).astype(f) * f(2)
    E[:, rng.random((max_hits, stride)) < 0.1] = 0                          # shaded, counted, no term
    E[0, rng.random((max_hits, stride)) < 0.01] = np.nan
    E[1, rng.random((max_hits, stride)) < 0.01] = np.inf
    return cnt, hP, hN, E


@pytest.mark.parametrize("max_hits", [12, 5, 1])
@pytest.mark.parametrize("cavity,literal", [(False, False), (True, True), (True, False)])
def test_synthetic_hits_against_the_host(ctx, max_hits, cavity, literal):
    T = _trace()
    n, spp_n = 300, 3
    spp = spp_n * spp_n
    case, _, _ = _setting("sphere", n)
    s = _sampler(ctx, case)
    q = T.sss_probe_rays(s, _dev(case["P"]), spp_n, SEED)
    stride = n * spp + 37
    cnt, hP, hN, E = _synthetic_hits(case, spp, max_hits, stride, seed=max_hits * 7 + cavity * 2 + literal)
    got, dgot = q.resolve(_dev(cnt), _dev(hP), _dev(hN), _dev(E), use_cavity_fade=cavity, literal_matrix=literal,
                          want_depth=True)
    want, dwant = host_resolve(case, spp, cnt, hP, hN, E, max_hits, cavity, literal)
    np.testing.assert_array_equal(_host(dgot), dwant)
    g = _host(got)
    if cases.strict_parity():
        same_bits_or_both_nan(g, want, (max_hits, cavity, literal))
    else:
        assert np.array_equal(np.isnan(g), np.isnan(want))
        fin = np.all(np.isfinite(want), axis=0) & np.all(np.isfinite(g), axis=0)
        cases.assert_tight(cases.summarize(cases.rel_err(g[:, fin], want[:, fin])), (max_hits, cavity, literal))
    assert np.isnan(g).any() and np.isinf(g).any()                          # the poisoned hits reached the sums
    assert float(dwant.max()) > (3.0 if max_hits >= 5 else 0.5)        # deep hit lists were walked


def test_a_ray_with_no_hits_and_an_empty_batch(ctx):
    T = _trace()
    n, spp_n = 64, 2
    case, _, _ = _setting("sphere", n)
    s = _sampler(ctx, case)
    q = T.sss_probe_rays(s, _dev(case["P"]), spp_n, SEED)
    rays = n * spp_n * spp_n
    z = torch.zeros(3, 1, rays, dtype=torch.float32, device="cuda")
    got, d = q.resolve(torch.zeros(rays, dtype=torch.uint8, device="cuda"), z, z, z, want_depth=True)
    assert not _host(got).any() and not _host(d).any()
    import rlshaders_amd as R
    e = T.ProbeQueue(ctx, 0, spp_n)
    e.offsets.fill_(-1)
    s0 = R.SssSampler(ctx, torch.zeros(3, 0, device="cuda"), torch.zeros(3, 0, device="cuda"), (1.0, 1.0, 1.0), (0.1, 0.1, 0.1))
    T.sss_probe_rays(s0, torch.zeros(3, 0, device="cuda"), spp_n, SEED, queue=e)
    assert _host(e.offsets).tolist() == [0]


# ---- 4. large batches, first_index past 2^32, graph capture, FAST --------------------------------------------------------------
def test_large_batch_and_first_index_past_2_32(ctx):
    T = _trace()
    n, spp_n, first = (1 << 22) + 4099, 1, (1 << 32) + 5
    case, kw, _ = _setting("plane", n)
    so, sg = _scene_pair(use_cavity_fade=True, **kw)
    s = _sampler(ctx, case)
    P = _dev(case["P"])
    q = T.sss_probe_rays(s, P, spp_n, SEED, first_index=first)
    off = _host(q.offsets)
    assert off[0] == 0 and off[-1] == n and np.array_equal(off[[1, n // 2, n - 1]], [1, n // 2, n - 1])
    origin, dirs, maxdist = _host(q.origin), _host(q.dir), _host(q.maxdist)
    cnt, hP, hN = trace_plane_np(so.plane_point[:], so.plane_normal[:], origin, dirs, maxdist)
    # the vectorised tracer is orc_scene_trace on a sample of the rays
    for j in np.linspace(0, n - 1, 400).astype(np.int64):
        k, _, hp, hn = O.scene_trace(so, origin[:, j], dirs[:, j], maxdist[j])
        assert k == cnt[j] and (k == 0 or (np.array_equal(np.float32(hp[0]), hP[:, 0, j]) and
                                           np.array_equal(np.float32(hn[0]), hN[:, 0, j]))), j
    E = light_irradiance(so, hP, hN)
    got, dgot = q.resolve(_dev(cnt), _dev(hP), _dev(hN), _dev(E), use_cavity_fade=True, want_depth=True)
    ref, dref = s.integrateScatter(P, sg, spp_n, SEED, want_depth=True, first_index=first)
    cases.assert_same_bits(_host(got), _host(ref), "2^22 + 4099 points: result")
    cases.assert_same_bits(_host(dgot), _host(dref), "mean_depth")
    # a window of points against the oracle at the same first_index
    w = slice(n - 300, n)
    cw = {k: np.ascontiguousarray(v[:, w]) for k, v in case.items()}
    o = O.Sss(300, cw["dist"], cw["albedo"], N=cw["N"], T=cw["T"])
    oref, _ = O.integrate_scatter(o, cw["P"], so, spp_n, SEED, first_index=first + n - 300)
    cases.assert_tight(cases.summarize(cases.rel_err(_host(got)[:, w], oref)), "window vs oracle")


def test_emit_and_resolve_in_a_graph(ctx):
    import rlshaders_amd as R
    T = _trace()
    n, spp_n = 3000, 3
    case, kw, _ = _setting("sphere", n)
    so, _ = _scene_pair(use_cavity_fade=True, **kw)
    gctx = R.Context(0, use_torch_stream=False)          # the context's own stream: the NULL stream cannot be captured
    try:
        s = _sampler(gctx, case)
        P = _dev(case["P"])
        torch.cuda.synchronize()
        direct = T.sss_probe_rays(s, P, spp_n, SEED)
        gctx.synchronize()
        cnt, hP, hN, E = _traced_hits(so, direct)
        want, dwant = direct.resolve(cnt, hP, hN, E, use_cavity_fade=True, want_depth=True)
        gctx.synchronize()
        want, dwant = _host(want), _host(dwant)
        q = T.ProbeQueue(gctx, n, spp_n)
        out, depth = gctx.empty(3, n), gctx.empty(n)
        q.sampler, q.P = s, P
        torch.cuda.synchronize()
        with gctx.capture() as g:
            T.sss_probe_rays(s, P, spp_n, SEED, queue=q)
            q.resolve(cnt, hP, hN, E, use_cavity_fade=True, want_depth=True, out=out, depth_out=depth)
        out.zero_()
        depth.zero_()
        q.origin.zero_()
        q.offsets.zero_()
        torch.cuda.synchronize()
        g.launch()
        gctx.synchronize()
        g.close()
        np.testing.assert_array_equal(_host(q.offsets), _host(direct.offsets))
        for k in ("origin", "dir", "maxdist"):
            cases.assert_same_bits(_host(getattr(q, k)), _host(getattr(direct, k)), k)
        cases.assert_same_bits(_host(out), want, "resolve")
        cases.assert_same_bits(_host(depth), dwant, "mean_depth")
    finally:
        gctx.close()


def test_fast_resolve_against_exact(ctx):
    T = _trace()
    n, spp_n = 2000, 4
    case, kw, _ = _setting("sphere", n)
    so, _ = _scene_pair(use_cavity_fade=True, **kw)
    s = _sampler(ctx, case)
    P = _dev(case["P"])
    q = T.sss_probe_rays(s, P, spp_n, SEED)
    cnt, hP, hN, E = _traced_hits(so, q)
    exact, dex = (_host(t) for t in q.resolve(cnt, hP, hN, E, use_cavity_fade=True, want_depth=True))
    ctx.set_math_mode(True)
    try:
        fast, dfa = (_host(t) for t in q.resolve(cnt, hP, hN, E, use_cavity_fade=True, want_depth=True))
    finally:
        ctx.set_math_mode(False)
    st = cases.summarize(cases.rel_err(fast, exact))
    print("sss resolve FAST vs EXACT", st)
    # test_gpu_fast_mode's gates for the probe-ray loop (test_gpu_scatter.py, test_fast_mode_within_roundoff)
    assert st["nonfinite"] == 0 and st["median"] <= 1e-5 and st["p99"] <= 1e-3
    assert (dfa != dex).mean() < 1e-3


# ---- argument checks that need a device ---------------------------------------------------------------------------------------
def test_python_argument_checks(ctx):
    T = _trace()
    n, spp_n = 16, 2
    case, _, _ = _setting("sphere", n)
    s = _sampler(ctx, case)
    q = T.ProbeQueue(ctx, n, spp_n)
    z = torch.zeros(3, 2, n * 4, dtype=torch.float32, device="cuda")
    c = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="no emit"):
        q.resolve(c, z, z, z)
    T.sss_probe_rays(s, _dev(case["P"]), spp_n, SEED, queue=q)
    with pytest.raises(ValueError, match="count"):
        q.resolve(c[:-1], z, z, z)
    with pytest.raises(ValueError, match="P"):
        q.resolve(c, torch.zeros(3, 13, n * 4, device="cuda"), z, z)
    with pytest.raises(ValueError, match="N"):
        q.resolve(c, z, torch.zeros(3, 3, n * 4, device="cuda"), z)
    with pytest.raises(ValueError, match="queue"):
        T.sss_probe_rays(s, _dev(case["P"]), 3, SEED, queue=q)
