"""GPU: the caller-traced rlGgx integrators (include/rlshaders_amd_trace.h, rlshaders_amd/trace.py).

Emit puts every sample ray of integrateGlossy / integrateRefract into a compacted queue; resolve reduces the radiance the
caller traced.  Checked here: with radiance 1 the resolves ARE the existing integrators, bit for bit (the same device
arithmetic, EXACT and FAST); the queue against the oracle composed per sample (orc_sample_02 -> orc_ggx_init ->
orc_ggx_eval_sample / _eval_brdf / _eval_pdf or orc_ggx_refract_sample); a non-constant radiance against float32 sequential
sums; chunking over first_index and the lane-group width; argument checks; graph capture."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
from trace_util import ggx_inputs as _inputs, ggx_oracle_queue as _oracle_queue, radiance as _radiance, \
    sequential as _sequential

pytestmark = pytest.mark.gpu

SEED = 4242
INVALID = 1            # RLS_ERR_INVALID_ARGUMENT


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


def _sampler(ctx, case, exiting=None, materials=None):
    import rlshaders_amd as R
    return R.GgxSampler(ctx, _dev(case["wo"]), _dev(case["N"]), _dev(case["T"]), specColor=_dev(case["KsColor"]),
                        ior=_dev(case["ior"]), roughness=_dev(case["roughness"]), anisotropic=_dev(case["anisotropic"]),
                        exiting=None if exiting is None else torch.from_numpy(exiting).cuda(), materials=materials)


KINDS = ["mixed", "edge", "uniform", "materials"] + [f"preset:{k}" for k in cases.GGX_PRESETS]


# ---- 1. radiance 1: the existing integrators, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("spp_n", [1, 2, 4, 8, 16])
def test_unit_radiance_is_the_integrator_bit_for_bit(ctx, spp_n, fast):
    T = _trace()
    n = 3001 if spp_n <= 8 else 1001
    ctx.set_math_mode(fast)
    try:
        for kind in KINDS:
            case, ex, mat = _inputs(kind, n)
            s = _sampler(ctx, case, ex, mat)
            ref_sum, ref_avg = s.integrate(spp_n, SEED)
            ref_res, ref_tir = s.integrateRefract(spp_n, SEED, traced=True, env=(1.0, 1.0, 1.0), want_tir=True)
            g = T.glossy_rays(s, spp_n, SEED)
            ones = torch.ones(3, max(g.count, 1), dtype=torch.float32, device=ctx.torch_device)
            got = g.resolve(ones)
            cases.assert_same_bits(_host(got), _host(ref_sum), (kind, spp_n, fast, "glossy sum"))
            cases.assert_same_bits(_host(g.avg_reflect_weight), _host(ref_avg), (kind, spp_n, fast, "avg_reflect_weight"))
            r = T.refract_rays(s, spp_n, SEED)
            ones = torch.ones(3, max(r.count, 1), dtype=torch.float32, device=ctx.torch_device)
            cases.assert_same_bits(_host(r.resolve(ones)), _host(ref_res), (kind, spp_n, fast, "refraction result"))
            cases.assert_same_bits(_host(r.tir_fraction), _host(ref_tir), (kind, spp_n, fast, "tir_fraction"))
    finally:
        ctx.set_math_mode(False)


# ---- 2. the queue against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("refract", [False, True], ids=["glossy", "refract"])
@pytest.mark.parametrize("kind,spp_n", [("mixed", 4), ("edge", 3), ("preset:0002_gold", 2)])
def test_queue_matches_the_oracle(ctx, kind, spp_n, refract):
    T = _trace()
    n = 1024
    case, ex, _ = _inputs(kind, n)
    s = _sampler(ctx, case, ex)
    q = (T.refract_rays if refract else T.glossy_rays)(s, spp_n, SEED)
    want = _oracle_queue(case, ex, spp_n, SEED, refract)
    offsets = _host(q.offsets)
    assert offsets[0] == 0 and np.all(np.diff(offsets) >= 0) and np.all(np.diff(offsets) <= spp_n * spp_n)
    np.testing.assert_array_equal(offsets, want["offsets"])          # which samples are kept: zero weights are absent
    cnt = q.count
    assert cnt == want["offsets"][-1]
    np.testing.assert_array_equal(_host(q.point).astype(np.int64), want["point"])       # point-major ...
    np.testing.assert_array_equal(_host(q.sample).astype(np.int64), want["sample"])     # ... samples ascending
    assert np.all(np.diff(want["point"] * 256 + want["sample"]) > 0)
    cases.assert_tight(cases.summarize(cases.rel_err(_host(q.dir), want["dir"])), (kind, "dir"))
    w = _host(q.weight)
    cases.assert_tight(cases.summarize(cases.rel_err(w if not refract else w[0], want["weight"] if not refract else want["weight"][0])),
                       (kind, "weight"))
    assert not np.any(np.all(w == 0.0, axis=0))
    if refract:
        np.testing.assert_array_equal(_host(q.kind).astype(np.int64), want["kind"])
        assert set(np.unique(want["kind"])) <= {T.RLS_RAY_TRANSMITTED, T.RLS_RAY_TIR_MIRROR}


# ---- 3. a radiance that varies -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refract", [False, True], ids=["glossy", "refract"])
def test_varying_radiance(ctx, refract):
    T = _trace()
    n, spp_n = 1024, 4
    case, ex, _ = _inputs("mixed", n)
    s = _sampler(ctx, case, ex)
    q = (T.refract_rays if refract else T.glossy_rays)(s, spp_n, SEED)
    cnt = q.count
    d, w, off = _host(q.dir), _host(q.weight), _host(q.offsets)
    L = _radiance(d, np.arange(cnt))
    got = _host(q.resolve(_dev(L)))
    inv = np.float32(1.0) / np.float32(spp_n * spp_n) if refract else None
    # the resolve arithmetic alone: the same float32 sequence on the host over the emitted weights
    cases.assert_same_bits(got, _sequential(L, w, off, inv), "resolve vs host sequential sum over the emitted queue")
    # end to end against the oracle's weights and directions
    want = _oracle_queue(case, ex, spp_n, SEED, refract)
    Lo = _radiance(want["dir"], np.arange(len(want["point"])))
    cases.assert_tight(cases.summarize(cases.rel_err(got, _sequential(Lo, want["weight"], want["offsets"], inv))),
                       "resolve vs oracle")


# ---- 4. chunks and lane-group widths -------------------------------------------------------------------------------------------
def _slice(case, a, b):
    return {k: (v[..., a:b].copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}


@pytest.mark.parametrize("refract", [False, True], ids=["glossy", "refract"])
def test_chunks_and_group_widths(ctx, refract):
    T = _trace()
    emit = T.refract_rays if refract else T.glossy_rays
    spp_n = 4
    n, cut = 1 << 16, 23457
    case, _, _ = _inputs("mixed", n)
    full = emit(_sampler(ctx, case), spp_n, SEED)
    L = torch.rand(3, full.count, generator=torch.Generator().manual_seed(1)).cuda()
    res_full = _host(full.resolve(L))
    off = _host(full.offsets)
    parts = [(0, cut), (cut, n), (n - 64, n), (100, 117)]           # the last two: a few points, the widest lane groups
    for a, b in parts:
        qa = emit(_sampler(ctx, _slice(case, a, b)), spp_n, SEED, first_index=a)
        oa = _host(qa.offsets)
        np.testing.assert_array_equal(oa, off[a:b + 1] - off[a], (a, b))
        lo, hi = int(off[a]), int(off[b])
        cases.assert_same_bits(_host(qa.dir), _host(full.dir)[:, lo:hi], (a, b, "dir"))
        cases.assert_same_bits(_host(qa.weight), _host(full.weight)[:, lo:hi], (a, b, "weight"))
        np.testing.assert_array_equal(_host(qa.point).astype(np.int64) + a, _host(full.point)[lo:hi])
        np.testing.assert_array_equal(_host(qa.sample), _host(full.sample)[lo:hi])
        cases.assert_same_bits(_host(qa.side), _host(full.side)[a:b], (a, b, "side"))
        cases.assert_same_bits(_host(qa.resolve(L[:, lo:hi].contiguous())), res_full[:, a:b], (a, b, "resolve"))


# ---- 5. argument checks ------------------------------------------------------------------------------------------------------
def test_argument_checks(ctx):
    T = _trace()
    lib = T.load()
    n, spp_n = 256, 2
    case, _, _ = _inputs("mixed", n)
    s = _sampler(ctx, case)
    q = T.RayQueue(ctx, n, spp_n, refract=False)

    def emit(qq, spp=spp_n, nn=n, fn=lib.rls_trace_ggx_glossy_emit, c=C.byref(s.c)):
        return fn(ctx.handle, nn, c, spp, SEED, 0, C.byref(qq), None)

    assert emit(q.q) == 0
    bad = T.RayQueue_.from_buffer_copy(q.q)
    bad.capacity = n * spp_n * spp_n - 1
    assert emit(bad) == INVALID and b"capacity" in O_last_error()
    for spp in (0, 17):
        assert emit(q.q, spp=spp) == INVALID
    for field in ("offsets", "scratch"):
        bad = T.RayQueue_.from_buffer_copy(q.q)
        setattr(bad, field, None)
        assert emit(bad) == INVALID, field
    bad = T.RayQueue_.from_buffer_copy(q.q)
    bad.dir.y = None
    assert emit(bad) == INVALID
    bad = T.RayQueue_.from_buffer_copy(q.q)
    bad.weight.b = None
    assert emit(bad) == INVALID
    assert emit(bad, fn=lib.rls_trace_ggx_refract_emit) == 0          # refraction needs weight.r only
    bad = T.RayQueue_.from_buffer_copy(q.q)
    bad.scratch_bytes = T.scratch_bytes(n, spp_n) - 1
    assert emit(bad) == INVALID
    assert emit(q.q, c=None) == INVALID
    # optional planes
    bad = T.RayQueue_.from_buffer_copy(q.q)
    bad.point, bad.sample, bad.kind = None, None, None
    assert emit(bad) == 0 and emit(bad, fn=lib.rls_trace_ggx_refract_emit) == 0
    # n = 0: an empty queue, offsets[0] = 0
    q0 = T.RayQueue(ctx, 0, spp_n, refract=False)
    q0.offsets.fill_(-1)
    assert emit(q0.q, nn=0, c=None) == 0
    assert q0.count == 0
    assert lib.rls_trace_ggx_glossy_resolve(ctx.handle, 0, C.byref(q0.q), T.capi.CRgb(), T.capi.Rgb()) == 0
    # resolve
    L = torch.ones(3, n * spp_n * spp_n, device=ctx.torch_device)
    out = ctx.empty(3, n)
    Lc = T.capi.CRgb(L[0].data_ptr(), L[1].data_ptr(), L[2].data_ptr())
    oc = T.capi.Rgb(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    assert lib.rls_trace_ggx_glossy_resolve(ctx.handle, n, C.byref(q.q), Lc, oc) == 0
    assert lib.rls_trace_ggx_glossy_resolve(ctx.handle, n, C.byref(q.q), T.capi.CRgb(L[0].data_ptr(), None, None), oc) == INVALID
    assert lib.rls_trace_ggx_glossy_resolve(ctx.handle, n, None, Lc, oc) == INVALID
    assert lib.rls_trace_ggx_refract_resolve(ctx.handle, n, C.byref(q.q), 0, Lc, oc) == INVALID
    assert lib.rls_trace_ggx_refract_resolve(ctx.handle, n, C.byref(q.q), 17, Lc, oc) == INVALID
    with pytest.raises(ValueError):
        q.resolve(torch.ones(3, 1, device=ctx.torch_device))
    b = C.c_size_t()
    assert lib.rls_trace_scratch_bytes(n, 0, C.byref(b)) == INVALID
    assert lib.rls_trace_scratch_bytes(-1, 2, C.byref(b)) == INVALID
    ctx.synchronize()


def O_last_error():
    import rlshaders_amd as R
    return R.load().rls_last_error()


# ---- 6. graph capture --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refract", [False, True], ids=["glossy", "refract"])
def test_emit_and_resolve_in_a_graph(ctx, refract):
    import rlshaders_amd as R
    T = _trace()
    emit = T.refract_rays if refract else T.glossy_rays
    n, spp_n = 5000, 3
    case, ex, _ = _inputs("edge", n)
    gctx = R.Context(0, use_torch_stream=False)          # the context's own stream: the NULL stream cannot be captured
    try:
        s = _sampler(gctx, case, ex)
        torch.cuda.synchronize()
        direct = emit(s, spp_n, SEED)
        gctx.synchronize()
        cnt = direct.count
        L = torch.from_numpy(_radiance(_host(direct.dir), np.arange(cnt))).cuda()
        q = T.RayQueue(gctx, n, spp_n, refract)
        out = gctx.empty(3, n)
        torch.cuda.synchronize()
        want = _host(direct.resolve(L))
        gctx.synchronize()
        with gctx.capture() as g:
            emit(s, spp_n, SEED, queue=q)
            q.resolve(L, out=out, count=cnt)
        # recording runs nothing
        out.zero_()
        q.offsets.zero_()
        torch.cuda.synchronize()
        g.launch()
        gctx.synchronize()
        g.close()
        np.testing.assert_array_equal(_host(q.offsets), _host(direct.offsets))
        cases.assert_same_bits(_host(q.dir), _host(direct.dir), "dir")
        cases.assert_same_bits(_host(q.weight), _host(direct.weight), "weight")
        cases.assert_same_bits(_host(q.side), _host(direct.side), "side")
        cases.assert_same_bits(_host(out), want, "resolve")
    finally:
        gctx.close()
