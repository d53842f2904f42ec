"""GPU: the caller-traced integrators (include/rlshaders_amd_trace.h) at production sizes and at their edges, for all four
emitters (rlGgx glossy and refraction, rlDisney diffuse and glossy):

  A. batches beyond one scan batch (n > kScanTile^2 = 2^22 points: trace_scan_totals_kernel's carry between batches)
     against a host int64 scan of chunked emits, the chunks' queues, the integrators and the oracle;
  B. every spp_n against the oracle (non-power-of-two compaction tiles, a partial last tile), and every lane-group width
     with the same bits;
  C. FAST mode against the EXACT oracle queue, by (point, sample);
  D. first_index beyond 2^32, hostile closure inputs, non-finite radiance, a float64 bound on the resolve;
  E. a queue of more than 2^31 rays (the int64 CSR offsets), when the device has the memory.

"Oracle" is the queue composed on the CPU per sample (tests/trace_util.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cases
import oracle_lib as O
from trace_util import DIFFUSE, GLOSSY, disney_inputs, disney_oracle_queue, ggx_inputs, ggx_oracle_queue, radiance, \
    sequential

pytestmark = pytest.mark.gpu

SEED = 4242
EMITTERS = ["ggx_glossy", "ggx_refract", "disney_diffuse", "disney_glossy"]
SCAN_BATCH = 2048 * 2048              # points per batch of trace_scan_totals_kernel (kScanTile tiles of kScanTile points)
CHUNK = 1 << 21                       # the reference chunks of part A: one scan batch each
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-38, 3e38, -3e38, 1e20, -1e20, 2.0, -1.0],
                   dtype=np.float32)  # test_gpu_hostile_inputs.py


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


def _dev_same(a, b, what):
    """the same bits, compared on the device"""
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), what


def _same(got, ref, what):
    """test_gpu_hostile_inputs.py: the same NaN pattern, the same bits everywhere else"""
    got, ref = np.asarray(got), np.asarray(ref)
    nan_g, nan_r = np.isnan(got), np.isnan(ref)
    assert np.array_equal(nan_g, nan_r), (what, "NaN pattern", int((nan_g != nan_r).sum()))
    ok = ~nan_r
    same = got.view(np.uint32)[ok] == ref.view(np.uint32)[ok]
    assert same.all(), (what, int((~same).sum()), "of", int(ok.sum()), got[ok][~same][:4], ref[ok][~same][:4])


def _poison(a, rng, frac=0.02):
    a = a.copy()
    flat = a.reshape(-1)
    k = rng.choice(flat.size, max(1, int(frac * flat.size)), replace=False)
    flat[k] = SPECIAL[rng.integers(0, SPECIAL.size, k.size)]
    return a


def _with_group(g, fn):
    os.environ["RLS_INTEGRATE_GROUP"] = str(g)
    try:
        return fn()
    finally:
        del os.environ["RLS_INTEGRATE_GROUP"]


def _tile_points(spp):
    return min(256, 4096 // spp)      # trace_compact_kernel's points per tile


# ---- the four emitters behind one interface ----------------------------------------------------------------------------------
def _ggx(e):
    return e.startswith("ggx")


def _refract(e):
    return e == "ggx_refract"


def _lobe(e):
    return DIFFUSE if e == "disney_diffuse" else GLOSSY


def _inputs(e, n):
    """host inputs whose per-point ray counts vary down to 0: rlGgx "edge" (black Ks, TIR, grazing views), rlDisney mixed
    with every third point metallic (no diffuse lobe) -> (case, exiting or None)"""
    if _ggx(e):
        case, ex, _ = ggx_inputs("edge", n)
        return case, ex
    case, _ = disney_inputs("metallic_mix", n)
    return case, None


def _mixed(e, n):
    if _ggx(e):
        case, ex, _ = ggx_inputs("mixed", n)
        return case, ex
    case, _ = disney_inputs("mixed", n)
    return case, None


def _sampler(ctx, e, case, ex=None):
    import rlshaders_amd as R
    d = {k: _dev(v) for k, v in case.items()}
    if _ggx(e):
        return R.GgxSampler(ctx, d["wo"], d["N"], d["T"], specColor=d["KsColor"], ior=d["ior"], roughness=d["roughness"],
                            anisotropic=d["anisotropic"], exiting=None if ex is None else _dev(ex))
    sc = {k: d[k] for k in R._capi.DISNEY_SCALARS if k in d}
    return R.DisneySampler(ctx, d["wo"], d["N"], d["T"], base_color=d.get("base_color", (1.0, 1.0, 1.0)), **sc)


def _emit(e, s, spp_n, first=0):
    T = _trace()
    if e == "ggx_glossy":
        return T.glossy_rays(s, spp_n, SEED, first)
    if e == "ggx_refract":
        return T.refract_rays(s, spp_n, SEED, first)
    return T.disney_rays(s, _lobe(e), spp_n, SEED, first)


def _integrate(e, s, spp_n):
    """the integrator the radiance-1 resolve is: (sum or result [3, n], side output [n])"""
    if e == "ggx_glossy":
        return s.integrate(spp_n, SEED)
    if e == "ggx_refract":
        return s.integrateRefract(spp_n, SEED, traced=True, env=(1.0, 1.0, 1.0), want_tir=True)
    ref = s.integrate(spp_n, SEED)
    return (ref["diffuse_sum"], ref["diffuse_count"]) if _lobe(e) == DIFFUSE else (ref["specular_sum"], ref["specular_count"])


def _oracle(e, case, ex, spp_n, first=0):
    if _ggx(e):
        return ggx_oracle_queue(case, ex, spp_n, SEED, _refract(e), first)
    return disney_oracle_queue(case, spp_n, SEED, _lobe(e), first)


def _ones(ctx, q):
    return torch.ones(3, max(q.count, 1), dtype=torch.float32, device=ctx.torch_device)


def _queue_host(q, a=0, b=None):
    """the rays of points [a, b) on the host; offsets and point relative to point a"""
    b = q.n if b is None else b
    off = _host(q.offsets[a:b + 1])
    lo, hi = int(off[0]), int(off[-1])
    h = dict(offsets=off - lo, dir=_host(q._dir[:, lo:hi]), weight=_host(q._weight[:, lo:hi]),
             point=_host(q._point[lo:hi]).astype(np.int64) - a, sample=_host(q._sample[lo:hi]).astype(np.int64))
    if q._kind is not None:
        h["kind"] = _host(q._kind[lo:hi]).astype(np.int64)
    return h


def _assert_matches_oracle(e, h, want, what):
    """offsets, point, sample (and kind) exactly; dir and weight tight"""
    np.testing.assert_array_equal(h["offsets"], want["offsets"], str(what))
    np.testing.assert_array_equal(h["point"], want["point"], str(what))
    np.testing.assert_array_equal(h["sample"], want["sample"], str(what))
    if _refract(e):
        np.testing.assert_array_equal(h["kind"], want["kind"], str(what))
    if len(want["point"]) == 0:
        return
    cases.assert_tight(cases.summarize(cases.rel_err(h["dir"], want["dir"])), (what, "dir"))
    w, ww = (h["weight"][0], want["weight"][0]) if _refract(e) else (h["weight"], want["weight"])
    cases.assert_tight(cases.summarize(cases.rel_err(w, ww)), (what, "weight"))


# ---- A. beyond one scan batch ------------------------------------------------------------------------------------------------
def _device_inputs(ctx, e, n):
    """device-generated inputs (rls_gen_frame / rls_gen_uniform, bit-exact to the oracle's generators) with per-point ray
    counts that vary over 0..spp: rlGgx with cases.ggx_edge's regimes by index mod 8, rlDisney mixed with every third
    point metallic -> (dict of device planes, exiting or None)"""
    import rlshaders_amd as R
    seed = cases.SEED_EDGE
    wo, N, T = R.gen_frame(ctx, seed, 0, n)
    u = lambda stream, lo=0.0, hi=1.0: R.gen_uniform(ctx, seed, 0, n, stream, lo, hi)
    i = torch.arange(n, device=wo.device)
    if _ggx(e):
        k = i % 8
        ct = 0.02 + 0.08 * u(40)                                     # 0: grazing views
        graz = torch.sqrt(1.0 - ct * ct) * T + ct * N
        graz = graz / torch.linalg.vector_norm(graz, dim=0)
        wo = torch.where(k == 0, graz, wo)
        wo = torch.where(k == 1, N, wo)                              # 1: normal incidence
        rough = u(O.S_ROUGH, 0.05, 1.0)
        rough = torch.where(k == 2, 0.0, torch.where(k == 3, 0.005, rough))   # roughness floors
        ior = u(O.S_IOR, 1.05, 2.55)
        ior = torch.where(k == 4, 0.3 + 0.6 * u(42), torch.where(k == 5, 1.0, ior))   # ior < 1 (TIR), ior == 1
        aniso = torch.where(k == 6, 1.0, R.gen_aniso(ctx, seed, 0, n))
        Ks = torch.stack([u(O.S_KS_R + j) for j in range(3)])
        Ks = torch.where(k == 7, 5e-5, Ks)                           # black: every sample dropped
        case = dict(wo=wo, N=N, T=T, KsColor=Ks, roughness=rough, ior=ior, anisotropic=aniso)
        return {k_: v.contiguous() for k_, v in case.items()}, (i % 5 == 3).to(torch.uint8)
    case = dict(wo=wo, N=N, T=T, base_color=torch.stack([u(O.S_KS_R + j) for j in range(3)]))
    for j, name in enumerate(O.DISNEY_SCALARS):
        case[name] = u(O.S_PARAM0 + j)
    case["metallic"] = torch.where(i % 3 == 1, 1.0, case["metallic"])
    return {k_: v.contiguous() for k_, v in case.items()}, None


def _dslice(case, ex, a, b):
    return {k: v[..., a:b].contiguous() for k, v in case.items()}, None if ex is None else ex[a:b].contiguous()


def _windows(n, w=64):
    """starts of the oracle windows: across scan-tile boundaries (multiples of 2048), a chunk boundary, the 2^22 batch
    boundary, past it, and the last point"""
    starts = [0, 2048 - 32, 5 * 2048 - 1, CHUNK - 32, SCAN_BATCH - 32, SCAN_BATCH - 1, SCAN_BATCH + 3 * 2048 - 32, n - w]
    return sorted({min(max(a, 0), n - w) for a in starts})


@pytest.mark.parametrize("e", EMITTERS)
@pytest.mark.parametrize("n", [SCAN_BATCH, SCAN_BATCH + 1, SCAN_BATCH + 2047, 3 * SCAN_BATCH + 12345],
                         ids=["one_batch", "one_tile_more", "ragged_batch", "three_batches"])
def test_beyond_one_scan_batch(ctx, e, n):
    spp_n = 2
    case, ex = _device_inputs(ctx, e, n)
    s = _sampler(ctx, e, case, ex)
    q = _emit(e, s, spp_n)
    # the scan: a host int64 cumsum of the per-point counts of chunks that are one scan batch each
    counts, chunks = [], []
    for a in range(0, n, CHUNK):
        b = min(a + CHUNK, n)
        ca, xa = _dslice(case, ex, a, b)
        qa = _emit(e, _sampler(ctx, e, ca, xa), spp_n, first=a)
        counts.append(np.diff(_host(qa.offsets)))
        chunks.append((a, b, qa))
    counts = np.concatenate(counts)
    assert len(np.unique(counts)) >= 2 and counts.min() == 0, np.unique(counts)      # the counts vary, down to 0
    want = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
    off = _host(q.offsets)
    np.testing.assert_array_equal(off, want)
    assert q.count == want[-1]
    # each chunk's rays are the batch's rays over the chunk's range
    for a, b, qa in chunks:
        lo, hi = int(off[a]), int(off[b])
        assert qa.count == hi - lo, (a, b)
        _dev_same(q.dir[:, lo:hi], qa.dir, (a, "dir"))
        _dev_same(q.weight[:, lo:hi], qa.weight, (a, "weight"))
        assert torch.equal(q.point[lo:hi] - a, qa.point), (a, "point")
        assert torch.equal(q.sample[lo:hi], qa.sample), (a, "sample")
        if _refract(e):
            assert torch.equal(q.kind[lo:hi], qa.kind), (a, "kind")
        _dev_same(q.side[a:b], qa.side, (a, "side"))
    del chunks
    # radiance 1: the integrator, bit for bit, on the device
    ref_sum, ref_side = _integrate(e, s, spp_n)
    _dev_same(q.resolve(_ones(ctx, q)), ref_sum, "radiance-1 resolve vs the integrator")
    _dev_same(q.side, ref_side, "side output vs the integrator")
    # the oracle on windows of 64 points
    for a in _windows(n):
        b = a + 64
        ca, xa = _dslice(case, ex, a, b)
        hc = {k: _host(v) for k, v in ca.items()}
        want_q = _oracle(e, hc, None if xa is None else _host(xa), spp_n, first=a)
        _assert_matches_oracle(e, _queue_host(q, a, b), want_q, (e, n, a))


# ---- B. every spp_n, every lane-group width -------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", EMITTERS)
def test_every_spp_n_against_the_oracle(ctx, e):
    for spp_n in range(1, 17):
        n = 3 * _tile_points(spp_n * spp_n) + 7       # a partial last compaction tile, a ragged last workgroup
        case, ex = _inputs(e, n)
        q = _emit(e, _sampler(ctx, e, case, ex), spp_n)
        _assert_matches_oracle(e, _queue_host(q), _oracle(e, case, ex, spp_n), (e, spp_n))


@pytest.mark.parametrize("e", EMITTERS)
@pytest.mark.parametrize("spp_n", [1, 3, 5, 8, 11, 16])
def test_every_group_width_gives_the_same_bits(ctx, e, spp_n):
    """RLS_INTEGRATE_GROUP forces G = 1, 4, 16, 64 lanes per point, G > spp included (only the override selects it)"""
    n = 3 * _tile_points(spp_n * spp_n) + 7
    case, ex = _inputs(e, n)
    s = _sampler(ctx, e, case, ex)

    def run():
        q = _emit(e, s, spp_n)
        h = _queue_host(q)
        h["side"] = _host(q.side)
        h["resolve"] = _host(q.resolve(_ones(ctx, q)))
        return h

    base = run()                                        # the automatic choice
    for g in (1, 4, 16, 64):
        h = _with_group(g, run)
        for k in ("offsets", "point", "sample", "kind"):
            if k in base:
                np.testing.assert_array_equal(h[k], base[k], str((g, k)))
        for k in ("dir", "weight", "side", "resolve"):
            cases.assert_same_bits(h[k], base[k], (e, spp_n, g, k))


# ---- C. FAST mode against the EXACT oracle ----------------------------------------------------------------------------------------
def _fast_gate(got, ref, what):
    """test_gpu_fast_mode.py::test_disney's per-output gates"""
    st = cases.summarize(cases.rel_err(got, ref))
    print("fast trace", what, st)
    assert st["nonfinite"] == 0 and st["median"] <= 3e-6 and st["frac_gt_1e5"] <= 6e-2, (what, st)
    assert st["p99"] <= 1e-4, (what, st)


@pytest.mark.parametrize("e", EMITTERS)
@pytest.mark.parametrize("spp_n", [4, 7])
def test_fast_queue_against_the_exact_oracle(ctx, e, spp_n):
    n, spp = 1 << 14, spp_n * spp_n
    case, ex = _mixed(e, n)
    want = _oracle(e, case, ex, spp_n)
    ko = want["point"] * 256 + want["sample"]
    s = _sampler(ctx, e, case, ex)
    ctx.set_math_mode(True)
    try:
        for g in (None, 1):
            q = _emit(e, s, spp_n) if g is None else _with_group(g, lambda: _emit(e, s, spp_n))
            h = _queue_host(q)
            kf = h["point"] * 256 + h["sample"]
            common, i_f, i_o = np.intersect1d(kf, ko, assume_unique=True, return_indices=True)
            kept_diff = len(kf) + len(ko) - 2 * len(common)
            assert kept_diff <= 1e-3 * n * spp, (e, spp_n, g, "kept sets differ on", kept_diff, "of", n * spp)
            if _refract(e):
                flips = int((h["kind"][i_f] != want["kind"][i_o]).sum())
                assert flips <= 1e-3 * len(common), (e, spp_n, g, "kind differs on", flips, "of", len(common))
            _fast_gate(h["dir"][:, i_f], want["dir"][:, i_o], (e, spp_n, g, "dir"))
            w, ww = h["weight"][:, i_f], want["weight"][:, i_o]
            _fast_gate(w[0] if _refract(e) else w, ww[0] if _refract(e) else ww, (e, spp_n, g, "weight"))
    finally:
        ctx.set_math_mode(False)


# ---- D. index and input edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", EMITTERS)
@pytest.mark.parametrize("first", [(1 << 32) - 40, (1 << 33) + 17], ids=["straddles_2^32", "beyond_2^33"])
def test_first_index_beyond_32_bits(ctx, e, first):
    n, spp_n = 100, 3
    case, ex = _inputs(e, n)
    q = _emit(e, _sampler(ctx, e, case, ex), spp_n, first=first)
    _assert_matches_oracle(e, _queue_host(q), _oracle(e, case, ex, spp_n, first=first), (e, first))
    # ... and the high word of the index matters: another one draws other samples
    q0 = _emit(e, _sampler(ctx, e, case, ex), spp_n, first=first ^ (1 << 34))
    assert not (q.count == q0.count and np.array_equal(_host(q.dir), _host(q0.dir))), (e, first)


@pytest.mark.parametrize("e", EMITTERS)
def test_hostile_closure_inputs(ctx, e):
    n, spp_n = 1 << 12, 3
    rng = np.random.default_rng(16 + EMITTERS.index(e))
    if _ggx(e):
        case, ex = cases.ggx_mixed(cases.SEED_EDGE, n), None
        keys = ("wo", "N", "T", "roughness", "ior", "anisotropic", "KsColor")
    else:
        case, ex = cases.disney_mixed(cases.SEED_EDGE, n), None
        keys = ("wo", "N", "T", "base_color", "roughness", "metallic", "anisotropic", "clearcoat", "clearcoat_gloss",
                "sheen_tint", "subsurface")
    for k in keys:
        case[k] = _poison(case[k], rng)
    s = _sampler(ctx, e, case, ex)
    q = _emit(e, s, spp_n)
    ref_sum, ref_side = _integrate(e, s, spp_n)
    got = _host(q.resolve(_ones(ctx, q)))
    assert np.isnan(got).any(), "the poison reaches the sums"
    _same(got, _host(ref_sum), (e, "radiance-1 resolve vs the integrator"))
    _same(_host(q.side), _host(ref_side), (e, "side output vs the integrator"))
    h, want = _queue_host(q), _oracle(e, case, ex, spp_n)
    for k in ("offsets", "point", "sample") + (("kind",) if _refract(e) else ()):
        np.testing.assert_array_equal(h[k], want[k], k)               # NaN weights are kept on both sides
    _same(h["dir"], want["dir"], (e, "dir"))
    _same(h["weight"], want["weight"], (e, "weight"))


@pytest.mark.parametrize("e", EMITTERS)
def test_non_finite_radiance(ctx, e):
    """a NaN / Inf radiance reaches exactly the points whose rays carry it: every other point has the bits of the clean
    resolve, points without rays stay +0 (the header: a non-finite radiance cannot come from a dropped ray)"""
    n, spp_n = 1024, 3
    case, ex = _inputs(e, n)
    q = _emit(e, _sampler(ctx, e, case, ex), spp_n)
    h = _queue_host(q)
    cnt, off = len(h["point"]), h["offsets"]
    inv = np.float32(1.0) / np.float32(spp_n * spp_n) if _refract(e) else None
    L = np.full((3, q.capacity), np.nan, np.float32)                 # past the rays: NaN that no point may read
    L[:, :cnt] = radiance(h["dir"], np.arange(cnt))
    clean = _host(q.resolve(_dev(L)))
    rng = np.random.default_rng(21)
    hit = rng.choice(cnt, max(3, cnt // 50), replace=False)
    L[rng.integers(0, 3, hit.size), hit] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(hit.size) % 3]
    got = _host(q.resolve(_dev(L)))
    _same(got, sequential(L[:, :cnt], h["weight"], off, inv), (e, "resolve vs host float32 sequential sum"))
    dirty = np.zeros(n, bool)
    dirty[h["point"][~np.isfinite(L[:, :cnt]).all(axis=0)]] = True
    assert dirty.any() and not dirty.all()
    assert np.array_equal(got[:, ~dirty].view(np.uint32), clean[:, ~dirty].view(np.uint32)), e
    empty = np.diff(off) == 0
    if e in ("ggx_glossy", "disney_diffuse"):
        assert empty.any(), (e, "no point without rays")                 # black Ks / metallic = 1
    assert np.all(got[:, empty].view(np.uint32) == 0), (e, "points without rays are +0")


@pytest.mark.parametrize("e", EMITTERS)
def test_resolve_within_a_float64_bound(ctx, e):
    """|resolve - sum_f64 L w| <= k 2^-24 sum_f64 |L w| per point and channel, k the point's ray count (one rounding per
    product and per addition); refraction one more for the 1/spp scale"""
    n, spp_n = 1 << 12, 4
    case, ex = _mixed(e, n)
    q = _emit(e, _sampler(ctx, e, case, ex), spp_n)
    h = _queue_host(q)
    cnt = len(h["point"])
    L = radiance(h["dir"], np.arange(cnt))
    got = _host(q.resolve(_dev(L))).astype(np.float64)
    w = h["weight"].astype(np.float64)
    prod = L.astype(np.float64) * w
    exact = np.stack([np.bincount(h["point"], weights=prod[c], minlength=n) for c in range(3)])
    mag = np.stack([np.bincount(h["point"], weights=np.abs(prod[c]), minlength=n) for c in range(3)])
    k = np.diff(h["offsets"]).astype(np.float64)
    if _refract(e):
        scale = np.float64(np.float32(1.0) / np.float32(spp_n * spp_n))
        exact, mag, k = exact * scale, mag * scale, k + 1
    err = np.abs(got - exact)
    bound = k * 2.0 ** -24 * mag + 1e-30
    assert np.all(err <= bound), (e, "worst ratio", float((err / bound).max()))


# ---- E. more than 2^31 rays ----------------------------------------------------------------------------------------------------
def test_more_than_2_31_rays(ctx):
    """rlGgx refraction at spp_n = 16 over enough points that the queue holds more than 2^31 rays (point, sample and kind
    left NULL): the int64 offsets, a window around ray 2^31 against a small emit, the radiance-1 resolve against
    rls_ggx_integrate_refract.  Skips unless the device has 1.25x the memory free."""
    import rlshaders_amd as R
    T = _trace()
    lib = T.load()
    spp_n, spp = 16, 256

    def sampler(n, first=0):
        wo, N, Tg = R.gen_frame(ctx, 77, first, n)
        return R.GgxSampler(ctx, wo, N, Tg, specColor=(1.0, 1.0, 1.0), ior=1.5, roughness=0.4, anisotropic=0.0)

    m = 1 << 16
    rate = T.refract_rays(sampler(m), spp_n, SEED).count / (m * spp)     # the keep rate of these inputs
    assert rate > 0.5, rate
    n = int(np.ceil(1.06 * 2 ** 31 / (spp * rate)))
    cap = n * spp
    need = T.scratch_bytes(n, spp_n) + cap * 16 + n * (8 + 4 + 36 + 16 + 4)   # staging, queue, offsets, side, inputs, refs
    free = ctx.device_info()["hbm_free"]
    if free < 1.25 * need:
        pytest.skip(f"needs 1.25 x {need / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} GiB ({free} B) free")
    dev = ctx.torch_device
    s = sampler(n)
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    dirs = torch.empty(3, cap, dtype=torch.float32, device=dev)
    w = torch.empty(cap, dtype=torch.float32, device=dev)
    tir = torch.empty(n, dtype=torch.float32, device=dev)
    scratch = torch.empty(T.scratch_bytes(n, spp_n), dtype=torch.uint8, device=dev)
    d = ones = out = ref = ref_tir = small = None
    try:
        q = T.RayQueue_()
        q.capacity, q.offsets = cap, offsets.data_ptr()
        q.dir = T.capi.Vec3(*[dirs[k].data_ptr() for k in range(3)])
        q.weight = T.capi.Rgb(w.data_ptr(), None, None)
        q.point = q.sample = q.kind = None
        q.scratch, q.scratch_bytes = scratch.data_ptr(), scratch.numel()
        T.check(lib.rls_trace_ggx_refract_emit(ctx.handle, n, C.byref(s.c), spp_n, SEED, 0, C.byref(q), tir.data_ptr()))
        ctx.synchronize()
        scratch = None                                             # the staging: not needed by the resolve
        count = int(offsets[n].item())
        assert count > 2 ** 31, (n, rate, count)
        d = offsets.diff()
        assert int(offsets[0].item()) == 0 and bool((d >= 0).all()) and bool((d <= spp).all())
        # a window of 200 points around the one whose rays cross index 2^31, against a small emit of it
        j = int(torch.searchsorted(offsets, torch.tensor([2 ** 31], dtype=torch.int64, device=dev), right=True).item()) - 1
        assert int(offsets[j].item()) <= 2 ** 31 < int(offsets[j + 1].item())
        a, b = j - 100, j + 100
        small = T.refract_rays(sampler(b - a, first=a), spp_n, SEED, first_index=a)
        assert torch.equal(small.offsets, offsets[a:b + 1] - offsets[a])
        lo, hi = int(offsets[a].item()), int(offsets[b].item())
        assert lo < 2 ** 31 < hi and small.count == hi - lo
        _dev_same(dirs[:, lo:hi], small.dir, "dir around ray 2^31")
        _dev_same(w[lo:hi], small.weight[0], "weight around ray 2^31")
        _dev_same(tir[a:b], small.tir_fraction, "tir_fraction around ray 2^31")
        # radiance 1 (one plane of ones as r, g and b): rls_ggx_integrate_refract(traced = 1, env = 1)
        ones = torch.ones(count, dtype=torch.float32, device=dev)
        out = ctx.empty(3, n)
        T.check(lib.rls_trace_ggx_refract_resolve(ctx.handle, n, C.byref(q), spp_n, T.capi.CRgb(*[ones.data_ptr()] * 3),
                                                  T.capi.Rgb(out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())))
        ones = None
        ref, ref_tir = s.integrateRefract(spp_n, SEED, traced=True, env=(1.0, 1.0, 1.0), want_tir=True)
        _dev_same(out, ref, "radiance-1 resolve vs rls_ggx_integrate_refract")
        _dev_same(tir, ref_tir, "tir_fraction vs rls_ggx_integrate_refract")
        print("more than 2^31 rays:", dict(n=n, keep_rate=rate, rays=count, need_bytes=need, free_bytes=free))
    finally:
        # None, not del: a failing test's traceback keeps this frame, and with it whatever its names still hold
        offsets = dirs = w = tir = scratch = s = d = ones = out = ref = ref_tir = small = None
        torch.cuda.empty_cache()
