"""GPU: the caller-traced rlSss families (include/rlshaders_amd_trace.h; csrc_trace/rls_trace_probe.hpp, rls_trace_hits.hpp) at
their grid, tile, sample-count and capacity edges, for two flavours:
  sss   rls_trace_sss_probe_emit / rls_trace_sss_scatter_resolve (trace.sss_probe_rays, ProbeQueue.resolve);
  hits  rls_trace_sss_hits_emit / rls_trace_sss_hits_resolve (trace.sss_hit_rays, HitQueues.resolve).

  A. several rounds of every grid-stride loop, on a context capped at one workgroup per CU (RLS_BLOCKS_PER_CU=1): the gate,
     list, emit, both compactions, fill and resolve kernels of the hits family with a list that ends inside a round, whole tiles
     of unlisted capacity behind it; hits_compact_kernel's one-hit tiles (8 lights x 2 segments x 256 samples = 4096 slots a hit);
     sss_probe_emit_kernel and sss_scatter_resolve_kernel on plane and sphere;
  B. every spp_n 1..16 of the gate, probe emit and scatter resolve at n = P + 1 and 2 P - 1 points, P the kernel's own tile;
     every hit_spp_n 1..16 (the emit's segment loops take up to 4 and 256 steps at G = 1), coloured visibility at hit_spp_n 16,
     hit_capacity at the shaded count and a compaction tile + 1 below it;
  C. every plane the verbs write a view inside a sentinel-filled buffer, scratch of exactly the documented size;
  D. NaN, infinities, denormals and huge values in the hits, the shading points and the profile parameters, hit counts of 0,
     max_hits, above max_hits and 255.

What a result is held to (nothing to the code under test):
  hits  the list to trace_hits_util.gate_np and a host int64 cumsum; E at unit visibility to rls_ggx_direct_lighting's
        direct_diffuse over the flattened elements on the default context, bit for bit; the shadow rays to
        rls_trace_ggx_direct_emit by (element, light, segment, sample); the diffuse ray to rls_sss_sample_diffuse_direction on
        orc_batch_sample_02; coloured visibility and radiance to trace_hits_util.compose_E and its float64 bound;
  sss   probes traced on the host through the analytic scene (trace_sss_util.trace_np: orc_scene_trace vectorised, checked
        against it on a sample of the rays) to rls_sss_integrate_scatter's result and mean_depth, bit for bit;
        orc_batch_sss_integrate_scatter on windows (cases.assert_tight); the queue to orc_batch_sample_02 + orc_batch_sss_probe
        and rls_sss_probe_ray.
  FAST on the sphere: the integrator intersects the sphere with the hardware's reciprocal and square root, which no host
  tracer reproduces (tests/test_gpu_trace_skin.py); there the capped context is held to the default context alone.

Tile constants (read from the sources below): kBlock 256, kSssEmitRays 1024, kSssEmitPoints 256 (sss_emit_tile_points = min(1024 /
spp, 256), sss_resolve_tile_points = 256 / spp), kShadowMaxSlots 6144, kCompactSlots 4096, kCompactMaxPoints 256,
RLS_SPEC_BLOCK 4."""
import re

import numpy as np
import pytest
import torch

import cases
import rlshaders_amd as R
import trace_sss_util as U
from gpu_util import dev, host
from test_gpu_loop_edges import LIGHTS, _lights, _sl
from test_gpu_trace_hits import (Hits, _assert_E, _bytes_equal, _ones, _sss, assert_documented_composition,
                                 assert_shadow_queue_invariants, assert_shadow_rays_are_the_ggx_emit)
from test_gpu_trace_node_edges import (KBLOCK, KCOMPACT, KMAXPTS, ROOT, SCRATCH_PAD, _SRC, Padded, T, _const, _math_mode,  # noqa: F401
                                       _poison_case, _rehouse, _sat_lights, _with_group, one_block_per_cu)
from test_gpu_trace_sss import _scene_pair, _setting
from trace_hits_util import DIFFUSE, gate_np, listed_elements, queues_host

pytestmark = pytest.mark.gpu

F = np.float32
SEED = 6173                                  # test_gpu_trace_hits.py's: Hits emits its probe queue with it
FIRST = (1 << 36) + 5
Z, X = np.array([0.0, 0.0, 1.0], F), np.array([1.0, 0.0, 0.0], F)

_LOOPS = (ROOT / "rlshaders_amd" / "csrc" / "rls_loops.hpp").read_text()
KSPEC = int(re.search(r"#define RLS_SPEC_BLOCK (\d+)", _LOOPS).group(1))
KMAXSPP = int(re.search(r"constexpr int kMaxSpp = (\d+);", _LOOPS).group(1))
MAXLIGHTS = int(re.search(r"#define RLS_MAX_LIGHTS\s+(\d+)", (ROOT / "include" / "rlshaders_amd.h").read_text()).group(1))
KEMITRAYS = int(re.search(r"constexpr int kSssEmitRays = (\d+) \* rlsh::kBlock;", _SRC).group(1)) * KBLOCK
assert re.search(r"constexpr int kSssEmitPoints = rlsh::kBlock;", _SRC)
KEMITPTS = KBLOCK
assert re.search(r"constexpr int kShadowMaxSlots = RLS_MAX_LIGHTS \* kShadowSegments \* kMaxSpp;", _SRC)
KSHADOWMAX = MAXLIGHTS * _const("kShadowSegments") * KMAXSPP
SEGS = _const("kSkinShadowSegments")         # the hit list's light loop: a light and a BSDF strategy, no specular segment
assert (KBLOCK, KEMITRAYS, KEMITPTS, KSHADOWMAX, KCOMPACT, KMAXPTS, KSPEC, KMAXSPP, SEGS) == (256, 1024, 256, 6144, 4096, 256, 4, 256, 2)


def emit_tile(spp):
    """sss_emit_tile_points: the points of a tile of sss_probe_emit_kernel and sss_hits_gate_kernel"""
    return min(KEMITRAYS // spp, KEMITPTS)


def resolve_tile(spp):
    """sss_resolve_tile_points: the points of a tile of sss_scatter_resolve_kernel"""
    return 1 if spp >= KBLOCK else KBLOCK // spp


def compact_tile(tile_slots, per_point):
    """compact_tile_points"""
    return min(tile_slots // per_point, KMAXPTS)


def rounds(cu, n, per_block):
    """the rounds a grid-stride loop over n items takes, per_block items a workgroup, on the capped context (grid_for: at most cu
    workgroups, a multiple of 8 from 8 on)"""
    want = max(1, min(-(-n // per_block), cu))
    if want >= 8:
        want = (want + 7) // 8 * 8
    return n / per_block / want


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _dev_same(a, b, what):
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    b = b.to(a.device)
    assert torch.equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum().item()), "words differ of", a.numel())


# ---- the two flavours ---------------------------------------------------------------------------------------------------------
def _hq_planes(hq):
    """every device plane of a HitQueues the verbs write, the rays' up to the counts"""
    sc, dc, listed = hq.shadow_count, hq.diffuse_count, hq.listed
    d = dict(hit_count=hq._hit_count, hit_element=hq._hit_element[:listed], shadow_offsets=hq.shadow_offsets,
             sdir=hq._sdir[:, :sc], smaxdist=hq._smaxdist[:sc], swd=hq._swd[:, :sc], skind=hq._skind[:sc], spoint=hq._spoint[:sc],
             ssample=hq._ssample[:sc])
    if hq.trace_diffuse:
        d.update(diffuse_offsets=hq.diffuse_offsets, ddir=hq._ddir[:, :dc], dw=hq._dw[:, :dc], dpoint=hq._dpoint[:dc])
    return d


def _same_hq(a, b, what):
    pa, pb = _hq_planes(a), _hq_planes(b)
    assert set(pa) == set(pb)
    for k in pa:
        _dev_same(pa[k], pb[k], (what, k))


QUEUE_PLANES = ("_hit_count", "_hit_element", "shadow_offsets", "_sdir", "_smaxdist", "_swd", "_skind", "_spoint", "_ssample",
                "diffuse_offsets", "_ddir", "_dw", "_dpoint")


def _unit_E(hq):
    """the resolve at visibility 1 (and, with a diffuse queue, radiance 0: the diffuse term adds +0 to a sum that is never -0),
    into planes that held -7 everywhere"""
    ctx = hq.ctx
    rad = torch.zeros(3, max(hq.diffuse_count, 1), dtype=torch.float32, device=ctx.torch_device) if hq.trace_diffuse else None
    out = torch.full((3, hq.max_hits, hq.stride), -7.0, dtype=torch.float32, device=ctx.torch_device)
    return host(hq.resolve(_ones(ctx, hq.shadow_count) if hq.n_lights else None, rad, out=out))


def _stale_queues(T, h, nl, hit_spp_n, diffuse):
    """HitQueues of the default capacity for h whose every plane holds 0xA5 bytes: what an emit leaves unwritten is not what an
    earlier emit wrote into the same memory"""
    hq = T.HitQueues(h.ctx, h.n, h.spp_n, h.max_hits, h.stride, h.max_hits * h.n * h.spp, nl, hit_spp_n, diffuse)
    for name in QUEUE_PLANES:
        getattr(hq, name).view(torch.uint8).fill_(0xA5)
    return hq


def _reference_counts(T, hits, lights, hit_spp_n, first=0):
    """per element the diffuse-carrying rays of rls_trace_ggx_direct_emit over the flattened elements (hits: on the context the
    reference runs on), counted on the device -> int64 [max_hits * stride]"""
    g, Pf = hits.ggx()
    q = T.ggx_shadow_rays(g, T.ggx_shader(g, KdColor=(1.0, 1.0, 1.0), Kd=1.0, diffuseRoughness=0.0, Ks=0.5), Pf, lights,
                          hit_spp_n, SEED, first)
    m = (q.kind.to(torch.int32) & DIFFUSE) != 0
    return host(torch.bincount(q.point[m].to(torch.int64), minlength=hits.max_hits * hits.stride))


def _diffuse_kept(oracle, hits, first=0):
    """per element whether integrateDiffuse's ray has a weight: the first point of the (0,2) sequence at pair 24 through
    rls_sss_sample_diffuse_direction, CLAMP(N . dir, 0, 1) != 0 in numpy float32 (test_diffuse_ray_direction_and_weight)"""
    total = hits.max_hits * hits.stride
    rx, ry = oracle.batch_sample_02(SEED, first, total, 24, 0)
    Nf, Tf = np.ascontiguousarray(hits.hN.reshape(3, -1)), np.ascontiguousarray(hits.hT.reshape(3, -1))
    d = host(R.SssSampler.sampleDiffuseDirection(hits.ctx, dev(rx), dev(ry), dev(Nf), dev(Tf)))
    with np.errstate(invalid="ignore", over="ignore"):
        nd = ((Nf[0] * d[0] + Nf[1] * d[1]).astype(F) + Nf[2] * d[2]).astype(F)
        return np.minimum(np.maximum(nd, F(0)), F(1)) != 0


def _csr(per_listed, cap):
    """the offsets of a queue over a list of len(per_listed) hits with capacity cap: a host int64 cumsum, flat past the list"""
    off = np.zeros(cap + 1, np.int64)
    off[1:len(per_listed) + 1] = np.cumsum(per_listed, dtype=np.int64)
    off[len(per_listed) + 1:] = off[len(per_listed)]
    return off


def _assert_list_and_offsets(hq, el, per_el, kept, what):
    """hit_element, hit_count and both offsets arrays against the host: gate_np's elements, the reference's per-element counts"""
    cap = hq.hit_capacity
    listed = min(len(el), cap)
    assert hq.hit_count == len(el), (what, hq.hit_count, len(el))
    np.testing.assert_array_equal(host(hq.hit_element), el[:listed], str(what))
    np.testing.assert_array_equal(host(hq.shadow_offsets), _csr(per_el[el[:listed]], cap), str((what, "shadow offsets")))
    if hq.trace_diffuse:
        np.testing.assert_array_equal(host(hq.diffuse_offsets), _csr(kept[el[:listed]].astype(np.int64), cap),
                                      str((what, "diffuse offsets")))


class Sss:
    """n points of one analytic setting (tests/test_gpu_trace_sss.py, _setting) on one context: the probe queue, its rays traced
    on the host through the analytic scene, the resolve and the integrator"""

    def __init__(self, T, ctx, kind, n, cavity, case=None):
        self.T, self.ctx, self.kind, self.n, self.cavity = T, ctx, kind, n, cavity
        c, kw, self.has_dPdu = _setting(kind, n)
        self.case = c if case is None else case
        self.so, self.sg = _scene_pair(use_cavity_fade=cavity, **kw)
        self.s = _sss(ctx, self.case, self.has_dPdu)
        self.P = dev(self.case["P"])

    def emit(self, spp_n, first=0, queue=None):
        return self.T.sss_probe_rays(self.s, self.P, spp_n, SEED, first_index=first, queue=queue)

    def traced(self, q):
        """the queue through the analytic scene on the host -> (count, P, N, E) numpy"""
        cnt, hP, hN = U.trace_np(self.so, host(q.origin), host(q.dir), host(q.maxdist))
        return cnt, hP, hN, U.light_irradiance(self.so, hP, hN)

    def resolve(self, q, hits, out=None, depth_out=None):
        got = q.resolve(*[dev(h) for h in hits], use_cavity_fade=self.cavity, want_depth=True, out=out, depth_out=depth_out)
        return host(got[0]), host(got[1])

    def integrator(self, spp_n, first=0):
        ref = self.s.integrateScatter(self.P, self.sg, spp_n, SEED, want_depth=True, first_index=first)
        return host(ref[0]), host(ref[1])


def _assert_tracer_is_the_oracles(oracle, so, q, hits, k=200):
    """the vectorised host tracer is orc_scene_trace on k of the rays"""
    cnt, hP, hN = hits[:3]
    o, d, md = host(q.origin), host(q.dir), host(q.maxdist)
    for j in np.linspace(0, len(md) - 1, k).astype(np.int64):
        c, _, hp, hn = oracle.scene_trace(so, o[:, j], d[:, j], md[j])
        assert c == cnt[j], j
        for m in range(c):
            assert np.array_equal(F(hp[m]), hP[:, m, j]) and np.array_equal(F(hn[m]), hN[:, m, j]), (j, m)


def _assert_emit_is_the_oracles(oracle, b, q, spp_n, first, a, e, samples=None, tight=True):
    """the rays of points [a, e) against rls_sss_probe_ray on orc_batch_sample_02's samples (bit for bit, or both NaN) and, with
    `tight`, against orc_batch_sss_probe on them (cases.assert_tight; EXACT, finite inputs)"""
    n, spp = b.n, spp_n * spp_n
    c = _sl(b.case, a, e)
    origin, dirs = (host(t).reshape(3, n, spp)[:, a:e] for t in (q.origin, q.dir))
    maxdist = host(q.maxdist).reshape(n, spp)[a:e]
    o = oracle.Sss(e - a, c["dist"], c["albedo"], N=c["N"], T=c["T"], has_dPdu=b.has_dPdu)
    s = _sss(b.ctx, c, b.has_dPdu)
    for smp in (range(spp) if samples is None else samples):
        rx, ry = oracle.batch_sample_02(SEED, first + a, e - a, 0, smp)
        got = s.getProbeRay(dev(rx), dev(ry), P=dev(c["P"]))
        U.same_bits_or_both_nan(origin[:, :, smp], host(got["origin"]), (a, smp, "origin vs rls_sss_probe_ray"))
        U.same_bits_or_both_nan(dirs[:, :, smp], host(got["dir"]), (a, smp, "dir vs rls_sss_probe_ray"))
        U.same_bits_or_both_nan(maxdist[:, smp], host(got["maxdist"]), (a, smp, "maxdist vs rls_sss_probe_ray"))
        if tight:
            ref = o.probe(rx, ry)
            cases.assert_tight(cases.summarize(cases.rel_err(origin[:, :, smp], (c["P"] + ref["origin"]).astype(F))), (a, smp, "origin"))
            cases.assert_tight(cases.summarize(cases.rel_err(dirs[:, :, smp], ref["dir"])), (a, smp, "dir"))
            cases.assert_tight(cases.summarize(cases.rel_err(maxdist[:, smp], ref["maxdist"])), (a, smp, "maxdist"))


def _assert_dense_queue(q, n, spp):
    np.testing.assert_array_equal(host(q.offsets), np.arange(n + 1, dtype=np.int64) * spp)
    np.testing.assert_array_equal(host(q.point), np.repeat(np.arange(n), spp))
    np.testing.assert_array_equal(host(q.sample), np.tile(np.arange(spp), n))


def _same_probe_queue(a, b, what):
    for k in ("offsets", "origin", "dir", "maxdist", "point", "sample"):
        _dev_same(getattr(a, k), getattr(b, k), (what, k))


# ---- A. several grid rounds --------------------------------------------------------------------------------------------------
def _shape_many(h):
    """by ray index mod 16, slot 0: 0 an upright hit at the origin (under _sat_lights: a ray in every shadow slot), 1 a hit at the
    origin that faces away from every light (no shadow ray); both reported.  The other rays are the generator's"""
    j = np.arange(h.stride)
    for r, nz in ((0, 1.0), (1, -1.0)):
        m = j % 16 == r
        h.hP[:, 0, m] = 0.0
        h.hN[:, 0, m] = (Z * F(nz))[:, None]
        h.hT[:, 0, m] = X[:, None]
        h.cnt[m] = np.maximum(h.cnt[m], 1)


def many_hits(T, ctx, cu, src=None):
    n = 2 * cu * 64 + cu * 32 + 3
    return Hits(T, ctx, n=n, spp_n=4, max_hits=2, shape=_shape_many, src=src)


def many_hits_shares(h, cavity=False):
    """gate_np on the CPU -> (elements, dict of the shares the generator produced)"""
    keep = gate_np(h.case, h.spp, h.cnt, h.hP, h.hN, h.max_hits, cavity)
    el = listed_elements(keep, h.stride)
    rays = h.n * h.spp
    listed = np.zeros(h.max_hits * h.stride, bool)
    listed[el] = True
    j = np.arange(rays)
    return el, dict(listed=len(el) / (h.max_hits * h.stride), rays_without=float((~keep).all(axis=0).mean()),
                    rays_full=float(keep.all(axis=0).mean()), saturated=int(listed[:rays][j % 16 == 0].sum()),
                    empty=int(listed[:rays][j % 16 == 1].sum()))


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_hits_many_hits_take_several_grid_rounds(gpu, oracle, T, one_block_per_cu, fast):
    """A, hits.  spp_n = 4 (the gate's tile: 64 points), n = 2.5 CU x 64 + 3 points, max_hits 2, two lights, hit_spp_n 1, the
    diffuse ray on, hit_capacity every element: the list ends inside a round of every list-indexed kernel.  The list, both offsets
    arrays, E and every queue byte against the host references and the default context; EXACT: also at G = 1 (the list's end
    mid-wavefront) and G = 64 (mid-workgroup), the queues' bytes the same"""
    ctx = one_block_per_cu
    cu = ctx.device_info()["compute_units"]
    h0 = many_hits(T, gpu, cu)
    h1 = many_hits(T, ctx, cu, src=h0)
    n, spp, rays, cap = h0.n, h0.spp, h0.n * h0.spp, h0.max_hits * h0.n * h0.spp
    el, share = many_hits_shares(h0)
    L = len(el)
    print("many hits:", dict(cu=cu, n=n, rays=rays, listed=L), share)
    assert 0.3 <= share["listed"] <= 0.7, share
    assert share["rays_without"] > 0.02 and share["rays_full"] > 0.02 and share["saturated"] > 100 and share["empty"] > 100, share
    nl, hit_spp_n = 2, 1
    slots = nl * SEGS * hit_spp_n * hit_spp_n
    r = dict(sss_hits_gate_kernel=rounds(cu, n, emit_tile(spp)), sss_hits_list_kernel=rounds(cu, rays, KBLOCK),
             sss_hits_emit_kernel_G1=L / KBLOCK / cu, sss_hits_emit_kernel_G64=L / (KBLOCK // 64) / cu,
             hits_compact_kernel=L / compact_tile(KSHADOWMAX, slots) / cu, trace_compact_kernel=L / compact_tile(KCOMPACT, 1) / cu,
             sss_hits_fill_kernel=rounds(cu, h0.max_hits * h0.stride, KBLOCK), sss_hits_resolve_kernel=L / KBLOCK / cu)
    print("rounds to the list's end on the capped context:", {k: round(v, 2) for k, v in r.items()})
    assert min(r.values()) >= 2.5, r
    # the list ends inside a round, and at least one whole round of unlisted capacity follows it
    for per in (KBLOCK, compact_tile(KSHADOWMAX, slots), compact_tile(KCOMPACT, 1)):
        assert L % (per * cu) != 0 and cap - L > per * cu
    assert rounds(cu, cap, KBLOCK) >= 8 and cu >= 8
    _, lights = _sat_lights(oracle, nl)
    _math_mode((gpu, ctx), fast)
    try:
        per_el, kept = _reference_counts(T, h0, lights, hit_spp_n, FIRST), _diffuse_kept(oracle, h0, FIRST)
        sat, emp = el[(el < rays) & (el % 16 == 0)], el[(el < rays) & (el % 16 == 1)]
        # (the reference's own counts; the lights leave 2e-6 of the hemisphere's measure uncovered)
        assert (per_el[sat] == slots).mean() > 0.99 and (per_el[emp] == 0).mean() > 0.99 and per_el[el].max() == slots
        want = h0.direct_diffuse(lights, hit_spp_n, first=FIRST)
        emit = lambda h: h.emit(lights, hit_spp_n, first=FIRST, trace_diffuse=True, queues=_stale_queues(T, h, nl, hit_spp_n, True))
        base = None
        for g in ((None,) if fast else (None, 1, 64)):
            q1, q0 = _with_group(g, lambda: emit(h1)), _with_group(g, lambda: emit(h0))
            _assert_list_and_offsets(q1, el, per_el, kept, (fast, g))
            _same_hq(q1, q0, (fast, g, "vs the default context"))
            if base is None:
                base = q1
            else:
                _same_hq(q1, base, (fast, g, "vs the host's pick of G"))
            E1 = _unit_E(q1)
            _assert_E(E1, want, el, (fast, g, "rls_ggx_direct_lighting"))
            assert _bytes_equal(E1, _unit_E(q0)), (fast, g, "E vs the default context")
    finally:
        _math_mode((gpu, ctx), False)


def _shape_one_hit_tiles(h):
    """dense hits (every ray's one hit listed); by index mod 16: 0 and 4 an upright hit at the origin, 1 one that faces away,
    where the origin lies well inside the shading point's radius (the list keeps its length: asserted with gate_np)"""
    Po = h.case["P"][:, np.minimum(np.arange(h.stride) // h.spp, h.n - 1)].astype(np.float64)
    maxR = 3.0 * h.case["dist"].max(axis=0)[np.minimum(np.arange(h.stride) // h.spp, h.n - 1)]
    r = np.linalg.norm(Po, axis=0)
    near = (r < 0.9 * maxR) & (r > 1e-3)
    j = np.arange(h.stride)
    for rs, nz in (((0, 4), 1.0), ((1,), -1.0)):
        m = near & np.isin(j % 16, rs)
        h.hP[:, 0, m] = 0.0
        h.hN[:, 0, m] = (Z * F(nz))[:, None]
        h.hT[:, 0, m] = X[:, None]


def test_hits_one_hit_compaction_tiles_take_several_grid_rounds(gpu, oracle, T, one_block_per_cu):
    """A, hits.  8 lights at hit_spp_n = 16: 8 x 2 x 256 = 4096 slots a hit, compact_tile_points(kShadowMaxSlots, 4096) = 1, a list
    of 2.5 CU + 1 hits: hits_compact_kernel's hand-advanced (sp, p) walk with pc == 1 in its second and third round.  The queue is
    the diffuse-carrying rays of rls_trace_ggx_direct_emit, E direct_diffuse"""
    ctx = one_block_per_cu
    cu = ctx.device_info()["compute_units"]
    n, nl, hit_spp_n = 2 * cu + cu // 2 + 1, 8, 16
    slots = nl * SEGS * hit_spp_n * hit_spp_n
    assert compact_tile(KSHADOWMAX, slots) == 1 and rounds(cu, n, 1) >= 2.5
    mk = lambda c, src=None: Hits(T, c, n=n, spp_n=1, max_hits=1, pad=0, dense=True, shape=_shape_one_hit_tiles, src=src)
    h0 = mk(gpu)
    h1 = mk(ctx, h0)
    el = h0.elements(False)
    assert len(el) == n
    _, lights = _sat_lights(oracle, nl)
    per_el = _reference_counts(T, h0, lights, hit_spp_n)
    assert per_el.max() == slots and per_el.min() == 0, (int(per_el.min()), int(per_el.max()), slots)
    want = h0.direct_diffuse(lights, hit_spp_n)
    for g in (1, None):
        q1, q0 = (_with_group(g, lambda: h.emit(lights, hit_spp_n, queues=_stale_queues(T, h, nl, hit_spp_n, False))) for h in (h1, h0))
        _assert_list_and_offsets(q1, el, per_el, None, g)
        _same_hq(q1, q0, (g, "vs the default context"))
        _assert_E(_unit_E(q1), want, el, (g, "rls_ggx_direct_lighting"))
    sh, _, elements, _ = queues_host(q1)
    assert_shadow_rays_are_the_ggx_emit(T, h0, sh, elements, lights, hit_spp_n)


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("cavity", [False, True], ids=["nofade", "fade"])
@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_sss_many_points_take_several_grid_rounds(gpu, oracle, T, one_block_per_cu, kind, cavity, fast):
    """A, sss.  spp_n = 4: sss_probe_emit_kernel's tile is 64 points, sss_scatter_resolve_kernel's 16; n = 2.5 CU x 64 + 3.  The
    queue, result and mean_depth carry the default context's bits and, the probes traced through the analytic scene, the
    integrator's; EXACT: windows of 300 points across the round boundaries of both kernels and at the tail against the oracle"""
    ctx = one_block_per_cu
    cu = ctx.device_info()["compute_units"]
    n, spp_n = 2 * cu * 64 + cu * 32 + 3, 4
    spp = spp_n * spp_n
    r = dict(sss_probe_emit_kernel=rounds(cu, n, emit_tile(spp)), sss_scatter_resolve_kernel=rounds(cu, n, resolve_tile(spp)))
    print("rounds on the capped context:", {k: round(v, 2) for k, v in r.items()})
    assert (emit_tile(spp), resolve_tile(spp)) == (64, 16) and min(r.values()) >= 2.5, r
    _math_mode((gpu, ctx), fast)
    try:
        b1, b0 = Sss(T, ctx, kind, n, cavity), Sss(T, gpu, kind, n, cavity)
        q1, q0 = b1.emit(spp_n, FIRST), b0.emit(spp_n, FIRST)
        _assert_dense_queue(q1, n, spp)
        _same_probe_queue(q1, q0, (kind, "vs the default context"))
        hits = b1.traced(q1)
        _assert_tracer_is_the_oracles(oracle, b1.so, q1, hits)
        got, dgot = b1.resolve(q1, hits)
        ref0, dref0 = b0.resolve(q0, hits)
        cases.assert_same_bits(got, ref0, (kind, cavity, "result vs the default context"))
        cases.assert_same_bits(dgot, dref0, (kind, cavity, "mean_depth vs the default context"))
        if not (fast and kind == "sphere"):
            ref, dref = b0.integrator(spp_n, FIRST)
            cases.assert_same_bits(got, ref, (kind, cavity, "result vs rls_sss_integrate_scatter"))
            cases.assert_same_bits(dgot, dref, (kind, cavity, "mean_depth vs rls_sss_integrate_scatter"))
        assert float(dgot.mean()) > 0.2
        if fast:
            return
        c = b1.case
        edges = [cu * emit_tile(spp), 2 * cu * emit_tile(spp), cu * resolve_tile(spp), 2 * cu * resolve_tile(spp)]
        for a in [e - 150 for e in edges] + [n - 300]:
            e = a + 300
            cw = _sl(c, a, e)
            o = oracle.Sss(300, cw["dist"], cw["albedo"], N=cw["N"], T=cw["T"], has_dPdu=b1.has_dPdu, nthreads=4)
            oref, odref = oracle.integrate_scatter(o, cw["P"], b1.so, spp_n, SEED, first_index=FIRST + a)
            cases.assert_tight(cases.summarize(cases.rel_err(got[:, a:e], oref)), (kind, cavity, a, "window vs the oracle"))
            np.testing.assert_array_equal(dgot[a:e], odref)
            _assert_emit_is_the_oracles(oracle, b1, q1, spp_n, FIRST, a, e, samples=(0, 7, 15))
    finally:
        _math_mode((gpu, ctx), False)


# ---- B. tile and sample-count edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp_n", list(range(1, 17)))
def test_hits_gate_at_every_spp_n(gpu, oracle, T, spp_n):
    """B.  sss_hits_gate_kernel: a tile of P = sss_emit_tile_points(spp) points; n = P + 1 (a tile of one point) and 2 P - 1 (a last
    tile one point short), max_hits 3, cavity fade on: the list is gate_np's elements and count"""
    spp = spp_n * spp_n
    P = emit_tile(spp)
    _, lights = _lights(oracle, LIGHTS[:1])
    for n in (P + 1, 2 * P - 1):
        hits = Hits(T, gpu, n=n, spp_n=spp_n, max_hits=3, seed=3 + spp_n)
        el = hits.elements(True)
        assert 0 < len(el) < 3 * n * spp
        hq = hits.emit(lights, 1, use_cavity_fade=True)
        assert hq.hit_count == len(el), (spp_n, n)
        np.testing.assert_array_equal(host(hq.hit_element), el, str((spp_n, n)))


@pytest.mark.parametrize("spp_n", list(range(1, 17)))
def test_sss_kernels_at_every_spp_n(gpu, oracle, T, spp_n):
    """B.  sss_probe_emit_kernel at n = P + 1 and 2 P - 1 of its tile P = sss_emit_tile_points(spp), sss_scatter_resolve_kernel at
    those of its own, sss_resolve_tile_points(spp): the emit is the oracle's and rls_sss_probe_ray's, the traced sphere (cavity
    fade on) rls_sss_integrate_scatter, bit for bit"""
    spp = spp_n * spp_n
    Pe, Pr = emit_tile(spp), resolve_tile(spp)
    for n in sorted({Pe + 1, 2 * Pe - 1, Pr + 1, 2 * Pr - 1}):
        b = Sss(T, gpu, "sphere", n, True)
        q = b.emit(spp_n, 77)
        _assert_dense_queue(q, n, spp)
        _assert_emit_is_the_oracles(oracle, b, q, spp_n, 77, 0, n, samples=sorted({0, min(1, spp - 1), spp // 2, spp - 1}))
        hits = b.traced(q)
        got, dgot = b.resolve(q, hits)
        ref, dref = b.integrator(spp_n, 77)
        cases.assert_same_bits(got, ref, (spp_n, n, "result"))
        cases.assert_same_bits(dgot, dref, (spp_n, n, "mean_depth"))


@pytest.mark.parametrize("hit_spp_n", list(range(1, 17)))
def test_hits_at_every_hit_spp_n(gpu, oracle, T, hit_spp_n):
    """B.  A list of a few hundred hits under the eight mixed-mode lights and under three: E at unit visibility is direct_diffuse
    bit for bit (EXACT; FAST at hit_spp_n 1, 7 and 16), the queue keeps its order, kind, cone and maxdist invariants; at hit_spp_n
    5, 7 and 16 also with G = 1, 4, 16 and 64 forced (at G = 1 the segment-0 loop takes hit_spp / RLS_SPEC_BLOCK steps, the
    segment-1 loop hit_spp)"""
    hit_spp = hit_spp_n * hit_spp_n
    hits = Hits(T, gpu)
    el = hits.elements(True)
    assert len(el) > 200
    for fast in ((False, True) if hit_spp_n in (1, 7, 16) else (False,)):
        gpu.set_math_mode(fast)
        try:
            for specs in (LIGHTS, LIGHTS[:3]):
                _, lights = _lights(oracle, specs)
                want = _with_group(1, lambda: hits.direct_diffuse(lights, hit_spp_n))
                base = None
                for g in ((None, 1, 4, 16, 64) if hit_spp_n in (5, 7, 16) and not fast else (None,)):
                    hq = _with_group(g, lambda: hits.emit(lights, hit_spp_n, use_cavity_fade=True))
                    _assert_E(_unit_E(hq), want, el, (hit_spp_n, fast, len(specs), g))
                    if base is None:
                        base = hq
                        sh, _, elements, _ = queues_host(hq)
                        np.testing.assert_array_equal(elements, el)
                        assert_shadow_queue_invariants(hits, sh, elements, hq.hit_capacity, specs, hit_spp)
                        assert np.diff(sh["offsets"]).max() > hit_spp
                    else:
                        _same_hq(hq, base, (hit_spp_n, len(specs), g, "the queues do not depend on G"))
        finally:
            gpu.set_math_mode(False)


def test_hits_coloured_visibility_at_hit_spp_n_16(gpu, oracle, T):
    """B.  Random visibility and radiance over eight decades at 256 samples a light, three lights: compose_E bit for bit and the
    float64 bound of test_coloured_visibility_and_radiance_follow_the_documented_composition"""
    _, lights = _lights(oracle, LIGHTS[:3])
    r = assert_documented_composition(gpu, Hits(T, gpu), lights, 16)
    assert np.diff(r["sh"]["offsets"]).max() > 256 and r["df"]["count"] > 100


def test_hits_capacity_at_and_a_tile_below_the_shaded_count(gpu, oracle, T):
    """B.  hit_capacity exactly the shaded count, and a compaction tile + 1 below it (a whole tile's worth of listed hits does not
    fit): hit_count is the true count, the queues are the full run's prefix, E is +0 at the hits that did not fit"""
    nl, hit_spp_n = 3, 2
    _, lights = _lights(oracle, LIGHTS[:nl])
    hits = Hits(T, gpu, n=197)
    el = hits.elements(True)
    tile = compact_tile(KSHADOWMAX, nl * SEGS * hit_spp_n * hit_spp_n)
    assert tile == KMAXPTS and len(el) > 2 * tile + 1
    full = hits.emit(lights, hit_spp_n, trace_diffuse=True, use_cavity_fade=True)
    fs, fd, fel, _ = queues_host(full)
    np.testing.assert_array_equal(fel, el)
    Efull = host(full.resolve(_ones(gpu, fs["count"]), _ones(gpu, fd["count"]))).reshape(3, -1)
    for cap in (len(el), len(el) - tile - 1):
        hq = hits.emit(lights, hit_spp_n, trace_diffuse=True, use_cavity_fade=True, hit_capacity=cap)
        sh, df, elements, count = queues_host(hq)
        assert count == len(el) and hq.listed == cap and hq.hit_capacity == cap
        np.testing.assert_array_equal(elements, el[:cap])
        lo, dlo = int(fs["offsets"][cap]), int(fd["offsets"][cap])
        np.testing.assert_array_equal(sh["offsets"], fs["offsets"][:cap + 1])
        np.testing.assert_array_equal(df["offsets"], fd["offsets"][:cap + 1])
        assert sh["count"] == lo and df["count"] == dlo and lo > 0 and dlo > 0
        for k in ("dir", "maxdist", "wd", "kind", "point", "sample"):
            assert _bytes_equal(sh[k], fs[k][..., :lo]), (cap, k)
        for k in ("dir", "weight", "point"):
            assert _bytes_equal(df[k], fd[k][..., :dlo]), (cap, k)
        E = host(hq.resolve(_ones(gpu, sh["count"]), _ones(gpu, df["count"])))
        want = Efull.copy()
        want[:, el[cap:]] = 0                                        # the hits that did not fit are not shaded
        _assert_E(E, want.reshape(E.shape), el[:cap], ("capacity", cap))


# ---- C. nothing is written outside the caller's views ------------------------------------------------------------------------
def _padded_hit_queues(T, hits, nl, hit_spp_n, pad):
    """HitQueues of the default capacity whose every plane, and the scratch of exactly rls_trace_sss_hits_scratch_bytes, is a view
    inside a sentinel-filled buffer; the C struct follows"""
    cap = hits.max_hits * hits.n * hits.spp
    hq = T.HitQueues(hits.ctx, hits.n, hits.spp_n, hits.max_hits, hits.stride, cap, nl, hit_spp_n, True)
    assert hq._scratch.numel() == T.sss_hits_scratch_bytes(hits.n, hits.spp_n, hits.max_hits, cap, nl, hit_spp_n)
    for name in QUEUE_PLANES:
        setattr(hq, name, pad.like(getattr(hq, name)))
    hq._scratch = pad.like(hq._scratch, SCRATCH_PAD)
    capi, q = T.capi, hq.q
    q.hit_count, q.hit_element = hq._hit_count.data_ptr(), hq._hit_element.data_ptr()
    q.shadow.offsets, q.diffuse.offsets = hq.shadow_offsets.data_ptr(), hq.diffuse_offsets.data_ptr()
    q.shadow.dir = capi.Vec3(*[hq._sdir[k].data_ptr() for k in range(3)])
    q.shadow.maxdist, q.shadow.weight_diffuse = hq._smaxdist.data_ptr(), capi.Rgb(hq._swd[0].data_ptr(), None, None)
    q.shadow.kind, q.shadow.point, q.shadow.sample = hq._skind.data_ptr(), hq._spoint.data_ptr(), hq._ssample.data_ptr()
    q.diffuse.dir = capi.Vec3(*[hq._ddir[k].data_ptr() for k in range(3)])
    q.diffuse.weight, q.diffuse.point = capi.Rgb(hq._dw[0].data_ptr(), None, None), hq._dpoint.data_ptr()
    q.scratch, q.scratch_bytes = hq._scratch.data_ptr(), hq._scratch.numel()
    return hq


SHAPES = [(1001, 3, 2, 2), (5, 16, 8, 16)]


@pytest.mark.parametrize("n,spp_n,nl,hit_spp_n", SHAPES, ids=["1001", "slot_maximum"])
def test_hits_nothing_is_written_outside_the_callers_views(gpu, oracle, T, n, spp_n, nl, hit_spp_n):
    """C, hits.  hit_count, hit_element, both queues' offsets and every dir, maxdist, weight, kind, point and sample plane, the E
    planes of exactly max_hits x stride words each and a scratch of exactly rls_trace_sss_hits_scratch_bytes, 67 words (the
    scratch: 67 x 256 bytes) inside buffers of 0x7FC0DEAD: after emit and resolve every guard word holds the sentinel, the views
    the bytes of the plain run"""
    _, lights = _sat_lights(oracle, nl)
    hits = Hits(T, gpu, n=n, spp_n=spp_n, max_hits=2, pad=0, shape=_shape_many)
    for g in (1, 64):
        plain = _with_group(g, lambda: hits.emit(lights, hit_spp_n, trace_diffuse=True))
        per = np.diff(host(plain.shadow_offsets))[:plain.listed]
        assert per.max() == nl * SEGS * hit_spp_n * hit_spp_n and per.min() == 0 and plain.listed > n
        gen = torch.Generator(device=gpu.torch_device)
        gen.manual_seed(n)
        vis, rad = (torch.rand(3, c, generator=gen, device=gpu.torch_device) for c in (plain.shadow_count, plain.diffuse_count))
        want = plain.resolve(vis, rad)
        pad = Padded()
        hq = _padded_hit_queues(T, hits, nl, hit_spp_n, pad)
        E = pad.like(torch.empty(3 * hits.max_hits * hits.stride, dtype=torch.float32, device=gpu.torch_device))
        E = E.view(3, hits.max_hits, hits.stride)
        _with_group(g, lambda: hits.emit(lights, hit_spp_n, trace_diffuse=True, queues=hq))
        got = hq.resolve(vis, rad, out=E)
        torch.cuda.synchronize()
        pad.check(("hits", n, g))
        _same_hq(hq, plain, (n, g, "in padded buffers"))
        _dev_same(got, want, (n, g, "E in padded buffers"))


@pytest.mark.parametrize("n,spp_n,nl,hit_spp_n", SHAPES, ids=["1001", "slot_maximum"])
def test_sss_nothing_is_written_outside_the_callers_views(gpu, oracle, T, n, spp_n, nl, hit_spp_n):
    """C, sss.  The probe queue's planes at capacity exactly n x spp, result and mean_depth as views inside sentinel-filled
    buffers, the irradiance the resolve reads too (a read beside it would bring the sentinel, a NaN, into the sums): every guard
    word unchanged, the views the bytes of the plain run"""
    for kind in ("plane", "sphere"):
        b = Sss(T, gpu, kind, n, True)
        plain = b.emit(spp_n, FIRST)
        hits = b.traced(plain)
        want, dwant = b.resolve(plain, hits)
        pad = Padded()
        q = T.ProbeQueue(gpu, n, spp_n)
        assert q.capacity == n * spp_n * spp_n
        _rehouse(T, q, pad)
        b.emit(spp_n, FIRST, queue=q)
        Ed = dev(hits[3])
        E = pad.like(Ed.reshape(-1))
        E.copy_(Ed.reshape(-1))
        out, depth = pad.empty((3, n), gpu.torch_device), pad.empty((n,), gpu.torch_device)
        got, dgot = b.resolve(q, hits[:3] + (E.view(Ed.shape),), out=out, depth_out=depth)
        torch.cuda.synchronize()
        pad.check(("sss", kind, n))
        _same_probe_queue(q, plain, (kind, n, "in padded buffers"))
        cases.assert_same_bits(got, want, (kind, n, "result"))
        cases.assert_same_bits(dgot, dwant, (kind, n, "mean_depth"))
        ref, dref = b.integrator(spp_n, FIRST)
        cases.assert_same_bits(got, ref, (kind, n, "result vs rls_sss_integrate_scatter"))
        cases.assert_same_bits(dgot, dref, (kind, n, "mean_depth vs rls_sss_integrate_scatter"))


# ---- D. hostile per-hit and per-point inputs ---------------------------------------------------------------------------------
def _poison_hits(h):
    """SPECIAL in 2 % of the words of hits.P, hits.N, hitT, the points' P, N, T and the profile parameters; hits.count at 0,
    max_hits, above max_hits and 255 (a negative count's byte) on every 11th ray.  h.dirty_ray / h.dirty_pt: what was touched"""
    rng = np.random.default_rng(91)
    rays = h.n * h.spp
    per_ray, dirty_ray = _poison_case(dict(hP=h.hP.reshape(-1, h.stride), hN=h.hN.reshape(-1, h.stride),
                                           hT=h.hT.reshape(-1, h.stride)), rng, h.stride)
    h.hP, h.hN, h.hT = (per_ray[k].reshape(3, h.max_hits, h.stride) for k in ("hP", "hN", "hT"))
    h.case, h.dirty_pt = _poison_case(h.case, rng, h.n)
    j = np.arange(0, h.stride, 11)
    h.cnt[j] = np.array([0, h.max_hits, h.max_hits + 2, 255], np.uint8)[np.arange(len(j)) % 4]
    dirty_ray[j] = True
    h.dirty_ray = dirty_ray[:rays] | np.repeat(h.dirty_pt, h.spp)


def _assert_csr(off, point, listed, cap, per_max, what):
    cnt = np.diff(off)
    assert off[0] == 0 and (cnt >= 0).all() and (cnt <= per_max).all() and not cnt[listed:].any(), what
    np.testing.assert_array_equal(point, np.repeat(np.arange(cap), cnt), str(what))


def _rays_of(q, elements, keep_el):
    """the planes of the rays whose hit's element is in the boolean set keep_el, in queue order, and those elements"""
    e = elements[q["point"]]
    m = keep_el[e]
    return {k: np.ascontiguousarray(v[..., m]) for k, v in q.items() if k in ("dir", "maxdist", "wd", "kind", "sample", "weight")}, e[m]


def test_hits_hostile_hits_and_points(gpu, oracle, T):
    """D, hits.  The emit returns RLS_OK (the binding raises otherwise); hit_count <= capacity; hit_element ascends ray-major and
    within a ray; both queues are valid CSR; the untouched rays of untouched points keep their hits' place in the list and their
    rays, bit for bit; E at unit visibility is direct_diffuse on the same hostile planes at every listed element (or both NaN)
    and +0 elsewhere"""
    n, spp_n, max_hits, nl, hit_spp_n = 301, 3, 3, 2, 2
    bad = Hits(T, gpu, n=n, spp_n=spp_n, max_hits=max_hits, shape=_poison_hits)
    clean = Hits(T, gpu, n=n, spp_n=spp_n, max_hits=max_hits)
    rays, stride, total = n * bad.spp, bad.stride, max_hits * bad.stride
    assert bad.dirty_ray.any() and (~bad.dirty_ray).sum() > rays // 4
    assert not np.array_equal(bad.hP, clean.hP, equal_nan=True) and np.isnan(bad.case["dist"]).any()
    _, lights = _sat_lights(oracle, nl)
    for g, cavity in ((1, True), (64, False)):
        qc = _with_group(g, lambda: clean.emit(lights, hit_spp_n, trace_diffuse=True, use_cavity_fade=cavity))
        qb = _with_group(g, lambda: bad.emit(lights, hit_spp_n, trace_diffuse=True, use_cavity_fade=cavity))
        sb, db, eb, count = queues_host(qb)
        sc, dc, ec, _ = queues_host(qc)
        cap = qb.hit_capacity
        assert 0 < count <= cap and len(eb) == count
        jb, kb = eb % stride, eb // stride
        assert (jb < rays).all() and (kb < max_hits).all() and np.all(np.diff(jb * 16 + kb) > 0)       # ray-major, slots ascending
        assert (kb < np.minimum(bad.cnt[jb].astype(np.int64), max_hits)).all()                       # a reported slot
        _assert_csr(sb["offsets"], sb["point"], count, cap, nl * SEGS * hit_spp_n * hit_spp_n, (g, "shadow"))
        _assert_csr(db["offsets"], db["point"], count, cap, 1, (g, "diffuse"))
        assert sb["offsets"][cap] == sb["count"] and db["offsets"][cap] == db["count"]
        assert (sb["sample"] < hit_spp_n * hit_spp_n).all() and np.isin(sb["kind"] & 7, range(nl)).all()
        # the untouched rays: the same listed elements in the same order, the same rays
        keep_el = np.zeros(total, bool)
        keep_el.reshape(max_hits, stride)[:, :rays] = ~bad.dirty_ray[None, :]
        np.testing.assert_array_equal(eb[keep_el[eb]], ec[keep_el[ec]])
        assert keep_el[ec].sum() > 100
        for hb, hc in ((sb, sc), (db, dc)):
            (rb, wb), (rc, wc) = _rays_of(hb, eb, keep_el), _rays_of(hc, ec, keep_el)
            np.testing.assert_array_equal(wb, wc)
            for k in rb:
                assert _bytes_equal(rb[k], rc[k]), (g, k, "rays of the untouched hits")
        # E from an emit without the diffuse queue (a NaN normal gives a NaN weight, which no radiance silences)
        qe = _with_group(g, lambda: bad.emit(lights, hit_spp_n, use_cavity_fade=cavity))
        np.testing.assert_array_equal(host(qe.hit_element), eb)
        want = _with_group(g, lambda: bad.direct_diffuse(lights, hit_spp_n))
        E = _unit_E(qe).reshape(3, -1)
        U.same_bits_or_both_nan(E[:, eb], want.reshape(3, -1)[:, eb], (g, "E vs direct_diffuse on the hostile planes"))
        rest = np.ones(total, bool)
        rest[eb] = False
        assert not E[:, rest].view(np.uint32).any(), (g, "an unlisted element is not +0")


def _gate_planes(elements, shape, seed):
    """two irradiance planes [3, max_hits, stride] with the same finite values at the listed elements, NaN against +0 elsewhere"""
    rng = np.random.default_rng(seed)
    base = (rng.random((3, shape[0] * shape[1])) * 2).astype(F)
    listed = np.zeros(shape[0] * shape[1], bool)
    listed[elements] = True
    a, b = base.copy(), base.copy()
    a[:, ~listed], b[:, ~listed] = np.nan, 0.0
    return a.reshape(3, *shape), b.reshape(3, *shape)


def test_the_list_is_the_scatter_resolves_gate_under_hostile_hits(gpu, oracle, T):
    """D.  rls_trace_sss_scatter_resolve gives the same bits whether the irradiance is NaN or 0 at every unlisted element
    (scatter_ray_terms adds +0 for a hit its gate rejects): sss_hits_gate_kernel's staged copy of the gate's inputs and the
    resolve's recomputed ones agree on every hit, clean and hostile, fade on and off"""
    n, spp_n, max_hits = 301, 3, 3
    for h in (Hits(T, gpu, n=n, spp_n=spp_n, max_hits=max_hits), Hits(T, gpu, n=n, spp_n=spp_n, max_hits=max_hits, shape=_poison_hits)):
        d = h.d
        for cavity in (False, True):
            hq = h.emit(None, 1, use_cavity_fade=cavity)
            el = host(hq.hit_element)
            assert 100 < len(el) == hq.hit_count
            Ea, Eb = _gate_planes(el, (max_hits, h.stride), 5)
            ra, da = h.pq.resolve(d["cnt"], d["hP"], d["hN"], dev(Ea), use_cavity_fade=cavity, want_depth=True)
            rb, dbb = h.pq.resolve(d["cnt"], d["hP"], d["hN"], dev(Eb), use_cavity_fade=cavity, want_depth=True)
            U.same_bits_or_both_nan(host(ra), host(rb), (cavity, "result: NaN against 0 at the unlisted elements"))
            cases.assert_same_bits(host(da), host(dbb), (cavity, "mean_depth"))
            # and the list's length is the resolve's shaded count: mean_depth x spp summed over the points
            per_point = np.bincount((el % h.stride) // h.spp, minlength=n)
            np.testing.assert_array_equal(host(da), (per_point.astype(F) * (F(1) / F(h.spp))).astype(F))
            assert np.isfinite(host(rb)).all(axis=0).mean() > 0.5


def test_the_list_is_the_skin_resolves_gate_under_hostile_hits(gpu, oracle, T):
    """D.  The same through rls_trace_skin_resolve: the rlSkin node on the plane, its probes traced on the host, SPECIAL in 2 % of
    the hits' words and the count edits; the list comes from the hit verbs with an SssSampler of the node's scatter parameters"""
    from test_gpu_trace_skin import Skin, _mk_lights, _resolve, _traced
    from test_gpu_trace_hits import ONE_LIGHT
    n, spp_n = 131, 3
    b = Skin(gpu, oracle, n, "plane", cavity=True)
    q = b.emit(T, _mk_lights([ONE_LIGHT]), spp_n)
    cnt, hP, hN, _ = b.hits(q)
    rng = np.random.default_rng(7)
    planes, _ = _poison_case(dict(hP=hP.reshape(-1, hP.shape[2]), hN=hN.reshape(-1, hN.shape[2])), rng, hP.shape[2])
    hP, hN = planes["hP"].reshape(hP.shape), planes["hN"].reshape(hN.shape)
    j = np.arange(0, len(cnt), 11)
    cnt = cnt.copy()
    cnt[j] = np.array([0, 1, 3, 255], np.uint8)[np.arange(len(j)) % 4]
    p = b.p
    dv = lambda v: dev(v) if isinstance(v, np.ndarray) else v
    s = R.SssSampler(gpu, dev(b.frame[1]), dev(b.frame[2]), dv(p["sss_color"]), dv(p["sss_scatter_dist"]),
                     multiplier=dv(p["sss_dist_multiplier"]))
    hq = T.sss_hit_rays(s, b.P, q.probes, dev(cnt), dev(hP), dev(hN), None, 1, SEED, use_cavity_fade=True)
    el = host(hq.hit_element)
    assert len(el) > n // 2
    Ea, Eb = _gate_planes(el, hP.shape[1:], 6)
    traced = _traced(gpu, q, (1.0, 1.0, 1.0))
    got, want = _resolve(b, q, traced, (cnt, hP, hN, Ea)), _resolve(b, q, traced, (cnt, hP, hN, Eb))
    for k in ("sss", "out"):
        U.same_bits_or_both_nan(got[k], want[k], (k, "NaN against 0 at the unlisted elements"))
    assert np.any(want["sss"] != 0) and np.isfinite(want["sss"]).all(axis=0).mean() > 0.5


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_sss_hostile_closure_planes(gpu, oracle, T, kind):
    """D, sss.  SPECIAL in 2 % of the words of P, N, T and the profile parameters: the probe emit is rls_sss_probe_ray on the same
    inputs and, the probes traced through the analytic scene, the scatter resolve rls_sss_integrate_scatter, bit for bit or both
    NaN; the untouched points keep the clean run's rays"""
    n, spp_n = 1001, 3
    spp = spp_n * spp_n
    clean = Sss(T, gpu, kind, n, True)
    case, dirty = _poison_case(clean.case, np.random.default_rng(41), n)
    bad = Sss(T, gpu, kind, n, True, case=case)
    assert dirty.any() and (~dirty).sum() > n // 4
    qc, qb = clean.emit(spp_n, FIRST), bad.emit(spp_n, FIRST)
    _assert_dense_queue(qb, n, spp)
    for k in ("origin", "dir", "maxdist"):
        x, y = (host(getattr(q, k)).reshape(-1, n, spp)[:, ~dirty] for q in (qb, qc))
        assert _bytes_equal(x, y), (k, "rays of the untouched points")
    _assert_emit_is_the_oracles(oracle, bad, qb, spp_n, FIRST, 0, n, tight=False)
    _assert_emit_is_the_oracles(oracle, clean, qc, spp_n, FIRST, 0, n)
    got, dgot = bad.resolve(qb, bad.traced(qb))
    ref, dref = bad.integrator(spp_n, FIRST)
    U.same_bits_or_both_nan(got, ref, (kind, "result vs rls_sss_integrate_scatter on the hostile planes"))
    U.same_bits_or_both_nan(dgot, dref, (kind, "mean_depth"))
    cgot, _ = clean.resolve(qc, clean.traced(qc))
    cases.assert_same_bits(got[:, ~dirty], cgot[:, ~dirty], (kind, "the untouched points' result"))
