"""GPU: the caller-traced light loops, whole nodes and rlSkin node (include/rlshaders_amd_trace.h; csrc_trace/trace.hip) at their
grid, scan-tile and compaction-tile edges, for five flavours behind one interface: lights-ggx, lights-disney
(rls_trace_*_direct_*), node-ggx, node-disney (rls_trace_*_shade_*) and skin (rls_trace_skin_*):

  A. several rounds of every grid-stride loop, on a context capped at one workgroup per CU (RLS_BLOCKS_PER_CU=1):
     A1 many points -- the emit kernels (ggx_direct_emit_kernel, disney_direct_emit_kernel, the five node emits,
        skin_shadow_emit_kernel, the two skin glossy emits, skin_probe_emit_kernel), trace_scan_add_kernel,
        trace_compact_kernel, shadow_compact_kernel, shadow_resolve_kernel, ggx_node_resolve_kernel,
        disney_node_resolve_kernel, skin_node_resolve_kernel run two and a half rounds and more;
     A2 one-point compaction tiles (8 lights x 3 segments x 256 samples = kShadowMaxSlots slots a point): shadow_compact_kernel's
        hand-advanced (sp, p) walk with pc == 1, grid-striding;
  B. n around kScanTile and 3 kScanTile + 5 at spp_n 2 and 3: trace_scan_block_kernel / _totals_ / _add_ with a carry and a
     partial last scan tile together with a partial last compaction tile, against chunked emits and a host int64 cumsum --
     rlSkin's four scans a call among them;
  C. every queue plane, side plane, scratch block and AOV plane a view inside a sentinel-filled buffer, queues and scratch of
     exactly the documented minimum size: nothing but the views is written (staging(), every kernel's stores);
  D. NaN, infinities, denormals and huge values in 2 % of the words of every per-point input plane: the emits' keep / drop
     decisions, ranks and counts stay a valid CSR queue, untouched points keep their rays, the unit resolve is the analytic
     call on the same inputs.

What a result is held to: the analytic call on the default context bit for bit (rls_*_direct_lighting, rls_*_shade(env = 1),
rls_skin_integrate with the probes traced through the analytic plane); the oracle's two-sums batch functions on windows
(cases.assert_tight); the documented float32 composition of tests/trace_lights_util.py and tests/test_gpu_trace_shade.py.

Inputs: the generators of the functional files with, by index mod 16, a point that fills every queue to its slot count (an
upright frame under lights that cover the hemisphere, a low roughness), a point without any ray (inside the lights, a view
from below or every lobe gated), and the nodes' gates; every test asserts that both extremes occur in every compacted queue.

Tile constants (named here, read from the sources below): kBlock 256 (rls_internal.hpp); kScanTile 2048, kCompactSlots 4096,
kCompactMaxPoints 256, kShadowMaxSlots 6144, kShadowTile = kResolveTile 1024 (rls_trace_device.hpp); the scatter
walk's sub-tile kBlock / spp points (sss_resolve_tile_points)."""
import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import cases
import rlshaders_amd as R
import test_gpu_trace_shade as TS
import test_gpu_trace_skin as TK
import trace_sss_util as U
from gpu_util import dev, disney_oracle, disney_sampler, ggx_oracle, ggx_sampler, host
from test_gpu_hostile_inputs import SPECIAL
from test_gpu_loop_edges import SENTINEL, _lights, _sl, make_case
from test_gpu_trace_edges import _same as _same_nan
from test_gpu_trace_lights import Batch, _rad, _visibility, bsdf_directions_against_the_oracle
from trace_lights_util import assert_float64_bound, compose, queue_host

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
_SRC = "".join(p.read_text() for p in [ROOT / "rlshaders_amd" / "csrc" / "rls_internal.hpp",
                                       *sorted((ROOT / "rlshaders_amd" / "csrc_trace").iterdir())])


def _const(name):
    return int(re.search(r"constexpr int " + name + r" = (\d+);", _SRC).group(1))


KBLOCK = int(re.search(r"#define RLS_BLOCK (\d+)", _SRC).group(1))                       # 256
KSCAN = KBLOCK * int(re.search(r"constexpr int kScanPer = (\d+);", _SRC).group(1))       # kScanTile 2048
KCOMPACT, KMAXPTS = _const("kCompactSlots"), _const("kCompactMaxPoints")                 # 4096, 256
KTILE = _const("kResolveTile")                                                           # kShadowTile = kResolveTile 1024
assert (KBLOCK, KSCAN, KCOMPACT, KMAXPTS, KTILE, _const("kShadowTile")) == (256, 2048, 4096, 256, 1024, 1024)

FLAVOURS = ("lights-ggx", "lights-disney", "node-ggx", "node-disney", "skin")
SEED = 77
FIRST = (1 << 36) + 5
F = np.float32
Z, X = np.array([0.0, 0.0, 1.0], F), np.array([1.0, 0.0, 0.0], F)
INSIDE = np.array([0.1, 0.2, 0.9], F)                 # a shading point inside every light of _sat_lights
RADS = ((3.0, 2.0, 1.0), (0.5, 4.0, 2.0), (1.0, 1.0, 6.0), (1.0, 1.0, 1.0), (2.0, 2.0, 2.0), (0.3, 0.6, 0.9), (5.0, 1.0, 1.0),
        (0.7, 0.7, 0.2))


def _sat_lights(oracle, nl):
    """nl lights of one geometry and nl radiances, both strategies: from the origin each covers the hemisphere about +z but
    for 2e-6 of its cosine-weighted measure, so an upright point there has a ray in every slot; the slab's and the plane's
    other points see them as ordinary lights -- below the horizon of some frames, around some points (no valid cone)"""
    return _lights(oracle, [dict(center=(0.0, 0.0, 1.0), radius=0.999999, radiance=RADS[l], mis_mode=0) for l in range(nl)])


@pytest.fixture(scope="module")
def T():
    from rlshaders_amd import build, trace
    build.build_trace_library()
    trace.load()
    return trace


@pytest.fixture(scope="module")
def one_block_per_cu():
    """a context whose grids are capped at one workgroup per CU (RLS_BLOCKS_PER_CU, read at context creation):
    tests/test_gpu_loop_edges.py"""
    mp = pytest.MonkeyPatch()
    mp.setenv("RLS_BLOCKS_PER_CU", "1")
    try:
        ctx = R.Context(0)
    finally:
        mp.undo()
    yield ctx
    ctx.close()


def _with_group(g, fn):
    """fn() with RLS_INTEGRATE_GROUP = g (None: unset, the host picks the width)"""
    old = os.environ.pop("RLS_INTEGRATE_GROUP", None)
    if g is not None:
        os.environ["RLS_INTEGRATE_GROUP"] = str(g)
    try:
        return fn()
    finally:
        os.environ.pop("RLS_INTEGRATE_GROUP", None)
        if old is not None:
            os.environ["RLS_INTEGRATE_GROUP"] = old


# ---- the inputs --------------------------------------------------------------------------------------------------------------
_CASES = {}


def _put(a, mask, v):
    a[..., mask] = np.asarray(v, F)[:, None] if a.ndim == 2 else F(v)


def _host_case(fl, oracle, m):
    """the m points of one flavour on the host: a dict of float32 planes [.., m] (rlSkin: the parameters in c["params"]).
    By index mod 16: 0 and 4 points that fill every queue, 1 the point without rays, 2.. the node's gates, 11.. the generator's"""
    key = (fl.split("-")[-1], m)
    if key in _CASES:
        return _CASES[key]
    k = np.arange(m) % 16
    full, dead = (k == 0) | (k == 4), k == 1                        # (two of the first five points: n = 5 has both extremes)
    if key[0] == "ggx":
        c = {q: np.array(v, F) for q, v in make_case("ggx_shade", oracle, m).items()}
        for q, v in (("wo", Z), ("N", Z), ("T", X), ("P", (0.0, 0.0, 0.0)), ("KsColor", (0.9, 0.9, 0.9)), ("kdc", (0.9, 0.8, 0.7)),
                     ("ktc", (0.9, 0.9, 0.9)), ("roughness", 0.1), ("anisotropic", 0.0), ("ior", 1.5), ("kd", 0.8), ("kdr", 0.3),
                     ("ks", 0.7), ("kt", 0.6)):
            _put(c[q], full, v)
        for q, v in (("wo", Z), ("N", Z), ("T", X), ("P", INSIDE), ("KsColor", (0.0, 0.0, 0.0)), ("kd", 0.0), ("kt", 0.0)):
            _put(c[q], dead, v)
        _put(c["kd"], k == 2, 0.0)                                   # the node's gates (tests/test_gpu_shade.py)
        _put(c["kt"], k == 3, 0.0)
        _put(c["KsColor"], k == 5, (0.0, 0.0, 0.0))
    elif key[0] == "disney":
        c = {q: np.array(v, F) for q, v in make_case("disney_shade", oracle, m).items()}
        _put(c["metallic"], np.arange(m) % 3 == 1, 1.0)             # every third point metallic: no diffuse lobe
        for q, v in (("wo", Z), ("N", Z), ("T", X), ("P", (0.0, 0.0, 0.0)), ("base_color", (0.9, 0.8, 0.7)), ("roughness", 0.1),
                     ("metallic", 0.3), ("clearcoat", 0.0), ("anisotropic", 0.0)):
            _put(c[q], full, v)
        for q, v in (("wo", -Z), ("N", Z), ("T", X), ("P", INSIDE), ("metallic", 1.0)):      # a view from below: no lobe has a sample
            _put(c[q], dead, v)
    else:
        # tests/test_gpu_trace_skin.py, Skin: cases.skin_mixed on the plane z = 0 with N = z, T = x
        s = cases.skin_mixed(cases.SEED_PARITY, m)
        p = {q: np.array(v, F) for q, v in s["params"].items()}
        P = np.zeros((3, m), F)
        P[:2] = np.stack([oracle.gen_uniform(TK.SEED, 0, m, 40 + j, -0.5, 0.5) for j in range(2)])
        wo = np.array(cases.frame(cases.SEED_PARITY, m)[0], F)
        wo[2] = np.abs(wo[2]) + 0.05
        wo = (wo / np.linalg.norm(wo, axis=0, keepdims=True)).astype(F)
        _put(wo, full, Z)
        _put(P, full, (0.0, 0.0, 0.0))
        for q, v in (("sheen_weight", 0.5), ("specular_weight", 0.6), ("sheen_roughness", 0.1), ("specular_roughness", 0.1),
                     ("sheen_color", (0.9, 0.8, 0.7)), ("specular_color", (0.7, 0.8, 0.9)), ("sheen_ior", 1.5), ("specular_ior", 1.5),
                     ("sss_weight", 0.8)):
            _put(p[q], full, v)
        for q in ("sheen_weight", "specular_weight", "sss_weight"):
            _put(p[q], dead, 0.0)
        for r, q, v in ((2, "sheen_weight", 0.0), (3, "sheen_weight", 1e-4), (10, "specular_weight", 0.0), (5, "specular_weight", 1e-4),
                        (6, "sheen_color", (0.0, 0.0, 0.0)), (7, "specular_color", (0.0, 0.0, 0.0)), (8, "sss_weight", 0.0),
                        (9, "sss_weight", 5e-5)):                   # the gates of tests/test_gpu_trace_skin.py, _gated
            _put(p[q], k == r, v)
        c = dict(wo=wo, N=np.tile(Z[:, None], (1, m)), T=np.tile(X[:, None], (1, m)), P=P, params=p)
    _CASES[key] = c
    return c


# ---- the flavours behind one interface ---------------------------------------------------------------------------------------
class Flavour:
    """n points of one flavour on one context: c the host case of the points.
    emit -> the binding's queue object(s) E; members(E) -> {name: queue}; sides(E) -> {name: per-point plane};
    unit(E) -> the resolve under visibility 1, radiance 1 and the probes traced through the analytic plane {AOV: numpy};
    analytic -> reference 1 in the same keys; planes(E, seed) / resolve(E, planes) -> a resolve under random visibility and
    radiance; full(name) -> the slot count of a point in queue `name`"""

    def __init__(self, T, ctx, oracle, fl, c):
        self.T, self.ctx, self.oracle, self.fl, self.c = T, ctx, oracle, fl, c
        self.kind, self.node = fl.split("-") if "-" in fl else ("skin", "skin")
        n = self.n = c["P"].shape[1]
        if self.kind == "lights":
            self.b = Batch(T, ctx, self.node, n, c=dict(c))
        elif self.node == "ggx":
            self.b = TS.Node(T, ctx, oracle, "ggx", n, case=dict(
                P=c["P"], c={q: c[q] for q in ("wo", "N", "T", "KsColor", "roughness", "ior", "anisotropic")},
                shh=dict(KdColor=c["kdc"], Kd=c["kd"], diffuseRoughness=c["kdr"], Ks=c["ks"], KtColor=c["ktc"], Kt=c["kt"])))
        elif self.node == "disney":
            self.b = TS.Node(T, ctx, oracle, "disney", n, case=dict(P=c["P"], c={q: v for q, v in c.items() if q != "P"}))
        else:
            self.b = TK.Skin(ctx, oracle, n, "plane", case=c)

    def emit(self, lights, spp_n, first=0, traced=True, share=False, queues=None):
        if self.kind == "lights":
            return self.b.emit(lights, spp_n, SEED, first, queue=queues)
        if self.kind == "node":
            return self.b.emit(lights, spp_n, SEED, first, traced=traced, queues=queues, share=share)
        return self.b.emit(self.T, lights, spp_n, SEED, first, queues=queues, share=share)

    def new_queues(self, nl, spp_n, share=False):
        T, ctx, n = self.T, self.ctx, self.n
        if self.kind == "lights":
            return T.ShadowQueue(ctx, n, nl, spp_n, disney=self.node == "disney")
        cls = T.SkinNodeQueues if self.kind == "skin" else T.GgxNodeQueues if self.node == "ggx" else T.DisneyNodeQueues
        return cls(ctx, n, nl, spp_n, share)

    def members(self, E):
        if self.kind == "lights":
            return {"shadow": E}
        if self.kind == "node":
            return dict([("shadow", E.shadow)] + [(r, getattr(E, r)) for r in E.RAYS])
        return {r: getattr(E, r) for r in E.SHADOWS + E.RAYS + ("probes",)}

    def sides(self, E):
        return {r: getattr(E, r) for r in ("sheenFresnel", "specularFresnel", "sssWeight")} if self.kind == "skin" else {}

    def full(self, name, nl, spp, traced=True):
        if name == "probes":
            return None                                             # dense: spp rays a point, by construction
        if "shadow" in name:
            return nl * (2 if self.kind == "skin" else 3) * spp
        return 1 if name == "refract" and not traced else spp

    def analytic(self, lights, spp_n, first=0, traced=True):
        if self.kind == "lights":
            return dict(zip(("direct_diffuse", "direct_specular"), self.b.analytic(lights, spp_n, SEED, first)))
        if self.kind == "node":
            return self.b.analytic(lights, spp_n, SEED, first, traced=traced)
        return self.b.analytic(lights, spp_n, SEED, first)

    def oracle_ref(self, lo, spp_n, first=0, traced=True):
        """reference 2: the oracle's two-sums batch function on these points"""
        o, c = self.oracle, self.c
        if self.kind == "node":
            return self.b.oracle_shade(o, lo, spp_n, SEED, first, traced)
        if self.kind == "skin":
            return o.skin_integrate(c["wo"], c["N"], c["T"], c["params"], c["P"], self.b.oscene, spp_n, SEED, env=(1.0, 1.0, 1.0),
                                    first_index=first, nthreads=min(16, o.hardware_threads()), lights=lo)
        if self.node == "ggx":
            ref = ggx_oracle(o, c).direct_lighting(c["P"], lo, spp_n, SEED, Kd_color=c["kdc"], Kd=c["kd"], Kd_roughness=c["kdr"],
                                                   Ks=c["ks"], first_index=first)
        else:
            ref = disney_oracle(o, c).direct_lighting(c["P"], lo, spp_n, SEED, first_index=first)
        return dict(zip(("direct_diffuse", "direct_specular"), ref))

    def unit_planes(self, E):
        ctx = self.ctx
        if self.kind == "lights":
            return [torch.ones(3, max(E.count, 1), dtype=torch.float32, device=ctx.torch_device)]
        if self.kind == "node":
            return TS._unit(ctx, E)
        return list(TK._traced(ctx, E, (1.0, 1.0, 1.0))) + [dev(h) for h in self.b.hits(E)]

    def planes(self, E, seed):
        """random visibility and radiance, device planes in the resolve's order: the functional files' distributions (a
        visibility with zeros and ones; radiance over eight decades)"""
        if self.kind == "lights":
            return [dev(_visibility(E.count, seed))]
        if self.kind == "node":
            return [p.cuda() for p in TS._random_planes(E, seed, hdr=True)]
        cnt = E.counts()
        rng = np.random.default_rng(seed)
        vis = [dev(rng.random((3, max(cnt[k], 1))).astype(F)) for k in E.SHADOWS]
        rad = [dev((rng.random((3, max(cnt[k], 1))) * 10.0 ** rng.uniform(-4, 4, (3, max(cnt[k], 1)))).astype(F)) for k in E.RAYS]
        hc, hP, hN, Eh = self.b.hits(E)
        return vis + rad + [dev(hc), dev(hP), dev(hN), dev((Eh * rng.random(Eh.shape).astype(F)).astype(F))]

    def resolve(self, E, planes, out=None):
        if self.kind == "lights":
            got = E.resolve(planes[0], out=None if out is None else (out["direct_diffuse"], out["direct_specular"]))
            return {"direct_diffuse": host(got[0]), "direct_specular": host(got[1])}
        return {q: host(v) for q, v in E.resolve(*planes, out=out).items()}

    def aov_shapes(self):
        n = self.n
        if self.kind == "lights":
            return {"direct_diffuse": (3, n), "direct_specular": (3, n)}
        if self.kind == "node":
            return {q: (3, n) for q in self.b.s.SHADE_AOVS + ("out",)}
        return dict([(q, (3, n)) for q in ("sheen", "specular", "sss", "out")] +
                    [(q, (n,)) for q in ("sheenFresnel", "specularFresnel", "sssWeight")])


def make(T, ctx, oracle, fl, n, a=0, full=None, case=None):
    """points [a, a + n) of the flavour's `full` points (or of `case`)"""
    c = _host_case(fl, oracle, n if full is None else full) if case is None else case
    return Flavour(T, ctx, oracle, fl, _sl(c, a, a + n))


# ---- queues on the device ----------------------------------------------------------------------------------------------------
def _count(q):
    return q.count if hasattr(q, "origin") else int(q.offsets[q.n].item())


def _rows(q):
    """the planes of a queue, rays along the last axis"""
    if hasattr(q, "origin"):
        return dict(origin=q.origin, dir=q.dir, maxdist=q.maxdist, point=q.point, sample=q.sample)
    d = dict(dir=q._dir, point=q._point, sample=q._sample)
    if hasattr(q, "_ws"):
        d.update(maxdist=q._maxdist, ws=q._ws, wd=q._wd, kind=q._kind)
    else:
        d.update(weight=q._weight)
        if q._kind is not None:
            d["kind"] = q._kind
    return d


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _dev_same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum().item()), "words differ of", a.numel())


def _same_queue(qa, qb, what, a=0, b=None, shift=0):
    """qb is qa over the points [a, b): offsets, every plane up to offsets[n], point shifted by `shift`"""
    b = qa.n if b is None else b
    off = qa.offsets[a:b + 1]
    lo, hi = int(off[0].item()), int(off[-1].item())
    assert torch.equal(off - lo, qb.offsets.to(off.device)), (what, "offsets")
    assert _count(qb) == hi - lo, (what, "count")
    ra, rb = _rows(qa), _rows(qb)
    assert set(ra) == set(rb)
    for k in ra:
        x, y = ra[k][..., lo:hi], rb[k][..., :hi - lo].to(ra[k].device)
        _dev_same(x - shift if k == "point" else x, y, (what, k))


def _same_emit(fa, Ea, fb, Eb, what):
    ma, mb = fa.members(Ea), fb.members(Eb)
    assert set(ma) == set(mb)
    for r in ma:
        _same_queue(ma[r], mb[r], (what, r))
    for r, t in fa.sides(Ea).items():
        _dev_same(t, fb.sides(Eb)[r].to(t.device), (what, r))


def _counts(f, E):
    return {r: np.diff(host(q.offsets).astype(np.int64)) for r, q in f.members(E).items()}


def _assert_extremes(f, counts, nl, spp, traced=True, what=""):
    """no constant-count batch: in every compacted queue a point without rays and a point with a ray in every slot"""
    for r, cnt in counts.items():
        full = f.full(r, nl, spp, traced)
        if full is None:
            assert (cnt == spp).all(), (what, r)
            continue
        assert cnt.min() == 0 and cnt.max() == full, (what, r, "counts from", int(cnt.min()), "to", int(cnt.max()), "slots", full)


def _same_aovs(got, want, what, cols=slice(None)):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for q in want:
        U.same_bits_or_both_nan(got[q][..., cols], want[q], (what, q))


def _tight(got, ref, what, cols=slice(None)):
    for q in ref:
        cases.assert_tight(cases.summarize(cases.rel_err(got[q][..., cols], ref[q])), (what, q))


def _math_mode(ctxs, fast):
    for c in ctxs:
        c.set_math_mode(fast)


# ---- A. several grid rounds --------------------------------------------------------------------------------------------------
def _window_planes(f, E, planes, a, b):
    """the random planes of the rays of points [a, b): per compacted queue the columns offsets[a] .. offsets[b]; rlSkin's probe
    hits the dense columns a spp .. b spp"""
    names = [r for r in f.members(E) if r != "probes"]
    out = []
    for r, p in zip(names, planes):
        off = f.members(E)[r].offsets
        lo, hi = int(off[a].item()), int(off[b].item())
        out.append(p[:, lo:max(hi, lo + 1)].contiguous())
    if f.kind == "skin":
        spp = E.spp_n * E.spp_n
        out += [p[..., a * spp:b * spp].contiguous() for p in planes[len(names):]]
    return out


def _window_against_the_references(fw, Ew, planes, got, lights, spp_n, first, what):
    """a window's own emit Ew (bit-equal to the batch's queue over the window) and the batch's resolve `got` over it: reference
    3, the documented float32 composition and the float64 bound of the functional files; reference 2, the per-sample queue
    oracles (the light loops': the BSDF-strategy directions, the only per-sample oracle they have)"""
    spp, nl = spp_n * spp_n, len(lights)
    if fw.kind == "lights":
        h, vis, rad = queue_host(Ew), host(planes[0]), _rad(lights)
        g2 = (got["direct_diffuse"], got["direct_specular"])
        want = compose(h, vis, rad, spp, tail=fw.b.tail())
        for k in range(2):
            cases.assert_same_bits(g2[k], want[k], (what, k, "documented composition"))
        assert_float64_bound(h, vis, rad, spp, g2, fw.b.tail(), what)
        checked = bsdf_directions_against_the_oracle(fw.oracle, fw.node, fw.b.c, h, nl, spp_n, SEED, first)
        assert sum(checked.values()) > 0, (what, checked)
    elif fw.kind == "node":
        cpu = [p.cpu() for p in planes]
        _same_aovs(got, TS._compose_node(fw.b, Ew, cpu, lights, spp_n, True, np.float32)[0], (what, "documented composition"))
        TS._assert_within_the_float64_bound(fw.b, Ew, cpu, lights, spp_n, True, got, what)
        if fw.node == "ggx":
            TS._assert_ggx_queues_are_the_oracle_samplers(fw.oracle, fw.b, Ew, spp_n, first, SEED)
        else:
            TS._assert_disney_queues_are_the_oracle_samplers(fw.oracle, fw.b, Ew, spp_n, first, SEED)
    else:
        vis = {k: host(p) for k, p in zip(Ew.SHADOWS, planes[:2])}
        rad = {k: host(p) for k, p in zip(Ew.RAYS, planes[2:4])}
        specs = [dict(radiance=RADS[l]) for l in range(nl)]
        TK._documented_composition(fw.b, Ew, specs, spp_n, vis, rad, tuple(host(p) for p in planes[4:]), got)
        TK._assert_glossy_queues_are_the_oracle_sampler(fw.oracle, fw.b, Ew, spp_n, first, SEED)


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("fl", FLAVOURS)
def test_many_points_take_several_grid_rounds(gpu, oracle, T, one_block_per_cu, fl, fast):
    """A1.  One workgroup per CU: a round of the resolves' and emits' loops covers compute_units x kBlock points (the emits at
    G = 64 four of them), of shadow_compact_kernel compute_units tiles; n gives two and a half rounds and a ragged tail.
    Every queue and side plane and both resolves carry the default context's bits, the unit resolve the analytic call's;
    EXACT: windows of 141 points across the round boundaries and at the tail are their own chunked emit, resolve to the same
    bits, to the documented composition and within its float64 bound, and match the per-sample queue oracles and the oracle's
    two-sums batch function (_window_against_the_references)"""
    ctx = one_block_per_cu
    rnd = ctx.device_info()["compute_units"] * KBLOCK
    n, spp_n, nl = 2 * rnd + rnd // 2 + 37, 2, 2
    lo, lights = _sat_lights(oracle, nl)
    _math_mode((gpu, ctx), fast)
    try:
        f1, f0 = make(T, ctx, oracle, fl, n), make(T, gpu, oracle, fl, n)
        for g in (1, 64):
            E1 = _with_group(g, lambda: f1.emit(lights, spp_n, FIRST))
            E0 = _with_group(g, lambda: f0.emit(lights, spp_n, FIRST))
            _same_emit(f1, E1, f0, E0, (fl, g, "emit vs the default context"))
            if g == 1:
                _assert_extremes(f1, _counts(f1, E1), nl, spp_n * spp_n, what=fl)
            unit = f1.resolve(E1, f1.unit_planes(E1))
            _same_aovs(unit, _with_group(g, lambda: f0.analytic(lights, spp_n, FIRST)), (fl, g, "unit resolve vs the analytic call"))
            planes = f0.planes(E0, seed=5)
            got = f1.resolve(E1, planes)
            _same_aovs(got, f0.resolve(E0, planes), (fl, g, "random resolve vs the default context"))
        if fast:
            return
        for a in (rnd - 70, 2 * rnd - 70, n - 141):
            b = a + 141
            fw = make(T, gpu, oracle, fl, 141, a=a, full=n)
            Ew = _with_group(1, lambda: fw.emit(lights, spp_n, FIRST + a))
            for r, q in f1.members(E1).items():
                _same_queue(q, fw.members(Ew)[r], (fl, a, r, "window"), a, b, shift=a)
            pw = _window_planes(f1, E1, planes, a, b)
            gw = fw.resolve(Ew, pw)
            _same_aovs(got, gw, (fl, a, "random resolve of the window"), slice(a, b))
            _window_against_the_references(fw, Ew, pw, {q: v[..., a:b] for q, v in got.items()}, lights, spp_n, FIRST + a, (fl, a))
            _tight(unit, fw.oracle_ref(lo, spp_n, FIRST + a), (fl, a, "oracle"), slice(a, b))
    finally:
        _math_mode((gpu, ctx), False)


@pytest.mark.parametrize("fl,traced", [(f, True) for f in FLAVOURS] + [("node-ggx", False)])
def test_one_point_compaction_tiles_take_several_grid_rounds(gpu, oracle, T, one_block_per_cu, fl, traced):
    """A2.  8 lights at spp_n = 16: kShadowMaxSlots = 6144 slots a point (4096 for a lobe of rlSkin), tile_points == 1, and more
    tiles than the capped grid has workgroups: shadow_compact_kernel's slot walk with pc == 1 (dsp = kBlock, dp = 0) in its
    second and third round; the ray queues' tiles hold kCompactSlots / 256 = 16 points"""
    ctx = one_block_per_cu
    cu = ctx.device_info()["compute_units"]
    n, spp_n, nl = 2 * cu + cu // 2 + 3, 16, 8
    _, lights = _sat_lights(oracle, nl)
    f1, f0 = make(T, ctx, oracle, fl, n), make(T, gpu, oracle, fl, n)
    for g in (1, None):
        E1 = _with_group(g, lambda: f1.emit(lights, spp_n, FIRST, traced=traced))
        E0 = _with_group(g, lambda: f0.emit(lights, spp_n, FIRST, traced=traced))
        _same_emit(f1, E1, f0, E0, (fl, g, traced, "emit vs the default context"))
        if g == 1:
            _assert_extremes(f1, _counts(f1, E1), nl, spp_n * spp_n, traced, what=fl)
        _same_aovs(f1.resolve(E1, f1.unit_planes(E1)), _with_group(g, lambda: f0.analytic(lights, spp_n, FIRST, traced)),
                   (fl, g, traced, "unit resolve vs the analytic call"))


# ---- B. scan-tile and compaction-tile edges ----------------------------------------------------------------------------------
CHUNK = 700        # no multiple of it below 3 kScanTile + 5 is a multiple of a scan (2048), compaction or resolve tile's points


@pytest.mark.parametrize("n", [KSCAN - 1, KSCAN, KSCAN + 1, 3 * KSCAN + 5])
@pytest.mark.parametrize("fl", FLAVOURS)
def test_scan_and_compaction_tile_edges(gpu, oracle, T, fl, n):
    """B.  One, two and four scan tiles, the last one of 1 and of 5 points; spp_n = 3: compaction tiles of 256 points (9
    slots) and of 6144 / 27 = 227 (lights) or 6144 / 36 = 170 (rlSkin, two lights) points, the last one partial.  The queue is
    the concatenation of the queues of chunks of 700 points, offsets their host int64 cumsum; the unit resolve the analytic
    call"""
    nl = 2 if fl == "skin" else 1
    _, lights = _sat_lights(oracle, nl)
    f = make(T, gpu, oracle, fl, n)
    chunks = [(a, min(a + CHUNK, n)) for a in range(0, n, CHUNK)]
    cf = [(a, b, make(T, gpu, oracle, fl, b - a, a=a, full=n)) for a, b in chunks]
    for fast in (False, True):
        _math_mode((gpu,), fast)
        try:
            for spp_n in (2, 3):
                E = f.emit(lights, spp_n, FIRST)
                parts = [(a, b, fc, fc.emit(lights, spp_n, FIRST + a)) for a, b, fc in cf]
                what = (fl, n, spp_n, fast)
                for r, q in f.members(E).items():
                    cnt = np.concatenate([np.diff(host(fc.members(Ec)[r].offsets).astype(np.int64)) for _, _, fc, Ec in parts])
                    np.testing.assert_array_equal(host(q.offsets), np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)]), str((what, r)))
                    for a, b, fc, Ec in parts:
                        _same_queue(q, fc.members(Ec)[r], (what, r, a), a, b, shift=a)
                for r, t in f.sides(E).items():
                    _dev_same(t, torch.cat([fc.sides(Ec)[r] for _, _, fc, Ec in parts]), (what, r))
                _assert_extremes(f, _counts(f, E), nl, spp_n * spp_n, what=what)
                _same_aovs(f.resolve(E, f.unit_planes(E)), f.analytic(lights, spp_n, FIRST), (what, "unit resolve vs the analytic call"))
        finally:
            _math_mode((gpu,), False)


# ---- C. nothing is written outside what the caller handed over ----------------------------------------------------------------
PAD = 67                                     # words on each side of every row (tests/test_gpu_loop_edges.py)
SCRATCH_PAD = PAD * 256                      # bytes beside a scratch block: it stays 256-byte aligned, as a device allocation is


class Padded:
    """tensors whose rows are views inside larger buffers filled with SENTINEL"""

    def __init__(self):
        self.bufs = []

    def like(self, t, pad_bytes=None):
        if t.numel() == 0:
            return t
        item, w = t.element_size(), t.shape[-1]
        pad_bytes = PAD * max(item, 4) if pad_bytes is None else pad_bytes
        body = (w * item + 7) // 8 * 8
        buf = torch.full(tuple(t.shape[:-1]) + ((2 * pad_bytes + body) // 4,), SENTINEL, dtype=torch.int32, device=t.device)
        self.bufs.append((buf, pad_bytes, pad_bytes + w * item))
        return buf.view(torch.uint8)[..., pad_bytes:pad_bytes + w * item].view(t.dtype)

    def empty(self, shape, device):
        return self.like(torch.empty(shape, dtype=torch.float32, device=device))

    def check(self, what):
        for k, (buf, lo, hi) in enumerate(self.bufs):
            clean = torch.full_like(buf, SENTINEL).view(torch.uint8)
            got = buf.view(torch.uint8)
            assert torch.equal(got[..., :lo], clean[..., :lo]), (what, "buffer", k, tuple(buf.shape), "words before the view")
            assert torch.equal(got[..., hi:], clean[..., hi:]), (what, "buffer", k, tuple(buf.shape), "words after the view")


def _rehouse(T, q, pad, scratch=None):
    """move a queue of the binding into padded buffers: every plane, the offsets, the side plane, its scratch of exactly the
    size the binding asked the library for (or the shared block `scratch`); the C struct follows"""
    capi, c = T.capi, q.q
    q.offsets = pad.like(q.offsets)
    c.offsets = q.offsets.data_ptr()
    v3 = lambda t: capi.Vec3(*[t[k].data_ptr() for k in range(3)])
    if hasattr(q, "origin"):
        q.origin, q.dir, q.maxdist, q.point, q.sample = (pad.like(t) for t in (q.origin, q.dir, q.maxdist, q.point, q.sample))
        c.origin, c.dir = v3(q.origin), v3(q.dir)
        c.maxdist, c.point, c.sample = q.maxdist.data_ptr(), q.point.data_ptr(), q.sample.data_ptr()
        return
    q._dir, q._point, q._sample = pad.like(q._dir), pad.like(q._point), pad.like(q._sample)
    c.dir, c.point, c.sample = v3(q._dir), q._point.data_ptr(), q._sample.data_ptr()
    if hasattr(q, "_ws"):
        q._maxdist, q._ws, q._wd, q._kind = pad.like(q._maxdist), pad.like(q._ws), pad.like(q._wd), pad.like(q._kind)
        wd = q._wd
        c.maxdist, c.kind = q._maxdist.data_ptr(), q._kind.data_ptr()
        c.weight_specular = capi.Rgb(*[q._ws[k].data_ptr() for k in range(3)])
        c.weight_diffuse = capi.Rgb(*[wd[k].data_ptr() if k < wd.shape[0] else None for k in range(3)])
    else:
        q._weight, q.side = pad.like(q._weight), pad.like(q.side)
        w = q._weight
        c.weight = capi.Rgb(*[w[k].data_ptr() if k < w.shape[0] else None for k in range(3)])
        if q._kind is not None:
            q._kind = pad.like(q._kind)
            c.kind = q._kind.data_ptr()
    q._scratch = pad.like(q._scratch, SCRATCH_PAD) if scratch is None else scratch
    c.scratch, c.scratch_bytes = q._scratch.data_ptr(), q._scratch.numel()


def _padded_queues(T, f, nl, spp_n, share, pad):
    E = f.new_queues(nl, spp_n, share)
    shared = None
    if share:
        assert E.scratch.numel() == T.node_scratch_bytes(f.n, nl, spp_n)
        shared = E.scratch = pad.like(E.scratch, SCRATCH_PAD)
    for r, q in f.members(E).items():
        if r != "probes" and not share:
            want = T.shadow_scratch_bytes(f.n, nl, spp_n) if "shadow" in r else T.scratch_bytes(f.n, spp_n)
            assert q._scratch.numel() == want, (r, q._scratch.numel(), want)
        assert q.capacity == f.n * (f.full(r, nl, spp_n * spp_n) or spp_n * spp_n), (r, q.capacity)
        _rehouse(T, q, pad, shared)
    if f.kind == "skin":
        E.sheenFresnel, E.specularFresnel, E.sssWeight = (pad.like(t) for t in (E.sheenFresnel, E.specularFresnel, E.sssWeight))
    return E


@pytest.mark.parametrize("n,nl,spp_n", [(1001, 2, 3), (5, 8, 16)], ids=["1001", "slot_maximum"])
@pytest.mark.parametrize("fl", FLAVOURS)
def test_nothing_is_written_outside_what_the_caller_handed_over(gpu, oracle, T, fl, n, nl, spp_n):
    """C.  Queues of the documented minimum capacity and scratch of exactly rls_trace_scratch_bytes / rls_trace_shadow_scratch_bytes
    (or, the nodes' shared mode, one block of the largest of them for all queues of the emit), every plane 67 words inside a
    buffer of 0x7FC0DEAD: after emit and resolve every word beside a view still holds the sentinel (compared on the device),
    and the views hold the bits of the plain call"""
    _, lights = _sat_lights(oracle, nl)
    f = make(T, gpu, oracle, fl, n)
    for g in (1, 64):
        plain = _with_group(g, lambda: f.emit(lights, spp_n, FIRST))
        if g == 1:
            _assert_extremes(f, _counts(f, plain), nl, spp_n * spp_n, what=fl)
        planes = f.planes(plain, seed=n)
        want = f.resolve(plain, planes)
        for share in ((False,) if f.kind == "lights" else (False, True)):
            pad = Padded()
            E = _padded_queues(T, f, nl, spp_n, share, pad)
            out = {q: pad.empty(s, gpu.torch_device) for q, s in f.aov_shapes().items()}
            E = _with_group(g, lambda: f.emit(lights, spp_n, FIRST, share=share, queues=E))
            got = f.resolve(E, planes, out=out)
            torch.cuda.synchronize()
            pad.check((fl, n, g, share))
            _same_emit(f, plain, f, E, (fl, n, g, share, "in padded buffers"))
            _same_aovs(got, want, (fl, n, g, share, "in padded buffers"))


# ---- D. hostile per-point inputs ---------------------------------------------------------------------------------------------
def _poison_case(c, rng, n, frac=0.02):
    """2 % of the words of every plane replaced by SPECIAL -> (the case, the points with a replaced word)"""
    dirty = np.zeros(n, bool)

    def walk(v):
        if isinstance(v, dict):
            return {k: walk(x) for k, x in v.items()}
        a = np.array(v, F)
        flat = a.reshape(-1)
        k = rng.choice(flat.size, max(1, int(frac * flat.size)), replace=False)
        flat[k] = SPECIAL[rng.integers(0, SPECIAL.size, k.size)]
        dirty[k % n] = True
        return a

    return walk(c), dirty


def _kinds(T, r, nl):
    """the documented bytes of queue r's kind plane: a light-strategy ray of light l carries one or both lobes, a BSDF-strategy
    ray exactly one (rlSkin: the specular lobe alone); a refraction ray is transmitted or the mirror of a total reflection"""
    if "shadow" not in r:
        return [T.RLS_RAY_TRANSMITTED, T.RLS_RAY_TIR_MIRROR]
    S, D, B = T.RLS_SHADOW_SPECULAR, T.RLS_SHADOW_DIFFUSE, T.RLS_SHADOW_BSDF
    lobes = (S, B | S) if r != "shadow" else (S, D, S | D, B | S, B | D)
    return [l | k for l in range(nl) for k in lobes]


def _hash01(key, salt):
    """a float64 in [0, 1) per integer key (splitmix64's finaliser)"""
    x = (key.astype(np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return (x >> np.uint64(11)).astype(np.float64) / 2.0 ** 53


def _keyed_planes(f, E):
    """the resolve's planes as functions of (queue, point, sample, kind, channel), not of the ray index: a visibility in [0, 1]
    with zeros and ones per shadow ray, a radiance over eight decades per sample ray; rlSkin's hits are the run's own (the probe
    queue is dense), their irradiance scaled per (ray, hit, channel)"""
    planes = []
    for qi, (r, q) in enumerate(f.members(E).items()):
        if r == "probes":
            continue
        cnt = _count(q)
        rows = {k: host(v[..., :cnt]).astype(np.int64) for k, v in _rows(q).items() if k in ("point", "sample", "kind")}
        key = ((rows["point"] * 256 + rows["sample"]) * 256 + rows.get("kind", 0)) * 8 + qi
        p = np.zeros((3, max(cnt, 1)), F)
        for c in range(3):
            u = _hash01(key, 1000 + c)
            if "shadow" in r:
                u = np.where(u < 0.2, 0.0, np.where(u > 0.8, 1.0, u))
            else:
                u = u * 10.0 ** (8.0 * _hash01(key, 2000 + c) - 4.0)
            p[c, :cnt] = u
        planes.append(dev(p))
    if f.kind == "skin":
        hc, hP, hN, Eh = f.b.hits(E)
        j = np.arange(Eh.shape[1])[None, :, None] * (1 << 40) + np.arange(Eh.shape[2])[None, None, :] * 4 + np.arange(3)[:, None, None]
        planes += [dev(hc), dev(hP), dev(hN), dev((Eh * _hash01(j.reshape(-1), 3000).reshape(Eh.shape)).astype(F))]
    return planes


@pytest.mark.parametrize("fl", FLAVOURS)
def test_hostile_per_point_inputs(gpu, oracle, T, fl):
    """D.  NaN, infinities, signed zeros, denormals, +-3e38 in wo, N, T, P and every closure and shader parameter plane (the
    lights stay finite: copy_lights refuses others on the host).  The emit succeeds; every queue is a valid CSR queue within its
    capacity; a point none of whose inputs was touched has the rays of the clean run, bit for bit, and the clean run's resolve
    under a visibility and radiance keyed by (point, sample, kind); the unit resolve is the analytic call on the same inputs (the
    same NaN pattern, the same bits elsewhere)"""
    n, spp_n, nl = KSCAN + 1, 3, 2
    spp = spp_n * spp_n
    _, lights = _sat_lights(oracle, nl)
    clean = make(T, gpu, oracle, fl, n)
    bad_case, dirty = _poison_case(clean.c, np.random.default_rng(31 + FLAVOURS.index(fl)), n)
    bad = make(T, gpu, oracle, fl, n, case=bad_case)
    assert dirty.any() and (~dirty).sum() > n // 4
    for g in (1, 64):
        Ec = _with_group(g, lambda: clean.emit(lights, spp_n, FIRST))
        Eb = _with_group(g, lambda: bad.emit(lights, spp_n, FIRST))                  # RLS_OK, or the binding raises
        for r, q in bad.members(Eb).items():
            what = (fl, g, r)
            off = host(q.offsets).astype(np.int64)
            cnt = np.diff(off)
            full = bad.full(r, nl, spp)
            assert off[0] == 0 and (cnt >= 0).all() and (cnt <= (full or spp)).all() and off[n] <= q.capacity, what
            rows = {k: host(v[..., :off[n]]) for k, v in _rows(q).items()}
            np.testing.assert_array_equal(rows["point"].astype(np.int64), np.repeat(np.arange(n), cnt), str(what))
            assert (rows["sample"] < spp).all(), what
            if "kind" in rows:
                assert np.isin(rows["kind"], _kinds(T, r, nl)).all(), (what, np.unique(rows["kind"]))
            qc = clean.members(Ec)[r]
            offc = host(qc.offsets).astype(np.int64)
            keep = ~dirty
            np.testing.assert_array_equal(cnt[keep], np.diff(offc)[keep], str(what))
            rc = {k: host(v[..., :offc[n]]) for k, v in _rows(qc).items()}
            mb, mc = np.repeat(keep, cnt), np.repeat(keep, np.diff(offc))
            for k in rows:
                if k != "point":
                    x, y = np.ascontiguousarray(rows[k][..., mb]), np.ascontiguousarray(rc[k][..., mc])
                    assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, k, "rays of the untouched points")
        for r, t in bad.sides(Eb).items():
            U.same_bits_or_both_nan(host(t)[~dirty], host(clean.sides(Ec)[r])[~dirty], (fl, g, r, "untouched points"))
        # a visibility / radiance per (point, sample, kind) in both queues (the ray indices differ after the first poisoned
        # point): no clean point's resolve changes with respect to the clean run's, whatever its neighbours in the tile carry
        rc, rb = clean.resolve(Ec, _keyed_planes(clean, Ec)), bad.resolve(Eb, _keyed_planes(bad, Eb))
        for q in rc:
            cases.assert_same_bits(rb[q][..., ~dirty], rc[q][..., ~dirty], (fl, g, q, "keyed resolve of the untouched points"))
        got = bad.resolve(Eb, bad.unit_planes(Eb))
        ref = _with_group(g, lambda: bad.analytic(lights, spp_n, FIRST))
        for q in ref:
            _same_nan(got[q], ref[q], (fl, g, q, "unit resolve vs the analytic call on the poisoned inputs"))
