"""GPU: the caller-traced whole nodes (include/rlshaders_amd_trace.h, rls_trace_ggx_shade_* / rls_trace_disney_shade_*;
rlshaders_amd/trace.py, ggx_node_rays / disney_node_rays).

The node emit fills one queue per loop of rls_ggx_shade / rls_disney_shade; one resolve composes the AOVs.  Checked here:
  1. the contract: visibility 1 and radiance 1 give rls_*_shade(env = 1) bit for bit -- every AOV and out, EXACT and FAST,
     traced 0 and 1, any lane-group width, 0 / 1 / 2 / 8 lights, uniform parameters and parameters by reference, one shared
     scratch block;
  2. the queues are the NODE's samples (stream pairs 24, 25, 26), composed on the CPU from the oracle's samplers, and are not
     the stand-alone integrators' (pairs 0, 1); the shadow member is trace.ggx_shadow_rays' queue plane for plane.  The
     pair-26 queue: the oracle's cosine-weighted sampler and orc_oren_nayar_brdf / _pdf, ray by ray;
  3. the node's gates (the k = i % 8 pattern of tests/test_gpu_shade.py);
  4. non-unit radiance: a uniform radiance env gives the oracle's shade(env) within cases.assert_tight (and rls_*_shade(env)
     bit for bit); per-ray radiance and coloured visibility against the documented composition in numpy float32 (bits) and
     float64 (a rounding bound);
  5. robustness: non-finite radiance, first_index past 2^32, chunks, graph replay, argument checks on the device path.
Inputs are tests/test_gpu_shade.py's: cases.ggx_mixed / disney_mixed, the slab, its two lights."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import cases
import rlshaders_amd as R
from gpu_util import dev, disney_oracle, disney_sampler, ggx_oracle, ggx_sampler, host
from test_gpu_loop_edges import LIGHTS as LIGHTS8
from test_gpu_shade import LIGHTS, _lights, _slab
from trace_lights_util import compose, queue_host
from trace_util import DIFFUSE, EPS, GLOSSY, _queue, sequential

pytestmark = pytest.mark.gpu

SEED = 41
NODES = ("ggx", "disney")
ROOT = Path(__file__).resolve().parent.parent
KBLOCK = int(re.search(r"#define RLS_BLOCK (\d+)", (ROOT / "rlshaders_amd" / "csrc" / "rls_internal.hpp").read_text()).group(1))
PAIR0 = 24                             # the node's first stream pair after the lights' (3 * RLS_MAX_LIGHTS)
GGX_RAYS = ("glossy", "refract", "diffuse")
DISNEY_RAYS = ("diffuse", "specular")


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


class Node:
    """one node over the first n points of tests/test_gpu_shade.py's inputs: the closure, the slab, rlGgx's node parameters
    with Kd = 0, Kt = 0 and a black KsColor on the residues 0, 1, 2 of i % 8"""

    def __init__(self, T, ctx, oracle, node, n, a=0, full=None, case=None):
        """case: the caller's own points instead -- dict(P [3, n], c the closure's planes, shh rlGgx's node parameters), numpy"""
        self.T, self.ctx, self.node, self.n = T, ctx, node, n
        m = max(a + n, 128) if full is None else full
        sl = lambda v: np.ascontiguousarray(v[..., a:a + n])
        self.k = np.arange(a, a + n) % 8
        if case is not None:
            self.Ph, self.c, self.shh = case["P"], case["c"], case.get("shh")
        elif node == "ggx":
            c = cases.ggx_mixed(cases.SEED_PARITY, m)
            u = lambda j: oracle.gen_uniform(cases.SEED_PARITY, 0, m, oracle.S_PARAM0 + j, 0.0, 1.0)
            kdc, ktc = np.stack([u(j) for j in range(3)]), np.stack([u(3 + j) for j in range(3)])
            kd, kdr, ks, kt = u(6), u(7), u(8), u(9)
            k = np.arange(m) % 8
            kd = np.where(k == 0, np.float32(0.0), kd).astype(np.float32)
            kt = np.where(k == 1, np.float32(0.0), kt).astype(np.float32)
            c = dict(c, KsColor=np.where((k == 2)[None, :], np.float32(0.0), c["KsColor"]).astype(np.float32))
            self.c = {q: sl(v) for q, v in c.items()}
            self.shh = dict(KdColor=sl(kdc), Kd=sl(kd), diffuseRoughness=sl(kdr), Ks=sl(ks), KtColor=sl(ktc), Kt=sl(kt))
            self.Ph = sl(_slab(m))
        else:
            self.c = {q: sl(v) for q, v in cases.disney_mixed(cases.SEED_PARITY, m).items()}
            self.shh = None
            self.Ph = sl(_slab(m))
        self.P = dev(self.Ph)
        if node == "ggx":
            self.sh = {q: dev(v) for q, v in self.shh.items()}
            self.s = ggx_sampler(ctx, self.c)
        else:
            self.s = disney_sampler(ctx, self.c)
            self.sh = self.shh = None
        self.rays = GGX_RAYS if node == "ggx" else DISNEY_RAYS

    def analytic(self, lights, spp_n, seed=SEED, first=0, traced=True, env=(1.0, 1.0, 1.0)):
        if self.node == "ggx":
            out = self.s.shade(self.P, lights, spp_n, seed, env=env, traced=traced, first_index=first, **self.sh)
        else:
            out = self.s.shade(self.P, lights, spp_n, seed, env=env, first_index=first)
        return {q: host(v) for q, v in out.items()}

    def oracle_shade(self, oracle, lo, spp_n, seed=SEED, first=0, traced=True, env=(1.0, 1.0, 1.0)):
        if self.node == "ggx":
            h = self.shh
            return ggx_oracle(oracle, self.c, nthreads=oracle.hardware_threads()).shade(
                self.Ph, lo, spp_n, seed, Kd_color=h["KdColor"], Kd=h["Kd"], Kd_roughness=h["diffuseRoughness"], Ks=h["Ks"],
                Kt_color=h["KtColor"], Kt=h["Kt"], env=env, traced=traced, first_index=first)
        return disney_oracle(oracle, self.c).shade(self.Ph, lo, spp_n, seed, env=env, first_index=first)

    def emit(self, lights, spp_n, seed=SEED, first=0, traced=True, queues=None, share=False):
        T = self.T
        if self.node == "ggx":
            return T.ggx_node_rays(self.s, T.ggx_shader(self.s, **self.sh), self.P, lights, spp_n, seed, first, traced,
                                   queues=queues, share_scratch=share)
        return T.disney_node_rays(self.s, self.P, lights, spp_n, seed, first, queues=queues, share_scratch=share)


def _full(ctx, count, value=1.0):
    return torch.full((3, max(count, 1)), value, dtype=torch.float32, device=ctx.torch_device)


def _unit(ctx, nq, value=1.0):
    """[visibility, one radiance per ray queue]: `value` on every ray (the visibility stays 1)"""
    cnt = nq.counts()
    return [_full(ctx, cnt["shadow"])] + [_full(ctx, cnt[r], value) for r in nq.RAYS]


def _resolve(nq, planes):
    return {q: host(v) for q, v in nq.resolve(*planes).items()}


def _same(got, want, what):
    assert set(got) == set(want)
    for q in want:
        cases.assert_same_bits(got[q], want[q], (what, q))


def _ray_host(q):
    cnt = q.count
    h = dict(offsets=host(q.offsets).astype(np.int64), dir=host(q._dir[:, :cnt]), weight=host(q._weight[:, :cnt]),
             point=host(q._point[:cnt]).astype(np.int64), sample=host(q._sample[:cnt]).astype(np.int64), count=cnt)
    if q._kind is not None:
        h["kind"] = host(q._kind[:cnt]).astype(np.int64)
    return h


def _bytes_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _contract(b, lights, spp_n, first=0, traced=True, share=False, what=""):
    nq = b.emit(lights, spp_n, first=first, traced=traced, share=share)
    got = _resolve(nq, _unit(b.ctx, nq))
    _same(got, b.analytic(lights, spp_n, first=first, traced=traced), (b.node, b.n, spp_n, traced, what))
    return nq


# ---- 1. the contract -----------------------------------------------------------------------------------------------------------
SHAPES = [(4096, 3, 1 << 36), (1, 4, 0), (5, 4, 0), (67, 4, 0), (67, 1, 0), (67, 16, 0), (KBLOCK + 1, 2, 0)]


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("n,spp_n,first", SHAPES)
@pytest.mark.parametrize("node", NODES)
def test_unit_rays_are_the_whole_node_call(gpu, oracle, T, node, n, spp_n, first, fast):
    _, lights = _lights(oracle)
    gpu.set_math_mode(fast)
    try:
        b = Node(T, gpu, oracle, node, n)
        for traced in ((True, False) if node == "ggx" else (True,)):
            nq = _contract(b, lights, spp_n, first, traced, what=("fast", fast))
            cnt = nq.counts()
            if n >= 67:
                assert all(v > 0 for v in cnt.values()), cnt
    finally:
        gpu.set_math_mode(False)


@pytest.mark.parametrize("node", NODES)
def test_unit_rays_at_every_group_width_and_light_count(gpu, oracle, T, monkeypatch, node):
    _, l8 = _lights(oracle, LIGHTS8)
    _, l2 = _lights(oracle)
    n = 300
    b = Node(T, gpu, oracle, node, n)
    for traced in ((True, False) if node == "ggx" else (True,)):
        for lights in (None, l2[:1], l2, l8):
            for spp_n, g in ((4, 1), (4, 4), (4, 16), (8, 64), (3, 64), (5, None)):
                if lights is l8 and g not in (1, None):
                    continue
                want = _at(monkeypatch, 1, lambda: b.analytic(lights, spp_n, traced=traced))
                nq = _at(monkeypatch, g, lambda: b.emit(lights, spp_n, traced=traced))
                assert (nq.shadow is None) == (lights is None)
                _same(_resolve(nq, _unit(gpu, nq)), want, (node, traced, 0 if lights is None else len(lights), spp_n, g))
                if lights is None:
                    assert not want["direct_diffuse"].any() and not want["direct_specular"].any()


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("node", NODES)
def test_unit_rays_uniform_parameters_and_by_reference(gpu, oracle, T, node, fast):
    from trace_util import disney_inputs, ggx_inputs
    _, lights = _lights(oracle)
    n, spp_n = 1001, 3
    gpu.set_math_mode(fast)
    try:
        for kind in ("uniform", "materials"):
            b = Node(T, gpu, oracle, node, n)
            if node == "ggx":
                c, _, mat = ggx_inputs(kind, n)
                if mat is None:
                    b.s = ggx_sampler(gpu, c)
                    b.sh = dict(KdColor=(0.7, 0.5, 0.2), Kd=0.8, diffuseRoughness=0.3, Ks=0.6, KtColor=(0.2, 0.9, 0.7), Kt=0.5)
                else:
                    m = mat[1]
                    u = lambda j: dev(oracle.gen_uniform(cases.SEED_PARITY, 0, m, 900 + j))
                    u3 = lambda j: dev(np.stack([oracle.gen_uniform(cases.SEED_PARITY, 0, m, j + i) for i in range(3)]))
                    kt = oracle.gen_uniform(cases.SEED_PARITY, 0, m, 904)
                    kt[1] = 0.0                                     # one material without transmission
                    b.s = R.GgxSampler(gpu, dev(c["wo"]), dev(c["N"]), dev(c["T"]), specColor=dev(c["KsColor"]), ior=dev(c["ior"]),
                                       roughness=dev(c["roughness"]), anisotropic=dev(c["anisotropic"]), materials=mat)
                    b.sh = dict(KdColor=u3(910), Kd=u(0), diffuseRoughness=u(1), Ks=u(2), KtColor=u3(920), Kt=dev(kt))
            else:
                c, mat = disney_inputs(kind, n)
                if mat is None:
                    b.s = disney_sampler(gpu, c)
                else:
                    sc = {k: dev(c[k]) for k in R._capi.DISNEY_SCALARS if k in c}
                    b.s = R.DisneySampler(gpu, dev(c["wo"]), dev(c["N"]), dev(c["T"]), base_color=dev(c["base_color"]),
                                          materials=mat, **sc)
            for traced in ((True, False) if node == "ggx" else (True,)):
                _contract(b, lights, spp_n, traced=traced, what=kind)
    finally:
        gpu.set_math_mode(False)


@pytest.mark.parametrize("node", NODES)
def test_the_queues_of_one_emit_may_share_one_scratch_block(gpu, oracle, T, node):
    _, lights = _lights(oracle)
    n, spp_n = 777, 4
    b = Node(T, gpu, oracle, node, n)
    own = b.emit(lights, spp_n)
    nq = _contract(b, lights, spp_n, share=True, what="shared scratch")
    assert nq.scratch is not None and nq.scratch.numel() == T.node_scratch_bytes(n, 2, spp_n)
    members = [nq.shadow] + [getattr(nq, r) for r in nq.RAYS]
    assert len({q.q.scratch for q in members}) == 1
    # and the queues are what separate scratch blocks give
    assert _bytes_equal(host(own.shadow._ws[:, :own.shadow.count]), host(nq.shadow._ws[:, :nq.shadow.count]))
    for r in nq.RAYS:
        ho, hs = _ray_host(getattr(own, r)), _ray_host(getattr(nq, r))
        for k in ho:
            assert _bytes_equal(ho[k], hs[k]), (node, r, k)


@pytest.mark.parametrize("node", NODES)
def test_the_separate_kernels_path_keeps_the_unit_contract(gpu, oracle, T, monkeypatch, node):
    """RLS_NODE_RESOLVE=separate (the existing resolve kernels plus a compose kernel, kept for measurement): the same bits as
    the analytic call under unit rays, with and without lights"""
    _, lights = _lights(oracle)
    b = Node(T, gpu, oracle, node, 777)
    monkeypatch.setenv("RLS_NODE_RESOLVE", "separate")
    for traced in ((True, False) if node == "ggx" else (True,)):
        for l in (lights, None):
            _contract(b, l, 4, traced=traced, what="separate kernels")


# ---- 2. the queues are the node's samples ----------------------------------------------------------------------------------------
def _ggx_oracle_queue(oracle, case, spp_n, seed, refract, pair, first=0):
    """trace_util.ggx_oracle_queue at another dimension pair"""
    n, spp = case["wo"].shape[1], spp_n * spp_n
    og = ggx_oracle(oracle, case)
    dirs, ws, keep, kinds = [], [], [], []
    for s in range(spp):
        rx, ry = oracle.batch_sample_02(seed, first, n, pair, s)
        if refract:
            wt, w, flag = og.refract(rx, ry)
            dirs.append(wt); ws.append(w[None, :]); keep.append(w != 0.0); kinds.append(np.where(flag != 0, 0, 1))
        else:
            wi, f, pdf, _ = og.sample_eval_pdf(rx, ry)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                t = (f / pdf[None, :]).astype(np.float32)
            dirs.append(wi); ws.append(t); keep.append(~np.all(t == 0.0, axis=0)); kinds.append(np.zeros(n, np.int64))
    return dirs, ws, keep, kinds


def _disney_oracle_queue(oracle, case, spp_n, seed, lobe, pair, first=0):
    n, spp = case["wo"].shape[1], spp_n * spp_n
    od = disney_oracle(oracle, case)
    dirs, ws, keep = [], [], []
    for s in range(spp):
        rx, ry = oracle.batch_sample_02(seed, first, n, pair, s)
        wi, f, pdf = od.sample_eval_pdf(lobe, rx, ry)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            t = (f / pdf[None, :]).astype(np.float32)
        dirs.append(wi); ws.append(t); keep.append((pdf > EPS) & ~np.all(t == 0.0, axis=0))
    return _queue(dirs, ws, keep)


def _matches(h, want, what, kind=False):
    np.testing.assert_array_equal(h["offsets"], want["offsets"], str(what))
    np.testing.assert_array_equal(h["point"], want["point"], str(what))
    np.testing.assert_array_equal(h["sample"], want["sample"], str(what))
    if kind:
        np.testing.assert_array_equal(h["kind"], want["kind"], str(what))
    assert len(want["point"]) > 0, what
    cases.assert_tight(cases.summarize(cases.rel_err(h["dir"], want["dir"])), (what, "dir"))
    cases.assert_tight(cases.summarize(cases.rel_err(h["weight"], want["weight"])), (what, "weight"))


def _assert_ggx_queues_are_the_oracle_samplers(oracle, b, nq, spp_n, first, seed=SEED):
    """the glossy and refract queues of an rlGgx node emit (traced, one lane per point or any width: the queue does not depend
    on it) against the oracle's samplers at pairs 24 and 25, behind the node's gates"""
    h = b.shh
    open_g = ~np.all(np.abs(b.c["KsColor"]) < EPS, axis=0)
    open_t = ~np.all(np.abs(h["KtColor"] * h["Kt"][None, :]) < EPS, axis=0)
    for member, refract, pair, gate in (("glossy", False, PAIR0, open_g), ("refract", True, PAIR0 + 1, open_t)):
        dirs, ws, keep, kinds = _ggx_oracle_queue(oracle, b.c, spp_n, seed, refract, pair, first)
        want = _queue(dirs, ws, [k & gate for k in keep], kinds)
        _matches(_ray_host(getattr(nq, member)), want, ("ggx", member, pair), kind=refract)


def _assert_disney_queues_are_the_oracle_samplers(oracle, b, nq, spp_n, first, seed=SEED):
    for member, lobe, pair in (("diffuse", DIFFUSE, PAIR0), ("specular", GLOSSY, PAIR0 + 1)):
        _matches(_ray_host(getattr(nq, member)), _disney_oracle_queue(oracle, b.c, spp_n, seed, lobe, pair, first),
                 ("disney", member, pair))


def test_ggx_queues_are_the_oracle_samplers_at_the_node_pairs(gpu, oracle, T, monkeypatch):
    _, lights = _lights(oracle)
    n, spp_n, first = 1024, 3, 1 << 36
    b = Node(T, gpu, oracle, "ggx", n)
    nq = _at(monkeypatch, 1, lambda: b.emit(lights, spp_n, first=first))
    _assert_ggx_queues_are_the_oracle_samplers(oracle, b, nq, spp_n, first)
    # the stream fix: the stand-alone integrator's queue (pair 0) is another queue
    alone = _ray_host(_at(monkeypatch, 1, lambda: T.glossy_rays(b.s, spp_n, SEED, first)))
    mine = _ray_host(nq.glossy)
    m = min(alone["count"], mine["count"])
    assert m > 0 and not np.array_equal(alone["dir"][:, :m], mine["dir"][:, :m])
    # the shadow member is the light-loop emit's queue, plane for plane
    sq = T.ggx_shadow_rays(b.s, T.ggx_shader(b.s, **b.sh), b.P, lights, spp_n, SEED, first)
    ha, hb = queue_host(sq), queue_host(nq.shadow)
    assert ha["count"] > 0
    for k in ha:
        assert _bytes_equal(ha[k], hb[k]), k
    # pair 26: cosine-weighted directions about N -- unit, above the horizon, one scalar weight, nothing where Kd = 0
    d = _ray_host(nq.diffuse)
    assert d["count"] > n and np.all(np.abs(np.linalg.norm(d["dir"].astype(np.float64), axis=0) - 1.0) < 1e-6)
    assert np.all((d["dir"].astype(np.float64) * b.c["N"][:, d["point"]]).sum(axis=0) > -1e-6)
    assert np.all(d["weight"][0] != 0) and np.all(np.isfinite(d["weight"][0]))


def test_ggx_diffuse_queue_is_the_oracle_oren_nayar_at_pair_26(gpu, oracle, T, monkeypatch):
    """(point, sample, dir, weight) of the pair-26 queue, ray by ray: the numbers of orc_batch_sample_02 at dimension pair 26,
    the oracle's cosine-weighted direction about (N, T) -- rlDisney's diffuse-lobe sampler, which is that function on the same
    frame -- and orc_oren_nayar_brdf / orc_oren_nayar_pdf; kept where pdf > 0 and brdf / pdf is not 0, on points with
    sampleDiffuse"""
    import ctypes as C
    _, lights = _lights(oracle)
    n, spp_n, first = 256, 3, 1 << 36
    b = Node(T, gpu, oracle, "ggx", n)
    nq = _at(monkeypatch, 1, lambda: b.emit(lights, spp_n, first=first))
    lib = oracle.lib()

    class ON(C.Structure):
        _fields_ = [("N", oracle.V3), ("T", oracle.V3), ("A", C.c_float), ("B", C.c_float)]
    lib.orc_oren_nayar_brdf.restype = lib.orc_oren_nayar_pdf.restype = C.c_float
    lib.orc_oren_nayar_brdf.argtypes = [C.POINTER(ON), oracle.V3, oracle.V3]
    lib.orc_oren_nayar_pdf.argtypes = [C.POINTER(ON), oracle.V3]
    lib.orc_oren_nayar_init.argtypes = [C.POINTER(ON), oracle.V3, oracle.V3, C.c_float]
    c, h = b.c, b.shh
    v3 = lambda a, i: oracle.V3(*[float(x) for x in a[:, i]])
    ons = []
    for i in range(n):
        on = ON()
        lib.orc_oren_nayar_init(C.byref(on), v3(c["N"], i), v3(c["T"], i), float(h["diffuseRoughness"][i]))
        ons.append(on)
    cosine = disney_oracle(oracle, dict(cases.disney_mixed(cases.SEED_PARITY, n), wo=c["wo"], N=c["N"], T=c["T"]))
    open_d = ~np.all(np.abs(h["KdColor"] * h["Kd"][None, :]) < EPS, axis=0)
    dirs, ws, keep = [], [], []
    for s in range(spp_n * spp_n):
        rx, ry = oracle.batch_sample_02(SEED, first, n, PAIR0 + 2, s)
        d = cosine.sample(DIFFUSE, rx, ry)
        w = np.zeros(n, np.float32)
        for i in range(n):
            pd = np.float32(lib.orc_oren_nayar_pdf(C.byref(ons[i]), v3(d, i)))
            if pd > 0:
                w[i] = np.float32(lib.orc_oren_nayar_brdf(C.byref(ons[i]), v3(c["wo"], i), v3(d, i))) / pd
        dirs.append(d); ws.append(w[None, :]); keep.append((w != 0) & open_d)
    _matches(_ray_host(nq.diffuse), _queue(dirs, ws, keep), ("ggx", "diffuse", PAIR0 + 2))


def test_disney_queues_are_the_oracle_samplers_at_the_node_pairs(gpu, oracle, T, monkeypatch):
    _, lights = _lights(oracle)
    n, spp_n, first = 1024, 3, 98765
    b = Node(T, gpu, oracle, "disney", n)
    nq = _at(monkeypatch, 1, lambda: b.emit(lights, spp_n, first=first))
    _assert_disney_queues_are_the_oracle_samplers(oracle, b, nq, spp_n, first)
    alone = _ray_host(_at(monkeypatch, 1, lambda: T.disney_rays(b.s, GLOSSY, spp_n, SEED, first)))
    mine = _ray_host(nq.specular)
    m = min(alone["count"], mine["count"])
    assert m > 0 and not np.array_equal(alone["dir"][:, :m], mine["dir"][:, :m])
    sq = T.disney_shadow_rays(b.s, b.P, lights, spp_n, SEED, first)
    ha, hb = queue_host(sq), queue_host(nq.shadow)
    for k in ha:
        assert _bytes_equal(ha[k], hb[k]), k


# ---- 3. gates ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traced", [True, False])
def test_ggx_gates(gpu, oracle, T, traced):
    _, lights = _lights(oracle)
    from trace_util import exiting
    n, spp_n = 2048, 3
    b = Node(T, gpu, oracle, "ggx", n)
    b.s = ggx_sampler(gpu, b.c, exiting=exiting(n))               # every fifth point leaves the medium: total internal reflections
    nq = _contract(b, lights, spp_n, traced=traced, what="exiting")
    k = b.k
    cnt = {r: np.diff(host(getattr(nq, r).offsets).astype(np.int64)) for r in GGX_RAYS}
    assert not cnt["diffuse"][k == 0].any() and (cnt["diffuse"][k != 0] > 0).mean() > 0.9
    assert not cnt["refract"][k == 1].any() and cnt["refract"][k > 2].any()
    assert not cnt["glossy"][k == 2].any() and cnt["glossy"][k != 2].any()
    if not traced:
        # at most one ray a point, sample 0, transmitted; none where the analytic call reports total internal reflection
        assert cnt["refract"].max() == 1
        hr = _ray_host(nq.refract)
        assert not hr["sample"].any() and not hr["kind"].any()
        acc, tir = b.s.integrateRefract(spp_n, SEED, traced=False, want_tir=True)
        acc, tir = host(acc)[0], host(tir) != 0
        assert tir.any() and not cnt["refract"][tir].any()
        # a ray wherever the untraced branch has a term: not gated, refracted, and its weight eta2 |N . dir| not 0
        open_t = ~np.all(np.abs(b.shh["KtColor"] * b.shh["Kt"][None, :]) < EPS, axis=0)     # AiColorIsSmall(KtColor * Kt)
        assert not open_t[k == 1].any() and open_t[k != 1].mean() > 0.99
        bad = np.flatnonzero((cnt["refract"] == 1) != ((acc != 0) & open_t))
        assert bad.size == 0, (bad[:8], acc[bad[:8]], tir[bad[:8]], k[bad[:8]])
        assert not acc[tir].any()
    # NaN on every ray of every other point: a gated point's AOV is still exactly 0
    planes = _unit(gpu, nq)
    for j, (r, res) in enumerate((("glossy", 2), ("refract", 1), ("diffuse", 0))):
        pt = host(getattr(nq, r)._point[:getattr(nq, r).count]).astype(np.int64)
        bad = dev(np.where((k[pt] != res)[None, :] & (pt % 3 == 0)[None, :], np.float32(np.nan), np.float32(1.0)).astype(np.float32))
        if bad.shape[1]:
            planes[1 + j] = bad.repeat(3, 1) if bad.shape[0] == 1 else bad
    got = _resolve(nq, planes)
    assert (got["indirect_diffuse"][:, k == 0] == 0).all() and (got["direct_diffuse"][:, k == 0] == 0).all()
    assert (got["refraction"][:, k == 1] == 0).all()
    assert (got["indirect_specular"][:, k == 2] == 0).all()
    assert np.isnan(got["indirect_specular"]).any() and np.isnan(got["indirect_diffuse"]).any()


# ---- 4. non-unit radiance ------------------------------------------------------------------------------------------------------
ENV = (0.7, 0.8, 0.9)


def _env_planes(ctx, nq):
    cnt = nq.counts()
    e = torch.tensor(ENV, dtype=torch.float32, device=ctx.torch_device)[:, None]
    return [_full(ctx, cnt["shadow"])] + [e.expand(3, max(cnt[r], 1)).contiguous() for r in nq.RAYS]


def _tight_after_printing(what, got, ref):
    stats = {q: cases.summarize(cases.rel_err(got[q], ref[q])) for q in ref}
    for q, st in stats.items():
        print(*what, q, st)
    for q, st in stats.items():
        cases.assert_tight(st, (what, q))


@pytest.mark.parametrize("traced", [True, False])
def test_ggx_uniform_radiance_is_the_oracle_shade(gpu, oracle, T, monkeypatch, traced):
    """every AOV, the pair-26 Oren-Nayar queue through indirect_diffuse among them, against orc_batch_ggx_shade(env), at the
    project's parity gate for the quantity, cases.assert_tight.  The resolve sums about the radiance of a point's first ray, so
    under a uniform radiance it forms (sum w x inv) x env as the analytic call and the oracle do."""
    lo, lights = _lights(oracle)
    n, spp_n, first = 4096, 3, 1 << 36
    b = Node(T, gpu, oracle, "ggx", n)
    ref = b.oracle_shade(oracle, lo, spp_n, first=first, traced=traced, env=ENV)
    nq = _at(monkeypatch, 1, lambda: b.emit(lights, spp_n, first=first, traced=traced))
    got = _resolve(nq, _env_planes(gpu, nq))
    assert (ref["indirect_diffuse"] > 0).mean() > 0.5
    _same(got, _at(monkeypatch, 1, lambda: b.analytic(lights, spp_n, first=first, traced=traced, env=ENV)), ("ggx", traced, "env"))
    _tight_after_printing(("ggx node", traced), got, ref)


def test_disney_uniform_radiance_is_the_oracle_shade(gpu, oracle, T, monkeypatch):
    """as the rlGgx test above"""
    lo, lights = _lights(oracle)
    n, spp_n, first = 4096, 4, 98765
    b = Node(T, gpu, oracle, "disney", n)
    ref = b.oracle_shade(oracle, lo, spp_n, first=first, env=ENV)
    nq = _at(monkeypatch, 1, lambda: b.emit(lights, spp_n, first=first))
    got = _resolve(nq, _env_planes(gpu, nq))
    _same(got, _at(monkeypatch, 1, lambda: b.analytic(lights, spp_n, first=first, env=ENV)), ("disney", "env"))
    _tight_after_printing(("disney node",), got, ref)


def _rad(lights):
    return np.array([[l.radiance[k] for k in range(3)] for l in lights], np.float32)


def _random_planes(nq, seed=5, hdr=False):
    """a coloured visibility in [0.25, 1.25) and one radiance per ray and channel: in [0.25, 1.25), or (hdr) e^U(-7, 12) --
    eight decades, so that single rays outshine the rest of their point by 1e5 and more -- with every 13th value 0"""
    g = torch.Generator().manual_seed(seed)
    cnt = nq.counts()
    planes = [(0.25 + torch.rand(3, max(cnt[r], 1), generator=g)).to(torch.float32) for r in ("shadow",) + nq.RAYS]
    if hdr:
        for j in range(1, len(planes)):
            L = torch.exp(-7.0 + 19.0 * torch.rand(planes[j].shape, generator=g)).to(torch.float32)
            L.view(-1)[::13] = 0.0
            planes[j] = L
    return planes


def _compose_node(b, nq, planes, lights, spp_n, traced, dtype, absolute=False, plain=False):
    """the documented composition on the host in `dtype` (absolute: every factor's magnitude, for the rounding bound; plain:
    S = inv sum L w without a reference, the quantity the resolve stands for)"""
    f = (lambda a: np.abs(np.asarray(a, dtype))) if absolute else (lambda a: np.asarray(a, dtype))
    n, spp = b.n, spp_n * spp_n
    inv = dtype(np.float32(1.0) / np.float32(spp))
    hs = queue_host(nq.shadow)
    if absolute:
        hs = dict(hs, ws=np.abs(hs["ws"]), wd=np.abs(hs["wd"]))
    tail = None
    if b.node == "ggx":
        h = b.shh
        dcol = (h["KdColor"] * h["Kd"][None, :]).astype(np.float32)
        tcol = (h["KtColor"] * h["Kt"][None, :]).astype(np.float32)
        tail = (f(dcol), f(h["Ks"]))
    dd, ds = compose(hs, planes[0].numpy(), f(_rad(lights)), spp, dtype=dtype, tail=tail)
    # per ray queue S = (A inv) Lref + B inv with Lref the radiance of smallest magnitude among the point's rays, A = sum w, B = sum (L - Lref) w,
    # both grown in queue order (include/rlshaders_amd_trace.h); absolute: inv (|Lref| sum |w| + sum |L - Lref| |w|)
    sums = {}
    for j, r in enumerate(nq.RAYS):
        hq = _ray_host(getattr(nq, r))
        L, w, off = planes[1 + j].numpy()[:, :hq["count"]].astype(dtype), f(hq["weight"]), hq["offsets"]
        cnt = np.diff(off)
        inv_r = dtype(1) if (r == "refract" and not traced) else inv
        ref = np.zeros((3, n), dtype)
        if not plain:
            ref[:, cnt > 0] = L[:, off[:-1][cnt > 0]]
        with np.errstate(invalid="ignore"):
            for i in range(1, 0 if plain else (int(cnt.max()) if n else 0)):      # the radiance of smallest magnitude, the first such
                m = np.flatnonzero(cnt > i)
                cand = L[:, off[:-1][m] + i]
                ref[:, m] = np.where(np.abs(cand) < np.abs(ref[:, m]), cand, ref[:, m])
        A, B = np.zeros((3, n), dtype), np.zeros((3, n), dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(int(cnt.max()) if n else 0):
                m = cnt > i
                at = off[:-1][m] + i
                d = (L[:, at] - ref[:, m]).astype(dtype)
                A[:, m] = A[:, m] + w[:, at]
                # (a ray AT the reference adds nothing, whatever its weight: ray_sums_about_reference)
                B[:, m] = B[:, m] + np.where(d == 0, dtype(0), (np.abs(d) if absolute else d) * w[:, at]).astype(dtype)
            sums[r] = ((A * inv_r).astype(dtype) * f(ref)).astype(dtype) + (B * inv_r).astype(dtype)
    out = dict(direct_diffuse=dd, direct_specular=ds)
    if b.node == "ggx":
        small = lambda c: np.all(np.abs(c) < EPS, axis=0)
        out["refraction"] = np.where(small(tcol)[None, :], dtype(0), sums["refract"] * f(tcol))
        out["indirect_diffuse"] = np.where(small(dcol)[None, :], dtype(0), f(dcol) * sums["diffuse"])
        out["indirect_specular"] = np.where(small(b.c["KsColor"])[None, :], dtype(0), sums["glossy"] * f(h["Ks"])[None, :])
        out["out"] = ((dd + ds) + out["refraction"]) + (out["indirect_diffuse"] + out["indirect_specular"])
    else:
        out["indirect_diffuse"], out["indirect_specular"] = sums["diffuse"], sums["specular"]
        out["out"] = (dd + ds) + (out["indirect_diffuse"] + out["indirect_specular"])
    return {q: v.astype(dtype) for q, v in out.items()}, {r: np.diff(_ray_host(getattr(nq, r))["offsets"]) for r in sums}, \
        np.diff(hs["offsets"])


def _assert_within_the_float64_bound(b, nq, planes, lights, spp_n, traced, got, what=""):
    """got: the resolve of nq under `planes`, {AOV: [3, b.n]}"""
    node = b.node
    # float64, against the PLAIN sum inv sum L w, the quantity the resolve stands for, and relative to the plain sum's own
    # magnitude inv sum |L| |w| x |tail|.  Over a queue's k rays of the point: one rounding per addition into A, three per term
    # of B (L - Lref, x w, +), then x inv (twice), x Lref, the final + and up to two for the tail: (k + 6) 2^-24 of
    # inv (|Lref| sum |w| + sum |L - Lref| |w|) x |tail|, each term's roundings counted against its own magnitude; and
    # |Lref| <= |L| on every ray (Lref is the radiance of smallest magnitude), so that magnitude is at most 3 x the plain
    # sum's: 3 (k + 6) 2^-24, whatever single ray is bright (hdr: e^U(-7, 12) with zeros).  The light loop as
    # tests/test_gpu_trace_lights.py: k + 3 nl + 2; out adds the four or five AOVs: 4 more roundings on the sum of their bounds
    e64, kr, ks = _compose_node(b, nq, planes, lights, spp_n, traced, np.float64, plain=True)
    mag, _, _ = _compose_node(b, nq, planes, lights, spp_n, traced, np.float64, absolute=True, plain=True)
    u = 2.0 ** -24
    ray_of = dict(refraction="refract", indirect_diffuse="diffuse", indirect_specular="glossy") if node == "ggx" else \
        dict(indirect_diffuse="diffuse", indirect_specular="specular")
    bounds = {q: (ks + 3 * len(lights) + 2) * u * mag[q] for q in ("direct_diffuse", "direct_specular")}
    bounds.update({q: 3 * (kr[r] + 6) * u * mag[q] for q, r in ray_of.items()})
    bounds["out"] = sum(bounds.values()) + 4 * u * mag["out"]
    for q, bd in bounds.items():
        err = np.abs(got[q].astype(np.float64) - e64[q])
        assert np.all(err <= bd + 1e-30), (what, node, q, "worst ratio", float((err / (bd + 1e-30)).max()))


@pytest.mark.parametrize("hdr", [False, True], ids=["ldr", "hdr"])
@pytest.mark.parametrize("node,traced", [("ggx", True), ("ggx", False), ("disney", True)])
def test_random_radiance_is_the_documented_composition(gpu, oracle, T, node, traced, hdr):
    _, lights = _lights(oracle)
    n, spp_n = 1500, 4
    b = Node(T, gpu, oracle, node, n)
    nq = b.emit(lights, spp_n, traced=traced)
    planes = _random_planes(nq, hdr=hdr)
    got = _resolve(nq, [p.cuda() for p in planes])
    want, _, _ = _compose_node(b, nq, planes, lights, spp_n, traced, np.float32)
    _same(got, want, (node, traced, "numpy float32 composition"))
    _assert_within_the_float64_bound(b, nq, planes, lights, spp_n, traced, got)


# ---- 5. robustness ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("node", NODES)
def test_a_non_finite_radiance_stays_in_its_point_and_aov(gpu, oracle, T, node):
    _, lights = _lights(oracle)
    n, spp_n = 700, 3
    b = Node(T, gpu, oracle, node, n)
    nq = b.emit(lights, spp_n)
    clean = _resolve(nq, _unit(gpu, nq))
    aov_of = dict(glossy="indirect_specular", refract="refraction", diffuse="indirect_diffuse") if node == "ggx" else \
        dict(diffuse="indirect_diffuse", specular="indirect_specular")
    for j, r in enumerate(nq.RAYS):
        q = getattr(nq, r)
        ray = q.count // 2
        pt = int(q._point[ray].item())
        planes = _unit(gpu, nq)
        planes[1 + j][1, ray] = float("inf")
        got = _resolve(nq, planes)
        for a in clean:
            hit = a in (aov_of[r], "out")
            other = np.arange(n) != pt
            cases.assert_same_bits(got[a][:, other], clean[a][:, other], (node, r, a, "other points"))
            if hit:
                assert not np.isfinite(got[a][1, pt]), (node, r, a)
                cases.assert_same_bits(got[a][0::2, pt], clean[a][0::2, pt], (node, r, a, "other channels"))
            else:
                cases.assert_same_bits(got[a][:, pt], clean[a][:, pt], (node, r, a, "other AOVs"))


@pytest.mark.parametrize("node", NODES)
def test_first_index_past_2_32_and_chunks(gpu, oracle, T, node):
    _, lights = _lights(oracle)
    n, spp_n, first = 1500, 3, (1 << 32) - 600
    full_b = Node(T, gpu, oracle, node, n, full=n)
    nq = _contract(full_b, lights, spp_n, first, what="first_index past 2^32")
    planes = _random_planes(nq)
    rf = _resolve(nq, [p.cuda() for p in planes])
    q0 = full_b.emit(lights, spp_n, first=0)
    base = _resolve(q0, _unit(gpu, q0))                             # the index reaches the scrambles
    assert not np.array_equal(base["indirect_specular"], _resolve(nq, _unit(gpu, nq))["indirect_specular"])
    names = ("shadow",) + nq.RAYS
    off = {r: host(getattr(nq, r).offsets).astype(np.int64) for r in names}
    for a, e in ((0, 555), (555, 600), (600, 601), (601, n)):
        bc = Node(T, gpu, oracle, node, e - a, a=a, full=n)
        qc = bc.emit(lights, spp_n, first=first + a)
        sub = []
        for j, r in enumerate(names):
            lo, hi = int(off[r][a]), int(off[r][e])
            np.testing.assert_array_equal(host(getattr(qc, r).offsets).astype(np.int64), off[r][a:e + 1] - lo)
            sub.append(planes[j][:, lo:max(hi, lo + 1)].contiguous().cuda())
        got = _resolve(qc, sub)
        _same(got, {q: v[:, a:e] for q, v in rf.items()}, (node, a, e, "chunk"))


@pytest.mark.parametrize("node", NODES)
def test_emit_and_resolve_in_a_graph(oracle, T, node):
    _, lights = _lights(oracle)
    n, spp_n = 2000, 3
    gctx = R.Context(0, use_torch_stream=False)          # the context's own stream: the NULL stream cannot be captured
    try:
        b = Node(T, gctx, oracle, node, n)
        torch.cuda.synchronize()
        direct = b.emit(lights, spp_n)
        gctx.synchronize()
        cnt = direct.counts()
        planes = [p.cuda() for p in _random_planes(direct)]
        torch.cuda.synchronize()
        want = direct.resolve(*planes)
        gctx.synchronize()
        want = {q: host(v) for q, v in want.items()}
        cls = T.GgxNodeQueues if node == "ggx" else T.DisneyNodeQueues
        nq = cls(gctx, n, len(lights), spp_n, True)
        out = {q: gctx.empty(3, n) for q in want}
        torch.cuda.synchronize()
        with gctx.capture() as g:
            b.emit(lights, spp_n, queues=nq)
            nq.resolve(*planes, out=out, counts=cnt)
        for o in out.values():
            o.zero_()
        for r in ("shadow",) + nq.RAYS:
            getattr(nq, r).offsets.zero_()
        torch.cuda.synchronize()
        g.launch()
        gctx.synchronize()
        g.close()
        assert nq.counts() == cnt
        _same({q: host(v) for q, v in out.items()}, want, (node, "replay"))
    finally:
        gctx.close()


@pytest.mark.parametrize("node", NODES)
def test_argument_checks_on_the_device_path(gpu, oracle, T, node):
    import ctypes as C
    _, lights = _lights(oracle)
    n, spp_n = 64, 2
    b = Node(T, gpu, oracle, node, n)
    nq = b.emit(lights, spp_n)
    planes = _unit(gpu, nq)
    want = _resolve(nq, planes)
    err = lambda: R.load().rls_last_error().decode()
    emit_name = f"rls_trace_{node}_shade_emit"
    nq.spp_n = 17
    with pytest.raises(R.RlsError):
        b.emit(lights, 17, queues=nq)
    assert err().startswith(emit_name + ": spp_n"), err()
    nq.spp_n = spp_n
    # a short capacity, a short scratch
    ray = getattr(nq, nq.RAYS[-1])
    cap, sb = ray.q.capacity, ray.q.scratch_bytes
    ray.q.capacity = cap - 1
    with pytest.raises(R.RlsError):
        b.emit(lights, spp_n, queues=nq)
    assert err() == emit_name + ": queue.capacity < n * spp_n^2", err()
    ray.q.capacity, ray.q.scratch_bytes = cap, sb - 1
    with pytest.raises(R.RlsError):
        b.emit(lights, spp_n, queues=nq)
    assert err().startswith(emit_name + ": queue.scratch"), err()
    ray.q.scratch_bytes = sb
    # lights without a shadow queue, and a shadow queue without lights
    keep = nq.shadow
    nq.shadow, nq.n_lights = None, 2
    with pytest.raises(R.RlsError):
        b.emit(lights, spp_n, queues=nq)
    assert err() == emit_name + ": queues.shadow is NULL but n_lights > 0", err()
    nq.shadow, nq.n_lights = keep, 0
    with pytest.raises(R.RlsError):
        b.emit(None, spp_n, queues=nq)
    assert err() == emit_name + ": queues.shadow is set but n_lights is 0", err()
    nq.n_lights = 2
    # a radiance plane that is too short is refused by the binding; after the refusals the queues still resolve
    with pytest.raises(ValueError):
        nq.resolve(planes[0], *[p[:, :0] for p in planes[1:]])
    nq = b.emit(lights, spp_n, queues=nq)
    _same(_resolve(nq, planes), want, (node, "after the refusals"))
    # n == 0: empty queues
    e = Node(T, gpu, oracle, node, 1)
    e.s.n = 0
    cls = T.GgxNodeQueues if node == "ggx" else T.DisneyNodeQueues
    q0 = cls(gpu, 0, 2, spp_n)
    for r in ("shadow",) + q0.RAYS:
        getattr(q0, r).offsets.fill_(-1)
    if node == "ggx":
        T.ggx_node_rays(e.s, T.ggx_shader(e.s), None, lights, spp_n, SEED, queues=q0)
    else:
        T.disney_node_rays(e.s, None, lights, spp_n, SEED, queues=q0)
    assert all(v == 0 for v in q0.counts().values())
