"""GPU: rlGgx and rlDisney at the hits of secondary rays (include/rlshaders_amd_trace.h, rls_trace_ggx_bounce_* /
rls_trace_disney_bounce_* / rls_trace_ray_state_advance; rlshaders_amd/trace.py, ggx_bounce_rays / disney_bounce_rays /
advance_state).

Every expected value comes from calls that are already held to the oracle (rls_trace_*_shade_emit / _resolve,
rls_ggx_shade / rls_disney_shade, tests/test_gpu_trace_shade.py and tests/test_gpu_shade.py), never from the calls under test:
  1. identity: all-camera, depth-0 state and open depths give the node calls' bytes -- every queue plane, offsets, every
     output; depths.refraction = 0 gives rlGgx's traced = 0;
  2. a mixed state under unit visibility and a uniform radiance: every AOV and out is a per-point selection among the analytic
     calls, the ray-depth switches applied in numpy float32;
  3. the queues, point by point: each CSR slice is the matching existing emit's slice, filtered by the switches; offsets a host
     int64 cumsum; every plane and the exact-size scratch inside sentinels;
  4. random visibility and radiance over eight decades: the documented composition in numpy float32 (bits) and float64 (the
     node resolves' bound);
  5. rls_trace_ray_state_advance against numpy on a real glossy queue;
  6. chunks with first_index (past 2^36 too), graph replay, parameters uniform and by reference.
The state is drawn per point from STATES by (7 i + i // 3) % len(STATES): neighbouring lanes, lane groups and tiles differ.
Inputs: seed 99, the "mixed" parameters (colours in [0, 1)), the slab and lights of tests/test_gpu_shade.py."""
import numpy as np
import pytest
import torch

import cases
import rlshaders_amd as R
from gpu_util import dev, host
from test_gpu_loop_edges import LIGHTS as LIGHTS8
from test_gpu_shade import _lights
from test_gpu_trace_node_edges import Padded, _rehouse
from test_gpu_trace_shade import (ENV, EPS, KBLOCK, Node, T, _at, _bytes_equal, _compose_node, _random_planes, _ray_host, _same)  # noqa: F401
from trace_lights_util import BSDF, DIFFUSE as K_DIFFUSE, LIGHT_MASK, SPECULAR as K_SPECULAR, queue_host

pytestmark = pytest.mark.gpu

SEED_IN, SEED = 99, 41
NODES = ("ggx", "disney")
CAM, SHD, RFL, RFR, DIF, GLS = 0x01, 0x02, 0x04, 0x08, 0x20, 0x40          # RLS_RT_*
DEPTHS = dict(total=4, diffuse=2, glossy=3, refraction=2)
OPEN = dict(total=100, diffuse=100, glossy=100, refraction=100)
# (ray_type, Rr, Rr_diff, Rr_gloss, Rr_refr).  With DEPTHS: camera at depth 0; each secondary type; a shadow ray; each depth test
# at its limit, one below and one past it -- rlGgx tests Rr_diff / Rr_gloss with <=, rlDisney with <, so the limit itself opens
# one node's switch and shuts the other's; Rr_refr and Rr against refraction / total with <; Rr at depths.total and past it.
STATES = np.array([
    (CAM, 0, 0, 0, 0),       # a camera ray at depth 0
    (RFL, 1, 0, 0, 0),       # reflected
    (RFR, 1, 0, 0, 1),       # refracted, Rr_refr one below its limit: the traced branch
    (DIF, 2, 2, 0, 0),       # diffuse, Rr_diff AT the limit: rlGgx's sampleDiffuse holds (<=)
    (GLS, 3, 0, 3, 0),       # glossy, Rr_gloss AT the limit: rlGgx's specular term is there (<=); Rr one below total
    (SHD, 1, 0, 0, 0),       # a shadow ray: nothing
    (DIF, 3, 3, 0, 0),       # Rr_diff one past: no diffuse term
    (GLS, 4, 0, 4, 0),       # Rr_gloss one past: no specular term; Rr AT total: the untraced branch
    (RFR, 2, 0, 0, 2),       # Rr_refr AT its limit: the untraced branch (<)
    (CAM, 1, 1, 2, 1),       # a camera point below every limit: rlDisney's indirect loops run
    (CAM, 2, 2, 3, 1),       # camera, Rr_diff and Rr_gloss AT the limits: rlDisney's loops do not run (<), rlGgx's terms are there
    (CAM, 4, 1, 2, 1),       # camera, Rr AT total: rlDisney's loops do not run, rlGgx takes the untraced branch
    (CAM, 3, 3, 4, 3),       # camera past the diffuse, glossy and refraction limits
    (RFR, 5, 0, 0, 1),       # Rr one past total
    (RFR, 3, 0, 0, 1),       # Rr one below total: the traced branch
], np.uint8)
assert len({tuple(s) for s in STATES}) == len(STATES) >= 11


def plan(n, a=0, table=STATES):
    i = np.arange(a, a + n)
    return np.ascontiguousarray(table[(7 * i + i // 3) % len(table)].T)          # [5, n]


def gates(st, d):
    """the switches of include/rlshaders_amd_trace.h, per point"""
    rt, rr, rd, rg, rf = (st[k].astype(np.int64) for k in range(5))
    lit = (rt & SHD) == 0
    cam = lit & ((rt & CAM) != 0)
    g = dict(lit=lit, cam=cam, sD=lit & (rd <= d["diffuse"]), sS=lit & (rg <= d["glossy"]),
             tr=(rf < d["refraction"]) & (rr < d["total"]), scaled=(rt & (DIF | GLS)) != 0,
             td=cam & (rd < d["diffuse"]) & (rr < d["total"]), tg=cam & (rg < d["glossy"]) & (rr < d["total"]))
    return g


_CASES = {}


def _case(oracle, node, m):
    """the inputs of tests/test_gpu_trace_shade.py's Node at seed 99: the closure, the slab, rlGgx's node parameters with Kd = 0,
    Kt = 0 and a black KsColor on the residues 0, 1, 2 of i % 8; rlDisney's two scales with 0 and 1 among them"""
    if (node, m) in _CASES:
        return _CASES[node, m]
    u = lambda j: oracle.gen_uniform(SEED_IN, 0, m, oracle.S_PARAM0 + j, 0.0, 1.0)
    P = (cases.xi(SEED_IN, m, 3) * np.array([[4.0], [4.0], [1.0]], np.float32)).astype(np.float32)
    k = np.arange(m) % 8
    if node == "ggx":
        c = cases.ggx_mixed(SEED_IN, m)
        kdc, ktc = np.stack([u(j) for j in range(3)]), np.stack([u(3 + j) for j in range(3)])
        kd = np.where(k == 0, np.float32(0.0), u(6)).astype(np.float32)
        kt = np.where(k == 1, np.float32(0.0), u(9)).astype(np.float32)
        c = dict(c, KsColor=np.where((k == 2)[None, :], np.float32(0.0), c["KsColor"]).astype(np.float32))
        shh = dict(KdColor=kdc, Kd=kd, diffuseRoughness=u(7), Ks=u(8), KtColor=ktc, Kt=kt)
        r = dict(P=P, c=c, shh=shh)
    else:
        sc = [u(20 + j) for j in range(2)]
        for s, (zero, one) in zip(sc, ((0, 1), (3, 2))):
            s[k % 5 == zero] = 0.0
            s[k % 5 == one] = 1.0
        r = dict(P=P, c=cases.disney_mixed(SEED_IN, m), shh=None, scales=sc)
    _CASES[node, m] = r
    return r


class Bounce(Node):
    """Node over points a .. a + n of the seed-99 inputs, with the bounce emit"""

    def __init__(self, T, ctx, oracle, node, n, a=0, full=None):
        m = max(a + n, 128) if full is None else full
        full_case = _case(oracle, node, m)
        sl = lambda v: np.ascontiguousarray(v[..., a:a + n])
        case = dict(P=sl(full_case["P"]), c={q: sl(v) for q, v in full_case["c"].items()})
        if node == "ggx":
            case["shh"] = {q: sl(v) for q, v in full_case["shh"].items()}
        super().__init__(T, ctx, oracle, node, n, a=a, case=case)
        self.a = a
        self.scales_h = [sl(s) for s in full_case["scales"]] if node == "disney" else None
        self.scales = [dev(s) for s in self.scales_h] if node == "disney" else None

    def state(self, table=STATES):
        st = plan(self.n, self.a, table)
        return st, self.T.RayState(*[dev(st[k]) for k in range(5)])

    def bounce(self, lights, spp_n, state, depths, first=0, queues=None, share=False, seed=SEED):
        T = self.T
        if self.node == "ggx":
            return T.ggx_bounce_rays(self.s, T.ggx_shader(self.s, **self.sh), self.P, lights, spp_n, seed, state, depths, first,
                                     queues=queues, share_scratch=share)
        return T.disney_bounce_rays(self.s, self.P, lights, spp_n, seed, state, depths, first, queues=queues, share_scratch=share,
                                    indirectDiffuseScale=self.scales[0], indirectSpecularScale=self.scales[1])


def _members(nq):
    return {r: getattr(nq, r) for r in (("shadow",) if nq.shadow is not None else ()) + nq.RAYS}


def _queue_hosts(nq):
    return {r: (queue_host(q) if r == "shadow" else _ray_host(q)) for r, q in _members(nq).items()}


def _same_queues(got, want, what):
    assert set(got) == set(want)
    for r in want:
        np.testing.assert_array_equal(got[r]["offsets"], want[r]["offsets"], str((what, r, "offsets")))
        for k in want[r]:
            if k != "count":
                assert _bytes_equal(got[r][k], want[r][k]), (what, r, k)


def _planes(ctx, nq, value=None, seed=5, hdr=False):
    """[visibility, one radiance per ray queue] on the device: `value` on every ray under visibility 1, or random"""
    cnt = nq.counts()
    if value is not None:
        e = torch.tensor(value, dtype=torch.float32, device=ctx.torch_device)[:, None]
        one = torch.ones(3, max(cnt["shadow"], 1), dtype=torch.float32, device=ctx.torch_device)
        return [one] + [e.expand(3, max(cnt[r], 1)).contiguous() for r in nq.RAYS]
    return [p.cuda() for p in _random_planes(nq, seed=seed, hdr=hdr)]


def _resolve(nq, planes, out=None, counts=None):
    return {q: host(v) for q, v in nq.resolve(*planes, out=out, counts=counts).items()}


# ---- 1. identity ------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (5, 2), (67, 3), (67, 16), (KBLOCK + 1, 4), (2049, 2)]


def _assert_identity(b, lights, spp_n, first=0, what=""):
    cam = b.T.RayState.camera(b.ctx, b.n)
    for traced in ((True, False) if b.node == "ggx" else (True,)):
        depths = OPEN if traced else dict(OPEN, refraction=0)
        parent = b.emit(lights, spp_n, first=first, traced=traced)
        nq = b.bounce(lights, spp_n, cam, depths, first=first)
        _same_queues(_queue_hosts(nq), _queue_hosts(parent), (b.node, b.n, spp_n, traced, what))
        planes = _planes(b.ctx, parent, seed=b.n)
        _same(_resolve(nq, planes), {q: host(v) for q, v in parent.resolve(*planes).items()}, (b.node, b.n, spp_n, traced, what))
    return nq


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("n,spp_n", SHAPES)
@pytest.mark.parametrize("node", NODES)
def test_camera_state_at_depth_0_is_the_node_call(gpu, oracle, T, node, n, spp_n, fast):
    _, lights = _lights(oracle)
    gpu.set_math_mode(fast)
    try:
        b = Bounce(T, gpu, oracle, node, n)
        nq = _assert_identity(b, lights, spp_n, first=(1 << 36) + 5 if n == 67 else 0, what=("fast", fast))
        if n >= 67:
            assert all(v > 0 for v in nq.counts().values())
        # rlDisney's scales act on diffuse and glossy rays only: here they change nothing (they are not 1)
    finally:
        gpu.set_math_mode(False)


@pytest.mark.parametrize("node", NODES)
def test_camera_state_at_every_group_width_and_light_count(gpu, oracle, T, monkeypatch, node):
    _, l8 = _lights(oracle, LIGHTS8)          # mis_mode 0, 1 and 2 among them
    b = Bounce(T, gpu, oracle, node, 67)
    for lights in (None, l8[1:2], l8[:2], l8):
        for spp_n, g in ((4, 1), (4, 4), (4, 16), (8, 64), (3, 64), (3, None)):
            if lights is l8 and g not in (1, 64, None):
                continue
            _at(monkeypatch, g, lambda: _assert_identity(b, lights, spp_n, what=(0 if lights is None else len(lights), g)))


# ---- 2. a mixed state under a uniform radiance: a selection among the analytic calls ------------------------------------------------
def _select(b, st, d, A1, A0):
    """A1 / A0: the analytic call's AOVs at traced = 1 / 0 (rlDisney: A1 alone), under one env -> the bounce call's"""
    g, f = gates(st, d), np.float32
    zero = np.zeros((3, b.n), f)
    pick = lambda m, v: np.where(m[None, :], v, zero)
    if b.node == "ggx":
        h = b.shh
        dcol = (h["KdColor"] * h["Kd"][None, :]).astype(f)
        dd = pick(g["lit"], np.where(g["sD"][None, :], A1["direct_diffuse"], f(0.0) * dcol))
        ds = pick(g["lit"], np.where(g["sS"][None, :], A1["direct_specular"], f(0.0) * h["Ks"][None, :]))
        tx = pick(g["lit"], np.where(g["tr"][None, :], A1["refraction"], A0["refraction"]))
        iD, iS = pick(g["cam"] & g["sD"], A1["indirect_diffuse"]), pick(g["cam"], A1["indirect_specular"])
        out = np.where(g["cam"][None, :], ((dd + ds) + tx) + (iD + iS), (dd + ds) + tx)
        return dict(direct_diffuse=dd, direct_specular=ds, refraction=tx, indirect_diffuse=iD, indirect_specular=iS, out=out)
    kd, ks = b.scales_h
    dd = pick(g["lit"], np.where(g["scaled"][None, :], A1["direct_diffuse"] * kd[None, :], A1["direct_diffuse"]).astype(f))
    ds = pick(g["lit"], np.where(g["scaled"][None, :], A1["direct_specular"] * ks[None, :], A1["direct_specular"]).astype(f))
    iD, iS = pick(g["td"], A1["indirect_diffuse"]), pick(g["tg"], A1["indirect_specular"])
    out = np.where(g["cam"][None, :], (dd + ds) + (iD + iS), dd + ds)
    return dict(direct_diffuse=dd, direct_specular=ds, indirect_diffuse=iD, indirect_specular=iS, out=out)


def _assert_selection(b, lights, spp_n, first=0, what=""):
    st, state = b.state()
    nq = b.bounce(lights, spp_n, state, DEPTHS, first=first)
    for env in (ENV, (1.0, 1.0, 1.0)):
        A1 = b.analytic(lights, spp_n, first=first, traced=True, env=env)
        A0 = b.analytic(lights, spp_n, first=first, traced=False, env=env) if b.node == "ggx" else None
        got = _resolve(nq, _planes(b.ctx, nq, value=env))
        _same(got, _select(b, st, DEPTHS, A1, A0), (b.node, b.n, spp_n, env, what))
        shadow = (st[0] & SHD) != 0
        for q, v in got.items():                                  # +0, not -0, at a shadow ray's point
            assert not v[:, shadow].view(np.uint32).any(), (q, what)
    return nq


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("n,spp_n,g", [(1, 4, None), (5, 1, 1), (67, 3, 4), (67, 16, 64), (KBLOCK + 1, 4, 16), (2049, 2, None)])
@pytest.mark.parametrize("node", NODES)
def test_mixed_state_is_a_selection_among_the_analytic_calls(gpu, oracle, T, monkeypatch, node, n, spp_n, g, fast):
    _, lights = _lights(oracle)
    gpu.set_math_mode(fast)
    try:
        b = Bounce(T, gpu, oracle, node, n)
        _at(monkeypatch, g, lambda: _assert_selection(b, lights, spp_n, what=("fast", fast, g)))
    finally:
        gpu.set_math_mode(False)


@pytest.mark.parametrize("node", NODES)
def test_mixed_state_at_every_light_count(gpu, oracle, T, monkeypatch, node):
    _, l8 = _lights(oracle, LIGHTS8)
    b = Bounce(T, gpu, oracle, node, 300)
    for lights in (None, l8[1:2], l8[:2], l8):
        _at(monkeypatch, 1, lambda: _assert_selection(b, lights, 2, what=0 if lights is None else len(lights)))


# ---- 3. the queues, point by point --------------------------------------------------------------------------------------------------
def _csr(points, n):
    return np.concatenate([[0], np.cumsum(np.bincount(points, minlength=n).astype(np.int64), dtype=np.int64)])


def _filtered(h, keep, n):
    """the rays of a queue on the host whose mask is set, in order; offsets: the host int64 cumsum of what is left"""
    out = {k: v[..., keep] for k, v in h.items() if k not in ("offsets", "count")}
    out["offsets"], out["count"] = _csr(h["point"][keep], n), int(keep.sum())
    return out


def _expected_queues(b, st, d, N1, N0):
    """N1 / N0: the node emit's queues on the host at traced = 1 / 0 (rlDisney: N1 alone)"""
    g, n = gates(st, d), b.n
    want = {}
    if "shadow" in N1:
        h = N1["shadow"]
        if b.node == "ggx":
            allowed = np.where(g["sS"], K_SPECULAR, 0) | np.where(g["sD"], K_DIFFUSE, 0)
        else:
            allowed = np.where(g["lit"], K_SPECULAR | K_DIFFUSE, 0)
        kind = h["kind"] & (allowed[h["point"]] | LIGHT_MASK | BSDF)
        want["shadow"] = _filtered(dict(h, kind=kind), (kind & (K_SPECULAR | K_DIFFUSE)) != 0, n)
    if b.node == "ggx":
        want["glossy"] = _filtered(N1["glossy"], g["cam"][N1["glossy"]["point"]], n)
        want["diffuse"] = _filtered(N1["diffuse"], (g["cam"] & g["sD"])[N1["diffuse"]["point"]], n)
        h1, h0 = N1["refract"], N0["refract"]
        k1, k0 = (g["lit"] & g["tr"])[h1["point"]], (g["lit"] & ~g["tr"])[h0["point"]]
        pts = np.concatenate([h1["point"][k1], h0["point"][k0]])
        order = np.argsort(pts, kind="stable")                    # (a point's rays come from one of the two)
        r = {k: np.concatenate([h1[k][..., k1], h0[k][..., k0]], axis=-1)[..., order] for k in h1 if k not in ("offsets", "count")}
        r["offsets"], r["count"] = _csr(pts, n), len(pts)
        want["refract"] = r
    else:
        want["diffuse"] = _filtered(N1["diffuse"], g["td"][N1["diffuse"]["point"]], n)
        want["specular"] = _filtered(N1["specular"], g["tg"][N1["specular"]["point"]], n)
    return want, g


def _padded(T, b, nl, spp_n, pad):
    """a queue set of the documented capacities whose every plane, offsets and exact-size scratch is a view inside sentinels"""
    cls = T.GgxNodeQueues if b.node == "ggx" else T.DisneyNodeQueues
    E = cls(b.ctx, b.n, nl, spp_n, False)
    for r, q in _members(E).items():
        want = T.shadow_scratch_bytes(b.n, nl, spp_n) if r == "shadow" else T.scratch_bytes(b.n, spp_n)
        assert q._scratch.numel() == want and q.capacity == b.n * spp_n * spp_n * (nl * 3 if r == "shadow" else 1)
        _rehouse(T, q, pad)
    return E


@pytest.mark.parametrize("n", [2047, 2048, 2049])
@pytest.mark.parametrize("node", NODES)
def test_queues_are_the_existing_emits_slices_filtered_by_the_state(gpu, oracle, T, monkeypatch, node, n):
    _, lights = _lights(oracle)
    spp_n = 2
    b = Bounce(T, gpu, oracle, node, n)
    st, state = b.state()
    for g in (1, 4):
        N1 = _at(monkeypatch, g, lambda: _queue_hosts(b.emit(lights, spp_n, traced=True)))
        N0 = _at(monkeypatch, 1, lambda: _queue_hosts(b.emit(lights, spp_n, traced=False))) if node == "ggx" else None
        want, gt = _expected_queues(b, st, DEPTHS, N1, N0)
        pad = Padded()
        E = _padded(T, b, len(lights), spp_n, pad)
        out = {q: pad.empty((3, n), gpu.torch_device) for q in b.s.SHADE_AOVS + ("out",)}
        nq = _at(monkeypatch, g, lambda: b.bounce(lights, spp_n, state, DEPTHS, queues=E))
        got = _queue_hosts(nq)
        _same_queues(got, want, (node, n, g))
        cnt = {r: np.diff(h["offsets"]) for r, h in got.items()}
        # the switches, read off the counts: off camera no indirect ray; a shadow ray's point no ray at all; an untraced point
        # one ray at most, sample 0, transmitted
        for r in nq.RAYS:
            if r != "refract":
                assert not cnt[r][~gt["cam"]].any() and cnt[r][gt["cam"]].any(), r
        assert not any(c[~gt["lit"]].any() for c in cnt.values())
        if node == "ggx":
            one = ~gt["tr"]
            assert cnt["refract"][one].max() == 1 and cnt["refract"][gt["tr"] & gt["lit"]].max() > 1
            rr = got["refract"]
            sel = one[rr["point"]]
            assert sel.any() and not rr["sample"][sel].any() and not rr["kind"][sel].any()
            sk = got["shadow"]["kind"]
            pt = got["shadow"]["point"]
            assert not (sk[~gt["sS"][pt]] & K_SPECULAR).any() and not (sk[~gt["sD"][pt]] & K_DIFFUSE).any()
            assert (sk[gt["sS"][pt]] & K_SPECULAR).any() and (sk[gt["sD"][pt]] & K_DIFFUSE).any()
        # resolve into padded AOV planes; nothing beside any view has changed
        plain = b.bounce(lights, spp_n, state, DEPTHS)
        planes = _planes(gpu, plain, seed=n)
        res = _resolve(nq, planes, out=out)
        torch.cuda.synchronize()
        pad.check((node, n, g))
        _same(res, _resolve(plain, planes), (node, n, g, "in padded buffers"))


# ---- 4. random visibility and radiance ------------------------------------------------------------------------------------------------
def _documented(b, nq, planes, lights, spp_n, st, d, dtype, absolute=False, plain=False):
    """tests/test_gpu_trace_shade.py's composition over the bounce call's queues, the per-point switches on top: the refraction
    queue's factor by `tr`, rlDisney's scales, out without the indirect terms off camera"""
    g = gates(st, d)
    f = (lambda a: np.abs(np.asarray(a, dtype))) if absolute else (lambda a: np.asarray(a, dtype))
    c1, kr, ks = _compose_node(b, nq, planes, lights, spp_n, True, dtype, absolute=absolute, plain=plain)
    if b.node == "ggx":
        c0, _, _ = _compose_node(b, nq, planes, lights, spp_n, False, dtype, absolute=absolute, plain=plain)
        tx = np.where(g["tr"][None, :], c1["refraction"], c0["refraction"])
        dd, dsp = c1["direct_diffuse"], c1["direct_specular"]
        iD, iS = c1["indirect_diffuse"], c1["indirect_specular"]
        out = np.where(g["cam"][None, :], ((dd + dsp) + tx) + (iD + iS), (dd + dsp) + tx)
        return dict(c1, refraction=tx, out=out.astype(dtype)), kr, ks
    kd, ksc = (f(s)[None, :] for s in b.scales_h)
    dd = np.where(g["scaled"][None, :], (c1["direct_diffuse"] * kd).astype(dtype), c1["direct_diffuse"])
    dsp = np.where(g["scaled"][None, :], (c1["direct_specular"] * ksc).astype(dtype), c1["direct_specular"])
    iD, iS = c1["indirect_diffuse"], c1["indirect_specular"]
    out = np.where(g["cam"][None, :], (dd + dsp) + (iD + iS), dd + dsp)
    return dict(c1, direct_diffuse=dd, direct_specular=dsp, out=out.astype(dtype)), kr, ks


@pytest.mark.parametrize("hdr", [False, True], ids=["ldr", "hdr"])
@pytest.mark.parametrize("node", NODES)
def test_random_radiance_is_the_documented_composition(gpu, oracle, T, node, hdr):
    """float32: the bits.  float64, against the plain sum inv sum L w and relative to its magnitude: the node resolves' bound
    (tests/test_gpu_trace_shade.py, _assert_within_the_float64_bound: 3 (k + 6) 2^-24 per ray queue, (k + 3 nl + 2) 2^-24 for
    the light loop, out the sum of its terms' bounds + 4 roundings), with one more rounding on rlDisney's scaled direct terms.
    A gated queue has no ray at a gated point (test 3), so no radiance, finite or not, meets a shut switch."""
    _, lights = _lights(oracle)
    n, spp_n = 700, 3
    b = Bounce(T, gpu, oracle, node, n)
    st, state = b.state()
    nq = b.bounce(lights, spp_n, state, DEPTHS)
    planes = _random_planes(nq, hdr=hdr)
    got = _resolve(nq, [p.cuda() for p in planes])
    want, _, _ = _documented(b, nq, planes, lights, spp_n, st, DEPTHS, np.float32)
    _same(got, want, (node, hdr, "numpy float32 composition"))
    e64, kr, ks = _documented(b, nq, planes, lights, spp_n, st, DEPTHS, np.float64, plain=True)
    mag, _, _ = _documented(b, nq, planes, lights, spp_n, st, DEPTHS, np.float64, absolute=True, plain=True)
    u = 2.0 ** -24
    ray_of = dict(refraction="refract", indirect_diffuse="diffuse", indirect_specular="glossy") if node == "ggx" else \
        dict(indirect_diffuse="diffuse", indirect_specular="specular")
    bounds = {q: (ks + 3 * len(lights) + 2 + (node == "disney")) * u * mag[q] for q in ("direct_diffuse", "direct_specular")}
    bounds.update({q: 3 * (kr[r] + 6) * u * mag[q] for q, r in ray_of.items()})
    bounds["out"] = sum(bounds.values()) + 4 * u * mag["out"]
    for q, bd in bounds.items():
        err = np.abs(got[q].astype(np.float64) - e64[q])
        assert np.all(err <= bd + 1e-30), (node, q, "worst ratio", float((err / (bd + 1e-30)).max()))


# ---- 5. rls_trace_ray_state_advance -----------------------------------------------------------------------------------------------------
def test_ray_state_advance(gpu, oracle, T):
    _, lights = _lights(oracle)
    n, spp_n = 257, 3
    b = Bounce(T, gpu, oracle, "ggx", n)
    nq = b.emit(lights, spp_n)
    q = nq.glossy
    pts = host(q.point).astype(np.int64)
    assert len(pts) > n
    table = np.concatenate([STATES, np.array([(GLS, 255, 255, 255, 255), (DIF, 254, 254, 254, 254)], np.uint8)])
    st = plan(n, 0, table)
    parent = T.RayState(*[dev(st[k]) for k in range(5)])
    for rt in (RFL, RFR, DIF, GLS, CAM, DIF | GLS):
        child = T.advance_state(gpu, q, parent, rt)
        got = np.stack([host(getattr(child, k)) for k in T.RayState.PLANES])
        up = lambda v, grow: np.where(grow, np.minimum(255, v.astype(np.int64) + 1), v).astype(np.uint8)
        want = np.stack([np.full(len(pts), rt, np.uint8), up(st[1][pts], True), up(st[2][pts], bool(rt & DIF)),
                         up(st[3][pts], bool(rt & GLS)), up(st[4][pts], bool(rt & RFR))])
        np.testing.assert_array_equal(got, want, str(rt))
        assert got.shape[1] == q.count and (want[1] == 255).any()
    # rays == 0 launches nothing: the planes keep what they held
    keep = T.RayState(*[torch.full((4,), 7, dtype=torch.uint8, device=gpu.torch_device) for _ in range(5)])
    T.advance_state(gpu, q, parent, GLS, out=keep, rays=0)
    assert all(bool((getattr(keep, k) == 7).all()) for k in T.RayState.PLANES)
    # and the advanced state shades: the glossy rays' hits are glossy secondary points, off camera
    assert not (host(T.advance_state(gpu, q, parent, GLS).ray_type) & CAM).any()


# ---- 6. chunks, graphs, parameters -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, (1 << 36) + 5])
@pytest.mark.parametrize("node", NODES)
def test_two_chunks_with_first_index_are_the_whole_batch(gpu, oracle, T, node, first):
    _, lights = _lights(oracle)
    n, spp_n, cut = 700, 3, 333
    whole = Bounce(T, gpu, oracle, node, n, full=n)
    _, state = whole.state()
    nq = whole.bounce(lights, spp_n, state, DEPTHS, first=first)
    planes = _random_planes(nq)
    rf = _resolve(nq, [p.cuda() for p in planes])
    if first:
        base = whole.bounce(lights, spp_n, state, DEPTHS)
        assert not _bytes_equal(host(base.shadow._dir[:, :64]), host(nq.shadow._dir[:, :64]))      # the index reaches the scrambles
    names = ("shadow",) + nq.RAYS
    off = {r: host(getattr(nq, r).offsets).astype(np.int64) for r in names}
    hw = _queue_hosts(nq)
    for a, e in ((0, cut), (cut, n)):
        bc = Bounce(T, gpu, oracle, node, e - a, a=a, full=n)
        _, sc = bc.state()
        qc = bc.bounce(lights, spp_n, sc, DEPTHS, first=first + a)
        hc, sub = _queue_hosts(qc), []
        for j, r in enumerate(names):
            lo, hi = int(off[r][a]), int(off[r][e])
            np.testing.assert_array_equal(hc[r]["offsets"], off[r][a:e + 1] - lo)
            for k in hc[r]:
                if k not in ("offsets", "count", "point"):
                    assert _bytes_equal(hc[r][k], hw[r][k][..., lo:hi]), (node, a, r, k)
            sub.append(planes[j][:, lo:max(hi, lo + 1)].contiguous().cuda())
        _same(_resolve(qc, sub), {q: v[:, a:e] for q, v in rf.items()}, (node, a, e, "chunk"))


@pytest.mark.parametrize("node", NODES)
def test_emit_and_resolve_replay_in_a_graph(oracle, T, node):
    _, lights = _lights(oracle)
    n, spp_n = 700, 3
    gctx = R.Context(0, use_torch_stream=False)          # the context's own stream: the NULL stream cannot be captured
    try:
        b = Bounce(T, gctx, oracle, node, n)
        _, state = b.state()
        torch.cuda.synchronize()
        direct = b.bounce(lights, spp_n, state, DEPTHS)
        gctx.synchronize()
        cnt = direct.counts()
        planes = [p.cuda() for p in _random_planes(direct)]
        torch.cuda.synchronize()
        want = direct.resolve(*planes)
        gctx.synchronize()
        want, hq = {q: host(v) for q, v in want.items()}, _queue_hosts(direct)
        nq = (T.GgxNodeQueues if node == "ggx" else T.DisneyNodeQueues)(gctx, n, len(lights), spp_n, True)
        out = {q: gctx.empty(3, n) for q in want}
        torch.cuda.synchronize()
        with gctx.capture() as g:
            b.bounce(lights, spp_n, state, DEPTHS, queues=nq)
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
        _same_queues(_queue_hosts(nq), hq, (node, "replay"))
        _same({q: host(v) for q, v in out.items()}, want, (node, "replay"))
    finally:
        gctx.close()


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("node", NODES)
def test_mixed_state_with_uniform_parameters_and_by_reference(gpu, oracle, T, node, fast):
    """the closure's parameters as uniform values, and as per-material columns behind an index (trace_util's inputs); rlDisney's
    scales follow: two values, or two columns read through the closure's materials index"""
    from gpu_util import disney_sampler, ggx_sampler
    from trace_util import disney_inputs, ggx_inputs
    _, lights = _lights(oracle)
    n, spp_n = 257, 3
    gpu.set_math_mode(fast)
    try:
        for kind in ("uniform", "materials"):
            b = Bounce(T, gpu, oracle, node, n)
            if node == "ggx":
                c, _, mat = ggx_inputs(kind, n)
                if mat is None:
                    b.s = ggx_sampler(gpu, c)
                    b.sh = dict(KdColor=(0.7, 0.5, 0.2), Kd=0.8, diffuseRoughness=0.3, Ks=0.6, KtColor=(0.2, 0.9, 0.7), Kt=0.5)
                    b.shh = {q: np.broadcast_to(np.asarray(v, np.float32).reshape(-1, 1) if np.ndim(v) else np.float32(v),
                                                (3, n) if np.ndim(v) else (n,)) for q, v in b.sh.items()}
                else:
                    m = mat[1]
                    ids = host(mat[0]).astype(np.int64)
                    u = lambda j: oracle.gen_uniform(SEED_IN, 0, m, 900 + j)
                    u3 = lambda j: np.stack([oracle.gen_uniform(SEED_IN, 0, m, j + i) for i in range(3)])
                    kt = u(4)
                    kt[1] = 0.0                                     # one material without transmission
                    cols = dict(KdColor=u3(910), Kd=u(0), diffuseRoughness=u(1), Ks=u(2), KtColor=u3(920), Kt=kt)
                    b.s = R.GgxSampler(gpu, dev(c["wo"]), dev(c["N"]), dev(c["T"]), specColor=dev(c["KsColor"]), ior=dev(c["ior"]),
                                       roughness=dev(c["roughness"]), anisotropic=dev(c["anisotropic"]), materials=mat)
                    b.sh = {q: dev(v) for q, v in cols.items()}
                    b.shh = {q: np.ascontiguousarray(v[..., ids]) for q, v in cols.items()}
            else:
                c, mat = disney_inputs(kind, n)
                if mat is None:
                    b.s = disney_sampler(gpu, c)
                    b.scales, b.scales_h = [0.25, 0.75], [np.full(n, 0.25, np.float32), np.full(n, 0.75, np.float32)]
                else:
                    m, ids = mat[1], host(mat[0]).astype(np.int64)
                    sc = {k: dev(c[k]) for k in R._capi.DISNEY_SCALARS if k in c}
                    b.s = R.DisneySampler(gpu, dev(c["wo"]), dev(c["N"]), dev(c["T"]), base_color=dev(c["base_color"]),
                                          materials=mat, **sc)
                    cols = [oracle.gen_uniform(SEED_IN, 0, m, 930 + j) for j in range(2)]
                    cols[0][0], cols[1][0] = 0.0, 1.0
                    b.scales, b.scales_h = [dev(v) for v in cols], [np.ascontiguousarray(v[ids]) for v in cols]
            _assert_selection(b, lights, spp_n, what=(kind, fast))
    finally:
        gpu.set_math_mode(False)


def test_argument_checks_on_the_device_path(gpu, oracle, T):
    _, lights = _lights(oracle)
    b = Bounce(T, gpu, oracle, "ggx", 64)
    _, state = b.state()
    nq = b.bounce(lights, 2, state, DEPTHS)
    short = T.RayState.camera(gpu, 63)
    with pytest.raises(ValueError):
        b.bounce(lights, 2, short, DEPTHS, queues=nq)
    nq.spp_n = 17
    with pytest.raises(R.RlsError):
        b.bounce(lights, 17, state, DEPTHS, queues=nq)
    assert R.load().rls_last_error().decode().startswith("rls_trace_ggx_bounce_emit: spp_n")
    # n == 0: empty queues
    e = Bounce(T, gpu, oracle, "ggx", 1)
    e.s.n = 0
    q0 = T.GgxNodeQueues(gpu, 0, 2, 2)
    for r in ("shadow",) + q0.RAYS:
        getattr(q0, r).offsets.fill_(-1)
    T.ggx_bounce_rays(e.s, T.ggx_shader(e.s), None, lights, 2, SEED, T.RayState.camera(gpu, 0), DEPTHS, queues=q0)
    assert all(v == 0 for v in q0.counts().values())
