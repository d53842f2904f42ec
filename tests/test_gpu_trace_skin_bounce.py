"""GPU: the caller-traced rlSkin node at the hits of secondary rays (include/rlshaders_amd_trace.h, rls_trace_skin_bounce_emit /
rls_trace_skin_bounce_resolve; rlshaders_amd/trace.py, skin_bounce_rays).

  1. all-open: a camera state at depth 0 writes the node calls' bytes -- the five queues, their offsets, the three scalars, the
     AOVs and out -- and an empty diffuse_shadow: n = 1, 5, 67, kBlock + 1, 2049, spp_n 1, 2, 3, 16, 0 / 1 / 2 / 8 lights with
     mixed mis_modes, every lane-group width and the host's pick, EXACT and FAST, uniform parameters and parameters by reference,
     one shared scratch block, first_index 2^36 + 5;
  2. a per-point plan through the states of PLAN: every node queue is the node emit's queue filtered by the switches (offsets a
     host int64 cumsum); diffuse_shadow is rls_trace_ggx_direct_emit's diffuse-carrying rays at the derived seed on the diffuse
     rays' points; the scalars at Rr > 0 are the float32 sequential sum of the oracle's per-sample Fresnel over the lobe's
     light-loop BSDF samples (pairs 4 + 4 l / 6 + 4 l) divided by their count, exactly the weight without lights or under
     LIGHT_ONLY lights; 0, 0 and sss_weight past the glossy depth; +0 at a shadow ray's point;
  3. the resolve: at the diffuse rays' points under unit visibility sss = rls_ggx_direct_lighting's direct_diffuse (KdColor =
     sss_color, Kd = 1, diffuseRoughness 0, the derived seed) x sssWeight bit for bit; elsewhere under one env rls_skin_integrate's
     planes where the switches leave them whole, and everywhere the header's composition in numpy float32 from the queues; random
     coloured visibility and radiance over eight decades against that composition with the node resolve's float64 bound on the
     glossy sums (tests/test_gpu_trace_skin.py, _bound); a non-finite visibility in diffuse_shadow poisons its point alone; NaN
     probe hits at diffuse and shadow rays' points change nothing;
  4. chunked calls reproduce the whole, a captured graph of emit plus resolve replays the same bits, the Python layer refuses
     mismatched queues."""
import numpy as np
import pytest
import torch

import cases
import rlshaders_amd as R
import trace_sss_util as U
from gpu_util import dev, ggx_oracle, host
from test_gpu_shade import LIGHTS as LIGHTS2
from test_gpu_trace_skin import (ENVS, EPS, KBLOCK, KEYS, MIXED3, ODD_LIGHTS, SEED, F, Skin, T, _at, _bound, _gated, _lights8,  # noqa: F401
                                 _mk_lights, _resolve, _same, _traced)

pytestmark = pytest.mark.gpu

DEPTHS = (8, 2, 2, 4)                    # total, diffuse, glossy, refraction
CAM, SHD, RFL, RFR, DIF, GLS = 0x01, 0x02, 0x04, 0x08, 0x20, 0x40
# (ray_type, Rr, Rr_diff, Rr_gloss, Rr_refr) per state; the plan cycles through them by point index
PLAN = (
    (CAM, 0, 0, 0, 0),                   # 0  camera
    (GLS, 1, 0, 1, 0),                   # 1  glossy at Rr = 1, Rr_gloss below the depth
    (RFL, 1, 0, 0, 0),                   # 2  reflected at Rr = 1
    (RFR, 1, 0, 0, 1),                   # 3  refracted at Rr = 1
    (DIF, 1, 1, 0, 0),                   # 4  diffuse
    (SHD, 1, 0, 0, 0),                   # 5  shadow
    (GLS, 2, 0, 2, 0),                   # 6  Rr_gloss at the depth: open
    (GLS, 3, 0, 3, 0),                   # 7  Rr_gloss above the depth: both lobes shut
    (GLS, 0, 0, 0, 0),                   # 8  Rr = 0 with a non-camera type: integrateGlossy runs
    (DIF, 1, 1, 0, 0),                   # 9  diffuse with sssWeight below AI_EPSILON (the parameters of _plan_params)
    (DIF, 2, 1, 3, 0),                   # 10 diffuse past the glossy depth
    (SHD | CAM, 0, 0, 0, 0),             # 11 the shadow bit wins
    (DIF, 1, 1, 0, 0),                   # 12 diffuse with a small sss_color (rlGgx's own gate would shut: no gate here)
)
NS = len(PLAN)


def _plan(n):
    k = np.arange(n) % NS
    st = np.array(PLAN, np.uint8)[k].T.copy()                    # [5, n]
    return k, st


def _plan_params(p, n, a=0):
    """the plan's parameters for points a .. a + n - 1"""
    k = (a + np.arange(n)) % NS
    p = dict(p)
    p["sss_weight"] = np.where(k == 9, F(5e-5), np.maximum(p["sss_weight"], F(0.05))).astype(F)
    p["sss_color"] = np.where((k == 12)[None, :], F(2e-5), p["sss_color"]).astype(F)
    p["sheen_weight"] = np.where(k % 2 == 0, np.maximum(p["sheen_weight"], F(0.01)), p["sheen_weight"]).astype(F)
    return p


def _open_params(p, n):
    """for a state of the caller's own: every sssWeight at or above AI_EPSILON"""
    p = dict(p)
    p["sss_weight"] = np.maximum(p["sss_weight"], F(0.05)).astype(F)
    return p


def _state(T, gpu, st):
    return T.RayState(*[torch.from_numpy(np.ascontiguousarray(st[j])).to(gpu.torch_device) for j in range(5)])


def _gates(st):
    rt, rr, rg = st[0].astype(int), st[1].astype(int), st[3].astype(int)
    lit = (rt & SHD) == 0
    sS = lit & (rg <= DEPTHS[2])
    return dict(lit=lit, sS=sS, first=rr == 0, dif=lit & ((rt & DIF) != 0))


def _bounce(T, b, lights, spp_n, state, seed=SEED, first=0, queues=None, share=False):
    return T.skin_bounce_rays(b.sk, b.P, lights, spp_n, seed, state, DEPTHS, first, queues=queues, share_scratch=share)


def _shadow_host(sq, specular=True):
    off = host(sq.offsets)
    c = int(off[-1])
    h = dict(offsets=off, dir=host(sq._dir[:, :c]), maxdist=host(sq._maxdist[:c]), kind=host(sq._kind[:c]),
             point=host(sq._point[:c]), sample=host(sq._sample[:c]))
    h["weight"] = host(sq._ws[:, :c]) if specular else host(sq._wd[:, :c])
    return h


def _ray_host(rq):
    off = host(rq.offsets)
    assert int(off[-1]) == rq.count
    return dict(offsets=off, dir=host(rq.dir), weight=host(rq.weight), point=host(rq.point), sample=host(rq.sample))


def _node_hosts(q):
    h = {}
    for name in ("sheen_shadow", "specular_shadow"):
        if getattr(q, name) is not None:
            h[name] = _shadow_host(getattr(q, name))
    for name in ("sheen_glossy", "specular_glossy"):
        h[name] = _ray_host(getattr(q, name))
    pq = q.probes
    h["probes"] = dict(offsets=host(pq.offsets), origin=host(pq.origin), dir=host(pq.dir), maxdist=host(pq.maxdist),
                       point=host(pq.point), sample=host(pq.sample))
    h["scalars"] = {k: host(getattr(q, k)) for k in ("sheenFresnel", "specularFresnel", "sssWeight")}
    return h


def _same_hosts(got, want, what):
    assert got.keys() == want.keys(), what
    for name in want:
        for plane, v in want[name].items():
            g = got[name][plane]
            assert g.shape == v.shape and g.dtype == v.dtype, (what, name, plane, g.shape, v.shape)
            assert g.tobytes() == v.tobytes(), (what, name, plane)


def _filtered(h, keep):
    """a CSR queue with the rays of the points where keep is False taken out: offsets a host int64 cumsum"""
    cnt = np.diff(h["offsets"]).astype(np.int64)
    rays = np.repeat(keep, cnt)
    out = {k: (v[..., rays] if k != "offsets" else None) for k, v in h.items()}
    out["offsets"] = np.concatenate([[0], np.cumsum(np.where(keep, cnt, 0), dtype=np.int64)]).astype(np.int64)
    return out


# ---- 1. all-open -----------------------------------------------------------------------------------------------------------------
def _all_open(T, gpu, b, lights, spp_n, first=0, share=False, what=None):
    node = b.emit(T, lights, spp_n, first=first, share=share)
    q = _bounce(T, b, lights, spp_n, T.RayState.camera(gpu, b.n), first=first, share=share)
    _same_hosts(_node_hosts(q), _node_hosts(node), (what, "queues"))
    if lights is not None:
        assert q.diffuse_shadow.count == 0 and not host(q.diffuse_shadow.offsets).any()
    else:
        assert q.diffuse_shadow is None
    hits = b.hits(node)
    env = ENVS[1]
    want = _resolve(b, node, _traced(gpu, node, env), hits)
    got = _resolve(b, q, _traced(gpu, q, env), hits, diffuse_visibility=None if lights is None else torch.ones(3, 1, device=gpu.torch_device))
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes(), (what, k)
    return node


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("n,spp_n,first", [(1, 16, 0), (5, 3, (1 << 36) + 5), (67, 2, 0), (KBLOCK + 1, 1, (1 << 36) + 5), (2049, 2, 3)])
def test_all_open_is_the_node_call(gpu, oracle, T, n, spp_n, first, fast):
    gpu.set_math_mode(fast)
    try:
        b = Skin(gpu, oracle, n, "plane", cavity=True)
        node = _all_open(T, gpu, b, _mk_lights(MIXED3), spp_n, first, share=n == 67, what=(n, spp_n, fast))
        if n >= 67:
            assert all(v > 0 for v in node.counts().values())
    finally:
        gpu.set_math_mode(False)


def test_all_open_at_every_group_width_and_light_count(gpu, oracle, T, monkeypatch):
    b = Skin(gpu, oracle, 131, "plane")
    for specs in (None, MIXED3[:1], LIGHTS2, _lights8(), ODD_LIGHTS):
        lights = _mk_lights(specs)
        for spp_n, g in ((4, 1), (4, 4), (4, 16), (8, 64), (3, 64), (5, None)):
            _at(monkeypatch, g, lambda: _all_open(T, gpu, b, lights, spp_n, share=g == 4, what=(specs is None, spp_n, g)))


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_all_open_uniform_parameters_and_parameters_by_reference(gpu, oracle, T, fast):
    n, m = 131, 7
    cols = {k: np.ascontiguousarray(np.asarray(v)[..., :m]) for k, v in cases.skin_mixed(cases.SEED_EDGE, 64)["params"].items()}
    ids = ((oracle.gen_uniform(cases.SEED_PARITY, 0, n, 77) * m).astype(np.uint32) % m).astype(np.int32)
    gpu.set_math_mode(fast)
    try:
        for name, preset in cases.SKIN_PRESETS.items():
            _all_open(T, gpu, Skin(gpu, oracle, 67, "plane", params=dict(preset)), _mk_lights(MIXED3), 3, what=name)
        _all_open(T, gpu, Skin(gpu, oracle, n, "plane", cavity=True, params=cols, materials=(ids, m)), _mk_lights(MIXED3), 3, 5,
                  what="materials")
    finally:
        gpu.set_math_mode(False)


# ---- 2. the plan: queues and scalars ------------------------------------------------------------------------------------------
class Planned:
    """n points of the plan on the plane, the node emit and the bounce emit of the same samples"""

    def __init__(self, T, gpu, oracle, n, specs, spp_n, first=0, seed=SEED, share=False, st=None, case=None):
        """st: another state than the plan's, [5, n] uint8 (k is then -1 everywhere); case: the caller's own points (Skin)"""
        self.n, self.spp_n, self.specs, self.first, self.seed = n, spp_n, specs, first, seed
        self.k, self.st = _plan(n)
        if st is not None:
            self.k, self.st = np.full(n, -1), np.ascontiguousarray(st, dtype=np.uint8)
        self.g = _gates(self.st)
        self.b = Skin(gpu, oracle, n, "plane", cavity=True, params=_plan_params if st is None else _open_params, case=case)
        self.lights = _mk_lights(specs)
        self.state = _state(T, gpu, self.st)
        self.node = T.skin_node_rays(self.b.sk, self.b.P, self.lights, spp_n, seed, first)
        self.q = _bounce(T, self.b, self.lights, spp_n, self.state, seed, first, share=share)
        self.T, self.gpu, self.oracle = T, gpu, oracle

    def ggx(self, KdColor=None):
        """the rlGgx closure and node parameters of the light loop diffuse_shadow stands for; KdColor: sss_color, or a colour"""
        wo, N, Tt = self.b.frame
        s = R.GgxSampler(self.gpu, dev(wo), dev(N), dev(Tt), specColor=(0.5, 0.5, 0.5), ior=1.5, roughness=0.5)
        return s, dict(KdColor=dev(self.b.p["sss_color"]) if KdColor is None else KdColor, Kd=1.0, diffuseRoughness=0.0, Ks=0.5)


@pytest.fixture(scope="module")
def planned(gpu, oracle, T):
    return Planned(T, gpu, oracle, 20 * NS + 7, MIXED3, 3, first=(1 << 36) + 5)


def _assert_node_queues_filtered(w, same=_same_hosts):
    """every node queue of w.q is w.node's filtered by the state's switches -> (node hosts, bounce hosts, the walked points)"""
    g, hn, hq = w.g, _node_hosts(w.node), _node_hosts(w.q)
    for name in ("sheen_shadow", "specular_shadow"):
        same({name: hq[name]}, {name: _filtered(hn[name], g["sS"])}, name)
    for name in ("sheen_glossy", "specular_glossy"):
        same({name: hq[name]}, {name: _filtered(hn[name], g["sS"] & g["first"])}, name)
    # the probes: the node's rays; maxdist 0 at a shadow ray's, a diffuse ray's and a point of small sssWeight
    spp = w.spp_n ** 2
    for plane in ("offsets", "origin", "dir", "point", "sample"):
        assert hq["probes"][plane].tobytes() == hn["probes"][plane].tobytes(), plane
    walk = g["lit"] & ~g["dif"] & ~(hq["scalars"]["sssWeight"] < EPS)
    md, mdn = hq["probes"]["maxdist"].reshape(w.n, spp), hn["probes"]["maxdist"].reshape(w.n, spp)
    assert not md[~walk].any()
    both = walk & ~(hn["scalars"]["sssWeight"] < EPS)
    assert md[both].tobytes() == mdn[both].tobytes()
    return hn, hq, walk


def test_node_queues_are_the_node_emit_filtered_by_the_switches(planned):
    w = planned
    hn, hq, walk = _assert_node_queues_filtered(w)
    for name in ("sheen_glossy", "specular_glossy"):
        assert np.diff(hq[name]["offsets"])[w.k == 8].all() and not np.diff(hq[name]["offsets"])[w.k == 1].any()
    md = hq["probes"]["maxdist"].reshape(w.n, w.spp_n ** 2)
    assert md[walk].all() and walk[(w.k == 1) | (w.k == 7)].all()


def _assert_diffuse_shadow(w, same=_same_hosts):
    """w.q.diffuse_shadow against rls_trace_ggx_direct_emit's diffuse-carrying rays -> (its host planes, the points it serves)"""
    T = w.T
    s, shp = w.ggx((1.0, 1.0, 1.0))                             # a KdColor * Kd that is not small: sss_color does not gate the queue
    ref = T.ggx_shadow_rays(s, T.ggx_shader(s, **shp), w.b.P, w.lights, w.spp_n, w.seed ^ T.RLS_SKIN_DIFFUSE_SEED, w.first)
    r = _shadow_host(ref, specular=False)
    carries = (r["kind"] & T.RLS_SHADOW_DIFFUSE) != 0
    on = w.g["dif"] & ~(host(w.q.sssWeight) < EPS)
    keep = carries & on[r["point"].astype(np.int64)]
    cnt = np.bincount(r["point"].astype(np.int64)[keep], minlength=w.n).astype(np.int64)
    want = {k: v[..., keep] for k, v in r.items() if k != "offsets"}
    want["kind"] = (want["kind"] & ~np.uint8(T.RLS_SHADOW_SPECULAR)).astype(np.uint8)
    want["offsets"] = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)]).astype(np.int64)
    got = _shadow_host(w.q.diffuse_shadow, specular=False)
    same({"diffuse_shadow": got}, {"diffuse_shadow": want}, "diffuse_shadow")
    return got, on


def _view_below(b, n):
    """the first n points of b with the view mirrored below the plane"""
    wo = b.frame[0][:, :n].copy()
    wo[2] = -wo[2]
    return dict(wo=wo, N=b.frame[1][:, :n].copy(), T=b.frame[2][:, :n].copy(), P=b.Ph[:, :n].copy(),
                params={k: np.ascontiguousarray(np.asarray(v)[..., :n]) for k, v in b.p.items()})


def test_diffuse_shadow_is_the_ggx_direct_emit_at_the_derived_seed(planned):
    w, T = planned, planned.T
    got, on = _assert_diffuse_shadow(w)
    assert on[(w.k == 4) | (w.k == 10) | (w.k == 12)].all() and not on[w.k == 9].any() and not on[w.k == 5].any()
    assert got["offsets"][-1] > 0 and (got["kind"] & T.RLS_SHADOW_BSDF).any() and (~got["kind"] & T.RLS_SHADOW_BSDF).any()
    assert (np.diff(got["offsets"])[on] > 0).mean() > 0.9 and not np.diff(got["offsets"])[~on].any()
    below = Planned(T, w.gpu, w.oracle, 2 * NS, w.specs, 2, case=_view_below(w.b, 2 * NS))
    assert not np.diff(_assert_diffuse_shadow(below)[0]["offsets"]).any()     # a view below the horizon: the lobe is 0


def _loop_fresnel(oracle, b, specs, spp_n, seed, first, P):
    """per lobe the float32 running sum of the oracle's per-sample Fresnel over the light loops' BSDF samples -- lights
    ascending, samples ascending -- and their count: (sum [n], count [n]) by lobe name"""
    wo, N, Tt = b.frame
    n, spp = b.n, spp_n * spp_n
    out = {}
    for lobe, base in (("sheen", 4), ("specular", 6)):
        case = dict(wo=wo, N=N, T=Tt, KsColor=b.p[lobe + "_color"], ior=b.p[lobe + "_ior"], roughness=b.p[lobe + "_roughness"],
                    anisotropic=np.zeros(n, F))
        og = ggx_oracle(oracle, case)
        acc, cnt = np.zeros(n, F), np.zeros(n, F)
        draws = b.p[lobe + "_weight"] > EPS
        for l, s in enumerate(specs or ()):
            d = np.asarray(s["center"], np.float64)[:, None] - P.astype(np.float64)
            valid = (d * d).sum(0) - float(s["radius"]) ** 2 > 1e-3      # (the test's lights are far from or well around P)
            assert (np.abs((d * d).sum(0) - float(s["radius"]) ** 2) > 1e-3).all()
            if s["mis_mode"] == 1:                                       # RLS_MIS_LIGHT_ONLY: no BSDF sample
                continue
            for smp in range(spp):
                rx, ry = oracle.batch_sample_02(seed, first, n, base + 4 * l, smp)
                _, fr = og.sample(rx, ry)
                m = draws & valid
                acc = np.where(m, (acc + fr).astype(F), acc).astype(F)
                cnt = np.where(m, cnt + F(1), cnt).astype(F)
        out[lobe] = (acc, cnt)
    return out


def _expected_scalars(oracle, w, hn):
    """the three scalars the plan's switches leave, from the node emit's (first) or the oracle's light-loop Fresnel (!first)"""
    b, g, n = w.b, w.g, w.n
    loops = _loop_fresnel(oracle, b, w.specs, w.spp_n, w.seed, w.first, b.Ph)
    fres = {}
    for lobe in ("sheen", "specular"):
        acc, cnt = loops[lobe]
        weight = np.asarray(b.p[lobe + "_weight"], F) * np.ones(n, F)
        with np.errstate(divide="ignore", invalid="ignore"):
            avg = np.where(cnt > 0, (acc / cnt).astype(F), F(1)).astype(F)
        later = np.where(weight > EPS, (avg * weight).astype(F), F(0)).astype(F)
        fres[lobe] = np.where(g["first"], hn["scalars"][lobe + "Fresnel"], later).astype(F)
        fres[lobe] = np.where(g["sS"], fres[lobe], F(0)).astype(F)
    sw = (np.asarray(b.p["sss_weight"], F) * (F(1) - (fres["specular"] * (F(1) - fres["sheen"]).astype(F)).astype(F)).astype(F)).astype(F)
    sw = np.where(g["lit"], sw, F(0)).astype(F)
    return dict(sheenFresnel=fres["sheen"], specularFresnel=fres["specular"], sssWeight=sw)


def test_scalars_follow_the_switches(planned, oracle):
    w = planned
    hn, hq = _node_hosts(w.node), _node_hosts(w.q)
    want = _expected_scalars(oracle, w, hn)
    later = w.g["sS"] & ~w.g["first"]
    assert later.sum() > 5 * 20 and (want["sheenFresnel"][later] != hn["scalars"]["sheenFresnel"][later]).mean() > 0.5
    for k, v in want.items():
        got = hq["scalars"][k]
        print(k, "max |got - want| at Rr > 0:", float(np.abs(got[later] - v[later]).max()))
        assert got.tobytes() == v.tobytes(), (k, np.flatnonzero(got.view(np.uint32) != v.view(np.uint32))[:8])
    shadow = ~w.g["lit"]
    for k in want:                                               # +0: the sign bit too
        assert not hq["scalars"][k][shadow].view(np.uint32).any(), k
    shut = w.g["lit"] & ~w.g["sS"]
    assert not hq["scalars"]["sheenFresnel"][shut].any() and not hq["scalars"]["specularFresnel"][shut].any()
    assert hq["scalars"]["sssWeight"][shut].tobytes() == (np.asarray(w.b.p["sss_weight"], F) * np.ones(w.n, F))[shut].tobytes()


@pytest.mark.parametrize("specs", [None, [dict(s, mis_mode=1) for s in MIXED3[:2]]], ids=["no_lights", "light_only"])
def test_nothing_drawn_hands_down_exactly_the_weight(gpu, oracle, T, specs):
    w = Planned(T, gpu, oracle, 4 * NS, specs, 2)
    later = w.g["sS"] & ~w.g["first"]
    for lobe in ("sheen", "specular"):
        weight = np.asarray(w.b.p[lobe + "_weight"], F) * np.ones(w.n, F)
        want = np.where(weight > EPS, weight, F(0)).astype(F)
        assert host(getattr(w.q, lobe + "Fresnel"))[later].tobytes() == want[later].tobytes(), lobe
    assert later.sum() >= 16
    if specs is None:
        assert w.q.diffuse_shadow is None


# ---- 3. the resolve ------------------------------------------------------------------------------------------------------------------
def _light_part(sq, specs, vis, n, inv32):
    """lit [3, n] of a lobe's shadow queue: per light one float32 sum in queue order, (radiance * s) * inv added to +0"""
    off, kind, ws = host(sq.offsets), host(sq.kind), host(sq.weight_specular)
    out = np.zeros((3, n), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            for l, s in enumerate(specs):
                acc = np.zeros(3, F)
                for r in range(off[i], off[i + 1]):
                    if (kind[r] & 7) == l:
                        acc = (acc + (vis[:, r] * ws[:, r]).astype(F)).astype(F)
                out[:, i] = (out[:, i] + ((np.asarray(s["radiance"], F) * acc).astype(F) * inv32).astype(F)).astype(F)
    return out


def _diffuse_part(dq, specs, vis, n, inv32):
    """D [3, n] as rls_trace_sss_hits_resolve forms its direct term: four sums a light, the first light assigning"""
    off, kind, wd = host(dq.offsets), host(dq.kind), host(dq.weight_diffuse)[0]
    out = np.zeros((3, n), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            for l, s in enumerate(specs):
                lD, bD = np.zeros(3, F), np.zeros(3, F)
                for r in range(off[i], off[i + 1]):
                    if (kind[r] & 7) == l:
                        t = (vis[:, r] * wd[r]).astype(F)
                        if kind[r] & 0x08:
                            bD = (bD + t).astype(F)
                        else:
                            lD = (lD + t).astype(F)
                t = ((np.asarray(s["radiance"], F) * (lD + bD).astype(F)).astype(F) * inv32).astype(F)
                out[:, i] = t if l == 0 else (out[:, i] + t).astype(F)
    return out


def _composition(w, vis, rad, dvis, hits, got, uniform):
    """the header's composition on the host for the resolve `got` of w.q.  The light parts, D, the scatter part and out bit for
    bit; the lobes bit for bit where every glossy ray carries the radiance `uniform`, else within _bound about the light part"""
    b, q, g, n, spp = w.b, w.q, w.g, w.n, w.spp_n ** 2
    inv32 = F(1) / F(spp)
    hc, hP, hN, E = hits
    sF, sW = host(q.sheenFresnel), host(q.sssWeight)
    bc = np.asarray(b.p["sss_color"], F) * np.ones((3, n), F)
    D = _diffuse_part(q.diffuse_shadow, w.specs, dvis, n, inv32)
    case = dict(P=b.Ph, N=b.frame[1], T=b.frame[2], albedo=bc.copy(),
                dist=(np.asarray(b.p["sss_scatter_dist"], F).reshape(3, -1) * np.asarray(b.p["sss_dist_multiplier"], F)).astype(F)
                * np.ones((3, n), F))
    walk = g["lit"] & ~g["dif"] & ~(sW < EPS)
    rays = np.repeat(walk, spp)
    hc2 = np.where(rays, hc, 0).astype(hc.dtype)                 # (the resolve does not read the other points' hits)
    scat, _ = U.host_resolve(case, spp, hc2, np.nan_to_num(hP), np.nan_to_num(hN), np.nan_to_num(E), hP.shape[1], b.cavity, b.literal)
    with np.errstate(invalid="ignore", over="ignore"):
        sss = np.where(sW < EPS, F(0), np.where(g["dif"], ((bc * D).astype(F) * sW).astype(F), (scat * sW).astype(F))).astype(F)
    sss = np.where(walk | g["dif"], sss, F(0)).astype(F)
    U.same_bits_or_both_nan(got["sss"], sss, "sss")
    weight = {"sheen": np.asarray(b.p["sheen_weight"], F) * np.ones(n, F), "specular": np.asarray(b.p["specular_weight"], F) * np.ones(n, F)}
    W = {"sheen": weight["sheen"], "specular": (weight["specular"] * (F(1) - sF)).astype(F)}
    for name in ("sheen", "specular"):
        lit = _light_part(getattr(q, name + "_shadow"), w.specs, vis[name + "_shadow"], n, inv32)
        gq = getattr(q, name + "_glossy")
        off, wt = host(gq.offsets), host(gq.weight)
        L = None if rad is None else rad[name + "_glossy"]
        for i in range(n):
            r = slice(off[i], off[i + 1])
            if not g["sS"][i]:
                assert not got[name][:, i].view(np.uint32).any(), (name, i, "AI_RGB_BLACK")
                continue
            open_ = weight[name][i] > EPS
            if uniform is not None:
                A = np.zeros(3, F)
                for k in range(off[i], off[i + 1]):
                    A = (A + wt[:, k]).astype(F)
                S = ((A * inv32).astype(F) * (np.asarray(uniform, F) if off[i + 1] > off[i] else F(0))).astype(F)
                S = (S + (F(0) * inv32)).astype(F)
                want = (((lit[:, i] + S).astype(F) if open_ else np.zeros(3, F)) * W[name][i]).astype(F)
                assert got[name][:, i].tobytes() == want.tobytes(), (name, i, got[name][:, i], want)
            else:
                S = (L[:, r].astype(np.float64) * wt[:, r]).sum(1) / spp
                mag = (np.abs(L[:, r].astype(np.float64)) * np.abs(wt[:, r])).sum(1) / spp
                bS, u4 = _bound(off[i + 1] - off[i], 1.0, mag)
                want = (lit[:, i].astype(np.float64) + S) * W[name][i] if open_ else np.zeros(3)
                tol = abs(float(W[name][i])) * (bS + u4 * (np.abs(lit[:, i]) + mag)) * (1 + 2.0 ** -23)
                assert (np.abs(got[name][:, i] - want) <= tol).all(), (name, i, got[name][:, i], want, tol)
    U.same_bits_or_both_nan(got["out"], ((got["sheen"] + got["specular"]).astype(F) + got["sss"]).astype(F), "out")
    return D


def _unit(w, env):
    cnt = w.q.counts()
    tr = _traced(w.gpu, w.q, env, cnt)
    dvis = torch.ones(3, max(cnt["diffuse_shadow"], 1), device=w.gpu.torch_device)
    return cnt, tr, dvis


def test_unit_rays_under_the_plan(planned):
    w, T = planned, planned.T
    env = ENVS[1]
    cnt, tr, dvis = _unit(w, env)
    hits = w.b.hits(w.q)
    got = _resolve(w.b, w.q, tr, hits, diffuse_visibility=dvis)
    # the diffuse rays' points: rls_ggx_direct_lighting's diffuse AOV at the derived seed, x sssWeight
    s, shp = w.ggx()
    dd, _ = s.directLighting(w.b.P, w.lights, w.spp_n, w.seed ^ T.RLS_SKIN_DIFFUSE_SEED, first_index=w.first, **shp)
    sW = host(w.q.sssWeight)
    on = w.g["dif"] & (w.k != 12)
    want = np.where(sW < EPS, F(0), (host(dd) * sW).astype(F)).astype(F)
    assert (want[:, on & (w.k != 9)] > 0).mean() > 0.5 and not want[:, w.k == 9].any()
    U.same_bits_or_both_nan(got["sss"][:, on], want[:, on], "sss at the diffuse rays' points")
    assert (got["sss"][:, w.k == 12] > 0).any() and not host(dd)[:, w.k == 12].any()     # (no sampleDiffuse gate here)
    # the points the switches leave whole: rls_skin_integrate's planes
    whole = w.g["sS"] & w.g["first"] & ~w.g["dif"]
    ana = w.b.analytic(w.lights, w.spp_n, seed=w.seed, first=w.first, env=env)
    assert whole[(w.k == 0) | (w.k == 8)].all()
    for k in KEYS:
        U.same_bits_or_both_nan(got[k][..., whole], ana[k][..., whole], ("whole", k))
    # every point: the composition from the queues, bit for bit under one env
    vis = {k: np.ones((3, max(cnt[k], 1)), F) for k in ("sheen_shadow", "specular_shadow")}
    _composition(w, vis, None, np.ones((3, max(cnt["diffuse_shadow"], 1)), F), hits, got, env)
    # a shadow ray's point is +0 everywhere, the sign bit included
    for k in KEYS:
        assert not got[k][..., ~w.g["lit"]].view(np.uint32).any(), k


def test_random_visibility_and_radiance_and_garbage_hits(planned):
    w = planned
    cnt = w.q.counts()
    rng = np.random.default_rng(11)
    vis = {k: rng.random((3, cnt[k])).astype(F) for k in ("sheen_shadow", "specular_shadow")}
    dvis = rng.random((3, cnt["diffuse_shadow"])).astype(F)
    rad = {k: (rng.random((3, cnt[k])) * 10.0 ** rng.uniform(-4, 4, (3, cnt[k]))).astype(F) for k in ("sheen_glossy", "specular_glossy")}
    hc, hP, hN, E = w.b.hits(w.q)
    E = (E * rng.random(E.shape).astype(F)).astype(F)
    tr = (dev(vis["sheen_shadow"]), dev(vis["specular_shadow"]), dev(rad["sheen_glossy"]), dev(rad["specular_glossy"]))
    got = _resolve(w.b, w.q, tr, (hc, hP, hN, E), diffuse_visibility=dev(dvis))
    _composition(w, vis, rad, dvis, (hc, hP, hN, E), got, None)
    # probe hits at diffuse and shadow rays' points are not read
    skip = np.repeat(w.g["dif"] | ~w.g["lit"], w.spp_n ** 2)
    hc2, hP2, E2 = np.where(skip, np.uint8(255), hc).astype(np.uint8), hP.copy(), E.copy()
    hP2[:, :, skip] = np.nan
    E2[:, :, skip] = np.nan
    again = _resolve(w.b, w.q, tr, (hc2, hP2, hN, E2), diffuse_visibility=dev(dvis))
    for k in KEYS:
        assert again[k].tobytes() == got[k].tobytes(), k
    # a non-finite visibility in diffuse_shadow poisons its point's sss and out alone
    off = host(w.q.diffuse_shadow.offsets)
    i = int(np.flatnonzero((np.diff(off) > 0) & (w.k == 4))[3])
    bad = dvis.copy()
    bad[1, off[i]] = np.nan
    hurt = _resolve(w.b, w.q, tr, (hc, hP, hN, E), diffuse_visibility=dev(bad))
    others = np.arange(w.n) != i
    for k in KEYS:
        U.same_bits_or_both_nan(hurt[k][..., others], got[k][..., others], k)
    assert np.isnan(hurt["sss"][1, i]) and np.isnan(hurt["out"][1, i]) and np.isfinite(hurt["sss"][0, i])
    U.same_bits_or_both_nan(hurt["sheen"][:, i], got["sheen"][:, i], "sheen")


# ---- 4. chunks, graph replay, the Python layer's checks ---------------------------------------------------------------------
def test_chunked_calls_reproduce_the_whole(gpu, oracle, T):
    n, spp_n, first = 12 * NS, 3, (1 << 36) + 5
    lights = _mk_lights(MIXED3)
    _, st = _plan(n)
    mk = lambda a, m: Skin(gpu, oracle, m, "plane", cavity=True, a=a, full=n, params=lambda p, mm: _plan_params(p, mm, a))
    whole_b = mk(0, n)
    whole = _bounce(T, whole_b, lights, spp_n, _state(T, gpu, st), first=first)
    hw = _node_hosts(whole)
    hw["diffuse_shadow"] = _shadow_host(whole.diffuse_shadow, specular=False)
    parts, outs = [], []
    for a, m in ((0, 5 * NS + 3), (5 * NS + 3, n - 5 * NS - 3)):
        b = mk(a, m)
        q = _bounce(T, b, lights, spp_n, _state(T, gpu, st[:, a:a + m]), first=first + a)
        h = _node_hosts(q)
        h["diffuse_shadow"] = _shadow_host(q.diffuse_shadow, specular=False)
        parts.append(h)
        cnt, tr, dvis = _unit(Wrap(q, gpu), ENVS[1])
        outs.append(_resolve(b, q, tr, b.hits(q), diffuse_visibility=dvis))
    for name in ("sheen_shadow", "specular_shadow", "sheen_glossy", "specular_glossy", "diffuse_shadow"):
        for plane in ("dir", "weight", "sample"):
            cat = np.concatenate([p[name][plane] for p in parts], axis=-1)
            assert hw[name][plane].tobytes() == cat.tobytes(), (name, plane)
    for k in ("sheenFresnel", "specularFresnel", "sssWeight"):
        assert hw["scalars"][k].tobytes() == np.concatenate([p["scalars"][k] for p in parts]).tobytes(), k
    cnt, tr, dvis = _unit(Wrap(whole, gpu), ENVS[1])
    got = _resolve(whole_b, whole, tr, whole_b.hits(whole), diffuse_visibility=dvis)
    for k in KEYS:
        assert got[k].tobytes() == np.concatenate([o[k] for o in outs], axis=-1).tobytes(), k


class Wrap:
    def __init__(self, q, gpu):
        self.q, self.gpu = q, gpu


def test_graph_replay_of_emit_and_resolve(oracle, T):
    n, spp_n = 5 * NS + 2, 3
    gctx = R.Context(0, use_torch_stream=False)          # the context's own stream: the NULL stream cannot be captured
    try:
        w = Planned(T, gctx, oracle, n, MIXED3, spp_n, share=True)
        gctx.synchronize()
        cnt, tr, dvis = _unit(w, ENVS[1])
        hits = tuple(dev(h) for h in w.b.hits(w.q))
        torch.cuda.synchronize()
        want = w.q.resolve(*tr, *hits, diffuse_visibility=dvis, use_cavity_fade=True)
        gctx.synchronize()
        want = {k: host(v) for k, v in want.items()}
        out = {k: gctx.empty(3, n) for k in ("sheen", "specular", "sss", "out")}
        out.update({k: gctx.empty(n) for k in ("sheenFresnel", "specularFresnel", "sssWeight")})
        torch.cuda.synchronize()
        with gctx.capture() as graph:
            _bounce(T, w.b, w.lights, spp_n, w.state, queues=w.q)
            w.q.resolve(*tr, *hits, diffuse_visibility=dvis, use_cavity_fade=True, out=out, counts=cnt)
        for t in list(out.values()) + [w.q.sheenFresnel, w.q.specularFresnel, w.q.sssWeight, w.q.sheen_glossy.offsets,
                                       w.q.diffuse_shadow.offsets, w.q.probes.maxdist]:
            t.zero_()
        torch.cuda.synchronize()
        graph.launch()
        gctx.synchronize()
        _same({k: host(v) for k, v in out.items()}, want, "replay")
        assert int(w.q.diffuse_shadow.offsets[n].item()) == cnt["diffuse_shadow"] > 0
    finally:
        gctx.close()


def test_the_python_layer_refuses_what_does_not_fit(planned, gpu, oracle):
    w, T = planned, planned.T
    with pytest.raises(ValueError):
        _bounce(T, w.b, _mk_lights(MIXED3[:1]), w.spp_n, w.state, queues=w.q)        # another light count
    with pytest.raises(ValueError):
        _bounce(T, w.b, w.lights, w.spp_n, _state(T, gpu, _plan(w.n - 1)[1]))            # a state of fewer points
    cnt, tr, dvis = _unit(w, ENVS[1])
    with pytest.raises((ValueError, TypeError)):
        _resolve(w.b, w.q, tr, w.b.hits(w.q), diffuse_visibility=dvis[:, :1])          # fewer planes than rays
    node = T.skin_node_rays(w.b.sk, w.b.P, w.lights, w.spp_n, w.seed)
    assert not hasattr(node, "diffuse_shadow") and isinstance(w.q, T.SkinNodeQueues)
