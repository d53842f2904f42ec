"""helpers of the tests of the caller-traced shading of rlSss's probe hits (test_gpu_trace_hits.py): synthetic hit lists that
exercise every branch of the gate, the gate and the library's stand-in tangent restated in numpy float32, the queues on the
host, the resolve composed on the host in the documented order."""
import numpy as np

import oracle_lib as O
from trace_lights_util import BSDF, DIFFUSE, LIGHT_MASK, compose
from trace_sss_util import EPS, INV_PI, _length, sphere_case

F = np.float32


def _unit(v):
    return (v / np.linalg.norm(v, axis=0, keepdims=True)).astype(F)


def tangent_np(N):
    """the library's tangent at a hit without hitT (include/rlshaders_amd_trace.h), in float32, operation by operation"""
    N = N.astype(F)
    sg = np.copysign(F(1), N[2]).astype(F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = (F(-1) / (sg + N[2]).astype(F)).astype(F)
        b = ((N[0] * N[1]).astype(F) * a).astype(F)
        x = (F(1) + (((sg * N[0]).astype(F) * N[0]).astype(F) * a).astype(F)).astype(F)
        return np.stack([x, (sg * b).astype(F), ((-sg) * N[0]).astype(F)])


def orthogonal_tangent(N, seed):
    """some unit tangent orthogonal to every (non-zero) N, float32"""
    rng = np.random.default_rng(seed)
    t0 = rng.standard_normal(N.shape)
    n = N.astype(np.float64)
    nn = np.maximum((n * n).sum(axis=0, keepdims=True), 1e-30)
    t = t0 - n * (n * t0).sum(axis=0, keepdims=True) / nn
    return _unit(t)


def synthetic_hits(n, spp, max_hits, stride, seed=3, dense=False):
    """shading points on the sphere of trace_sss_util.sphere_case and a hit list no tracer makes, with every branch of the gate:
    counts of 0 and above max_hits, hits past maxRadius, duplicates of the previous hit and of the shading point within
    AI_EPSILON, normals the cavity fade shuts.  Every element of the planes -- listed or not, and the padding past the rays --
    holds a usable position and unit normal, so that a reference may be run over all of them.  dense: every ray reports
    max_hits distinct hits within the radius (the list's length is then exactly rays * max_hits, fade off).
    -> (case, count uint8 [stride], hitP, hitN [3, max_hits, stride])"""
    case = sphere_case(n)
    rng = np.random.default_rng(seed)
    pt = np.minimum(np.arange(stride) // spp, n - 1)
    Po, No = case["P"][:, pt], case["N"][:, pt]
    maxR = (np.maximum(case["dist"][0], np.maximum(case["dist"][1], case["dist"][2])).astype(F) * F(3))[pt]
    cnt = rng.integers(0, max_hits + 3, stride).astype(np.uint8)
    cnt[rng.random(stride) < 0.15] = 0
    hP = np.zeros((3, max_hits, stride), F)
    hN = np.zeros((3, max_hits, stride), F)
    for k in range(max_hits):
        d = _unit(rng.standard_normal((3, stride)))
        u = rng.random(stride).astype(F)
        mag = ((F(0.05) + F(0.85) * u) * maxR).astype(F) if dense else (u * F(1.4) * maxR + F(0.01)).astype(F)
        hP[:, k] = (Po + d * mag).astype(F)
        hN[:, k] = _unit(rng.standard_normal((3, stride)))
    if dense:
        cnt[:] = max_hits
        return case, cnt, hP, hN
    j = np.arange(stride)
    if max_hits > 1:
        dup = j % 3 == 0                                     # slot 1 repeats slot 0 within AI_EPSILON
        hP[:, 1, dup] = (hP[:, 0, dup] + F(3e-5)).astype(F)
    at_p = j % 7 == 1                                        # slot 0 repeats the shading point itself
    hP[:, 0, at_p] = (Po[:, at_p] + F(2e-5)).astype(F)
    # on the normal's side, facing away: the fade is 0 (a normal a thousandth too long, so that N . No is below -1 and clamped
    # in either math mode, not within an ulp of -1)
    shut = j % 5 == 2
    hP[:, 0, shut] = (Po[:, shut] + No[:, shut] * (F(0.3) * maxR[shut])).astype(F)
    hN[:, 0, shut] = (No[:, shut] * F(-1.001)).astype(F)
    return case, cnt, hP, hN


def gate_np(case, spp, cnt, hP, hN, max_hits, cavity):
    """which slots rls_trace_sss_scatter_resolve counts as shaded, restated: bool [max_hits, rays]"""
    n = case["P"].shape[1]
    rays = n * spp
    pt = np.arange(rays) // spp
    Po = case["P"][:, pt]
    dist = case["dist"].astype(F)
    maxR = (np.maximum(dist[0], np.maximum(dist[1], dist[2])) * F(3)).astype(F)[pt]
    c = np.minimum(cnt[:rays].astype(np.int64), max_hits)
    prev = Po.copy()
    keep = np.zeros((max_hits, rays), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(max_hits):
            hp = hP[:, k, :rays]
            moved = (k < c) & (_length((prev - hp).astype(F)) > EPS)
            prev = np.where(moved, hp, prev)
            d = (hp - Po).astype(F)
            keep[k] = moved & ~(_length(d) > maxR)
            if cavity and keep[k].any():
                m = keep[k]
                fade = O.cavity_fade(np.ascontiguousarray(d[:, m]), np.ascontiguousarray(hN[:, k, :rays][:, m]),
                                     np.ascontiguousarray(case["N"][:, pt[m]]))
                keep[k, np.flatnonzero(m)[~(fade > EPS)]] = False
    return keep


def listed_elements(keep, stride):
    """the list in its order: ray-major, slots ascending within a ray"""
    js, ks = np.nonzero(keep.T)
    return (ks.astype(np.int64) * stride + js).astype(np.int64)


def queues_host(hq):
    """HitQueues -> (shadow dict in trace_lights_util.queue_host's form over the hit_capacity list entries, diffuse dict,
    hit_element, hit_count)"""
    h = lambda t: t.detach().cpu().numpy()
    s, d = hq.shadow, hq.diffuse
    sc = hq.shadow_count
    wd = h(s["weight_diffuse"])
    sh = dict(offsets=h(hq.shadow_offsets).astype(np.int64), dir=h(s["dir"]), maxdist=h(s["maxdist"]),
              ws=np.zeros((3, sc), F), wd=np.ascontiguousarray(np.broadcast_to(wd, (3, sc))), kind=h(s["kind"]).astype(np.int64),
              point=h(s["point"]).astype(np.int64), sample=h(s["sample"]).astype(np.int64), count=sc)
    df = dict(offsets=h(hq.diffuse_offsets).astype(np.int64), dir=h(d["dir"]), weight=h(d["weight"])[0] if hq.trace_diffuse
              else np.zeros(0, F), point=h(d["point"]).astype(np.int64), count=hq.diffuse_count)
    return sh, df, h(hq.hit_element).astype(np.int64), hq.hit_count


def compose_E(sh, df, elements, shape, vis, rad_lights, hit_spp, radiance=None, dtype=F):
    """rls_trace_sss_hits_resolve on the host in `dtype`: direct = the light loop's diffuse sum (trace_lights_util.compose, no
    tail; black without lights), E = direct + (radiance * weight) * AI_ONEOVERPI where the hit has a diffuse ray; 0 elsewhere"""
    listed = len(elements)
    E = np.zeros((3, shape[0] * shape[1]), dtype)
    if len(rad_lights):
        direct = compose(sh, vis, rad_lights, hit_spp, dtype=dtype)[0][:, :listed]
    else:
        direct = np.zeros((3, listed), dtype)
    direct = direct.astype(dtype).copy()
    if radiance is not None and df["count"]:
        r = np.arange(df["count"])
        p = df["point"]
        with np.errstate(invalid="ignore", over="ignore"):
            t = ((radiance[:, r].astype(dtype) * df["weight"].astype(dtype)[None, :]).astype(dtype) * dtype(INV_PI)).astype(dtype)
            direct[:, p] = (direct[:, p] + t).astype(dtype)
    E[:, elements] = direct
    return E.reshape(3, *shape)


def shadow_keys(sh, elements=None):
    """(element or point, light, segment 0 / 1, sample) of every ray, as one sortable integer"""
    who = sh["point"] if elements is None else elements[sh["point"]]
    return ((who * 8 + (sh["kind"] & LIGHT_MASK)) * 2 + ((sh["kind"] & BSDF) != 0)) * 256 + sh["sample"]

