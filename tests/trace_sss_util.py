"""helpers of the -m gpu tests of the caller-traced rlSss integrator (test_gpu_trace_sss.py): the shading points on a plane
or a sphere, the probe rays traced on the host by the oracle's analytic scene (orc_scene_trace), the irradiance the
analytic integrator's light would give at each hit, and the resolve composed on the host from the oracle's NDProfile,
cavity fade and MIS pdf (orc_batch_nd_profile, orc_batch_sss_cavity_fade, orc_batch_sss_mis_pdf) with a float32 sequential
sum."""
import numpy as np

import cases
import oracle_lib as O

EPS = np.float32(1e-4)                     # AI_EPSILON
INV_PI = np.float32(0.318309886183790671538)   # AI_ONEOVERPI
MAX_HITS = 12                              # kMaxProbeDepth


def _unit(v):
    return (v / np.linalg.norm(v, axis=0)).astype(np.float32)


def sphere_case(n, radius=0.35, center=(0.3, -0.2, 0.1), bend=0.0, seed=cases.SEED_PARITY):
    """shading points on a sphere (the setting of test_gpu_scatter.py); `bend` tilts the shading normal"""
    _, G, T0 = cases.frame(seed, n)
    P = (np.asarray(center, np.float32)[:, None] + np.float32(radius) * G).astype(np.float32)
    Ns = _unit(G + np.float32(bend) * T0)
    T = _unit(np.cross(np.cross(Ns.T, T0.T), Ns.T).T)
    dist = np.stack([O.gen_uniform(seed, 0, n, O.S_PARAM0 + j, 0.02, 0.3) for j in range(3)])
    albedo = np.stack([O.gen_uniform(seed, 0, n, O.S_KS_R + j) for j in range(3)])
    return dict(P=P, N=Ns, T=T, dist=dist, albedo=albedo)


def plane_case(n, normal=(1.0, 2.0, 3.0), point=(0.5, -1.0, 0.25), seed=cases.SEED_EDGE):
    """shading points on a plane -> (case, the plane's unit normal)"""
    nrm = np.asarray(normal, np.float64)
    nrm /= np.linalg.norm(nrm)
    _, _, T0 = cases.frame(seed, n)
    T = T0 - nrm[:, None] * (nrm[:, None] * T0).sum(axis=0)
    T = (T / np.linalg.norm(T, axis=0)).astype(np.float32)
    B = np.cross(nrm, T.T).T
    ab = cases.xi(seed, n, 2) * 2 - 1
    P = (np.asarray(point, np.float64)[:, None] + ab[0] * T + ab[1] * B).astype(np.float32)
    Ns = np.ascontiguousarray(np.repeat(nrm.astype(np.float32)[:, None], n, axis=1))
    dist = np.stack([O.gen_uniform(seed, 0, n, O.S_PARAM0 + j, 0.02, 0.3) for j in range(3)])
    albedo = np.stack([O.gen_uniform(seed, 0, n, O.S_KS_R + j) for j in range(3)])
    return dict(P=P, N=Ns, T=T, dist=dist, albedo=albedo), nrm.astype(np.float32)


def trace_queue(scene, origin, dirs, maxdist, stride=None):
    """every probe ray through orc_scene_trace -> (count uint8 [rays], P [3, 2, stride], N [3, 2, stride]): hit k of ray j at
    [:, k, j], ascending t, as AiTraceProbe reports them to the integrator"""
    rays = origin.shape[1]
    stride = rays if stride is None else stride
    cnt = np.zeros(stride, np.uint8)
    hP = np.zeros((3, 2, stride), np.float32)
    hN = np.zeros((3, 2, stride), np.float32)
    for j in range(rays):
        k, _, hp, hn = O.scene_trace(scene, origin[:, j], dirs[:, j], maxdist[j])
        cnt[j] = k
        for m in range(k):
            hP[:, m, j] = hp[m]
            hN[:, m, j] = hn[m]
    return cnt, hP, hN


def trace_plane_np(plane_point, plane_normal, origin, dirs, maxdist):
    """orc_scene_trace of a plane, vectorised in float32 with the same operations in the same order (at most one hit)
    -> (count uint8, P [3, 1, rays], N [3, 1, rays])"""
    f = np.float32
    n = np.asarray(plane_normal, f)
    pp = np.asarray(plane_point, f)
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        denom = dot(n[:, None], dirs).astype(f)
        t = (dot(n[:, None], (pp[:, None] - origin).astype(f)) / denom).astype(f)
        ok = (denom != 0) & (t > 0) & (t <= maxdist)
        hp = (origin + dirs * t).astype(f)
    rays = origin.shape[1]
    hP = np.where(ok, hp, f(0))[:, None, :].astype(f)
    hN = np.where(ok, np.repeat(n[:, None], rays, axis=1), f(0))[:, None, :].astype(f)
    return ok.astype(np.uint8), np.ascontiguousarray(hP), np.ascontiguousarray(hN)


def trace_sphere_np(center, radius, origin, dirs, maxdist):
    """orc_scene_trace of a sphere, vectorised in float32 with the same operations in the same order (the two roots in
    ascending order, those in (0, maxdist] kept and packed to the front) -> (count uint8, P [3, 2, rays], N [3, 2, rays])"""
    f = np.float32
    c, rad = np.asarray(center, f), f(radius)
    dot = lambda a, b: ((a[0] * b[0] + a[1] * b[1]).astype(f) + a[2] * b[2]).astype(f)
    rays = origin.shape[1]
    cnt = np.zeros(rays, np.uint8)
    hP, hN = np.zeros((3, 2, rays), f), np.zeros((3, 2, rays), f)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        oc = (origin - c[:, None]).astype(f)
        a, b = dot(dirs, dirs), dot(oc, dirs)
        cc = (dot(oc, oc) - (rad * rad).astype(f)).astype(f)
        disc = ((b * b).astype(f) - (a * cc).astype(f)).astype(f)
        roots = ~(disc < 0) & (a != 0)
        sq = np.sqrt(disc).astype(f)
        for cand in (((-b - sq).astype(f) / a).astype(f), ((-b + sq).astype(f) / a).astype(f)):
            ok = roots & (cand > 0) & (cand <= maxdist)
            hp = (origin + (dirs * cand).astype(f)).astype(f)
            v = (hp - c[:, None]).astype(f)
            ln = np.sqrt(dot(v, v)).astype(f)
            inv = np.where(ln != 0, f(1) / ln, ln).astype(f)
            hn = (v * inv).astype(f)
            j = np.flatnonzero(ok)
            hP[:, cnt[j], j], hN[:, cnt[j], j] = hp[:, j], hn[:, j]
            cnt[j] += 1
    return cnt, hP, hN


def trace_np(scene, origin, dirs, maxdist):
    """orc_scene_trace of every ray, vectorised (trace_plane_np / trace_sphere_np by the scene's geometry)"""
    if scene.geometry == 0:
        return trace_plane_np(scene.plane_point[:], scene.plane_normal[:], origin, dirs, maxdist)
    return trace_sphere_np(scene.sphere_center[:], scene.sphere_radius, origin, dirs, maxdist)


def light_irradiance(scene, hP, hN):
    """E = light_color * (AI_ONEOVERPI * max(0, N.L)), 0 where the gate is shut: evalLightSample of the analytic scene
    before evalProfile and the fade (float32, the integrator's operations) -> [3, K, stride]"""
    f = np.float32
    L = np.asarray(scene.light_dir[:], f)
    lc = np.asarray(scene.light_color[:], f)
    d = (hN[0] * L[0] + hN[1] * L[1]) + hN[2] * L[2]
    w = (INV_PI * np.where(f(0) > d, f(0), d)).astype(f)
    if scene.has_gate:
        gp, gn = np.asarray(scene.gate_point[:], f), np.asarray(scene.gate_normal[:], f)
        g = ((hP[0] - gp[0]) * gn[0] + (hP[1] - gp[1]) * gn[1]) + (hP[2] - gp[2]) * gn[2]
        w = np.where(g > f(0), w, f(0)).astype(f)
    return np.stack([(lc[c] * w).astype(f) for c in range(3)])


def _length(v):
    return np.sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]).astype(np.float32)).astype(np.float32)


def host_resolve(case, spp, cnt, hP, hN, E, max_hits, cavity, literal, has_dPdu=True, nthreads=1):
    """rls_trace_sss_scatter_resolve composed on the host: the walk of every ray's hits in float32, the oracle's profile,
    cavity fade and MIS pdf for the hits that reach them, the terms summed per point in sample, then hit order
    -> (result [3, n], mean_depth [n])"""
    f = np.float32
    n = case["P"].shape[1]
    rays = n * spp
    pt = np.arange(rays) // spp
    Po = case["P"][:, pt]
    dist = case["dist"].astype(f)
    maxR = (np.maximum(dist[0], np.maximum(dist[1], dist[2])) * f(3)).astype(f)[pt]
    c = np.minimum(cnt[:rays].astype(np.int64), max_hits)
    prev = Po.copy()
    keep = np.zeros((max_hits, rays), bool)
    D = np.zeros((max_hits, 3, rays), f)
    R = np.zeros((max_hits, rays), f)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(max_hits):
            alive = k < c
            hp = hP[:, k, :rays]
            moved = alive & (_length((prev - hp).astype(f)) > EPS)
            prev = np.where(moved, hp, prev)
            d = (hp - Po).astype(f)
            r = _length(d)
            keep[k] = moved & ~(r > maxR)
            D[k], R[k] = d, r
    ks, js = np.nonzero(keep)                      # the hits that reach shadeProbeSample's fade
    if len(js):
        d, hn = D[ks, :, js].T.copy(), hN[:, ks, js].astype(f)
        fade = O.cavity_fade(d, hn, case["N"][:, pt[js]].copy()) if cavity else np.ones(len(js), f)
        shaded = fade > EPS
        ks, js, d, hn, fade = ks[shaded], js[shaded], d[:, shaded], hn[:, shaded], fade[shaded]
    else:
        shaded = np.zeros(0, bool)
    terms = np.zeros((max_hits, 3, rays), f)
    depth = np.zeros(rays, f)
    np.add.at(depth, js, f(1))
    if len(js):
        g = pt[js]
        o = O.Sss(len(js), case["dist"][:, g].copy(), case["albedo"][:, g].copy(), N=case["N"][:, g].copy(),
                  T=case["T"][:, g].copy(), has_dPdu=has_dPdu, nthreads=nthreads)
        prof = o.nd_profile(R[ks, js])
        with np.errstate(invalid="ignore", over="ignore"):
            irr = ((E[:, ks, js] * prof).astype(f) * fade).astype(f)
        nz = ~np.all(irr == 0, axis=0)
        pdf = np.ones(len(js), f)
        if nz.any():
            o2 = O.Sss(int(nz.sum()), case["dist"][:, g[nz]].copy(), case["albedo"][:, g[nz]].copy(),
                       N=case["N"][:, g[nz]].copy(), T=case["T"][:, g[nz]].copy(), has_dPdu=has_dPdu, nthreads=nthreads)
            pdf[nz] = o2.mis_pdf(d[:, nz].copy(), hn[:, nz].copy(), literal)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            t = np.where(nz, (irr / pdf).astype(f), f(0))
        terms[ks, :, js] = t.T
    acc = np.zeros((3, n), f)
    accD = np.zeros(n, f)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(spp):
            j = np.arange(n) * spp + s
            for k in range(max_hits):
                acc = (acc + terms[k][:, j]).astype(f)
            accD = (accD + depth[j]).astype(f)
        inv = f(1) / f(spp)
        res = ((case["albedo"].astype(f) * acc).astype(f) * inv).astype(f)
    return res, (accD * inv).astype(f)


def same_bits_or_both_nan(a, b, what=""):
    """bit equality, except that a NaN matches any NaN (the payload of a NaN is not part of the contract)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (what, "NaN positions differ", int((na != nb).sum()))
    d = (a.view(np.uint32) != b.view(np.uint32)) & ~na
    assert not d.any(), (what, "words differing", int(d.sum()), "of", d.size)
