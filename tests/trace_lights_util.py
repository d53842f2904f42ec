"""helpers shared by the tests of the caller-traced light loops (test_gpu_trace_lights.py): the queue on the host, the
resolve composed in numpy float32 in the documented order, the cone tests of the light restated on the host."""
import numpy as np

LIGHT_MASK, BSDF, SPECULAR, DIFFUSE = 0x07, 0x08, 0x10, 0x20          # RLS_SHADOW_*


def queue_host(q):
    """ShadowQueue -> dict of numpy arrays over its `count` rays; weight_diffuse broadcast to three planes (rlGgx has one)"""
    h = lambda t: t.detach().cpu().numpy()
    cnt = q.count
    wd = h(q._wd[:, :cnt])
    return dict(offsets=h(q.offsets).astype(np.int64), dir=h(q._dir[:, :cnt]), maxdist=h(q._maxdist[:cnt]),
                ws=h(q._ws[:, :cnt]), wd=np.ascontiguousarray(np.broadcast_to(wd, (3, cnt))),
                kind=h(q._kind[:cnt]).astype(np.int64), point=h(q._point[:cnt]).astype(np.int64),
                sample=h(q._sample[:cnt]).astype(np.int64), count=cnt)


def segment(kind):
    """0 the light-strategy samples, 1 the BSDF diffuse-lobe samples, 2 the BSDF specular-lobe samples"""
    return np.where(kind & BSDF, np.where(kind & DIFFUSE, 1, 2), 0)


def compose(h, vis, radiance, spp, dtype=np.float32, tail=None):
    """the resolve on the host, + and x only, in `dtype`: per point, light by light, the four sums (light or BSDF strategy x
    diffuse or specular lobe) grown in queue order by vis x weight over the rays that carry the term; then
    t = (radiance[l] * (light_sum + bsdf_sum)) * (1 / spp), the first light assigning.  radiance: [n_lights, 3].
    tail (rlGgx): (diffuse colour KdColor * Kd [3, n], Ks [n]) -> diffuse *= colour, specular *= Ks.
    -> (direct_diffuse [3, n], direct_specular [3, n])"""
    off, kind = h["offsets"], h["kind"]
    n, nl = len(off) - 1, len(radiance)
    pts = np.repeat(np.arange(n), np.diff(off))
    key = pts * 8 + (kind & LIGHT_MASK)
    vis = np.asarray(vis)[:, :h["count"]]
    with np.errstate(invalid="ignore", over="ignore"):
        ps = (vis.astype(dtype) * h["ws"].astype(dtype)).astype(dtype)
        pd = (vis.astype(dtype) * h["wd"].astype(dtype)).astype(dtype)
        inv = dtype(np.float32(1.0) / np.float32(spp))
        oD, oS = np.zeros((3, n), dtype), np.zeros((3, n), dtype)
        for l in range(nl):
            lo = np.searchsorted(key, np.arange(n) * 8 + l, "left")
            hi = np.searchsorted(key, np.arange(n) * 8 + l, "right")
            sums = {(b, lobe): np.zeros((3, n), dtype) for b in (0, 1) for lobe in "sd"}
            for j in range(int((hi - lo).max()) if n else 0):
                m = hi - lo > j
                r = (lo + j)[m]
                k = kind[r]
                for b in (0, 1):
                    for lobe, bit, prod in (("s", SPECULAR, ps), ("d", DIFFUSE, pd)):
                        take = (((k & BSDF) != 0) == bool(b)) & ((k & bit) != 0)
                        idx = np.flatnonzero(m)[take]
                        sums[(b, lobe)][:, idx] = sums[(b, lobe)][:, idx] + prod[:, r[take]]
            rad = np.asarray(radiance[l], dtype)[:, None]
            tS = (rad * (sums[(0, "s")] + sums[(1, "s")])) * inv
            tD = (rad * (sums[(0, "d")] + sums[(1, "d")])) * inv
            oS = tS if l == 0 else oS + tS
            oD = tD if l == 0 else oD + tD
        if tail is not None:
            colour, ks = tail
            oD = oD * np.asarray(colour, dtype)
            oS = oS * np.asarray(ks, dtype)[None, :]
    return oD.astype(dtype), oS.astype(dtype)


def assert_float64_bound(h, vis, radiance, spp, got, tail, what=""):
    """the resolve `got` (direct_diffuse, direct_specular) of the queue h under vis within the float64 rounding bound:
    one rounding per product and per addition over a light's k rays, two for the tail of a light, one per addition of a light, two
    for rlGgx's tail -> (k + 3 nl + 2) 2^-24 of the sum of magnitudes (test_gpu_trace_edges.py)"""
    e64 = compose(h, vis, radiance, spp, dtype=np.float64, tail=tail)
    habs = dict(h, ws=np.abs(h["ws"]), wd=np.abs(h["wd"]))
    mag = compose(habs, vis, np.abs(radiance), spp, dtype=np.float64,
                  tail=None if tail is None else (np.abs(tail[0]), np.abs(tail[1])))
    k = np.diff(h["offsets"]).astype(np.float64) + 3 * len(radiance) + 2
    for a in range(2):
        err = np.abs(got[a].astype(np.float64) - e64[a])
        bound = k * 2.0 ** -24 * mag[a] + 1e-30
        assert np.all(err <= bound), (what, a, "worst ratio", float((err / bound).max()))


def cone(center, radius, P):
    """float32, as the kernels' cone_make: d = center - P, c2 = |d|^2 - r^2"""
    f = np.float32
    d = (np.asarray(center, f)[:, None] - P.astype(f)).astype(f)
    dist2 = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]).astype(f)
    return d, (dist2 - f(radius) * f(radius)).astype(f)


def cone_hit(d, c2, dirs):
    """the kernels' cone_hit in float32: b = d . dir > 0 and not (b^2 - c2 |dir|^2 < 0)"""
    f = np.float32
    b = (d[0] * dirs[0] + d[1] * dirs[1] + d[2] * dirs[2]).astype(f)
    dd = (dirs[0] * dirs[0] + dirs[1] * dirs[1] + dirs[2] * dirs[2]).astype(f)
    return (b > 0) & ~((b * b).astype(f) - (c2 * dd).astype(f) < 0)


def near_hit_f64(center, radius, P, dirs):
    """float64: the near root t of |P + t dir - center| = radius for the emitted float32 directions, its discriminant
    (negative: the ray passes the sphere) and b = (center - P) . dir"""
    d = np.asarray(center, np.float64)[:, None] - P.astype(np.float64)
    u = dirs.astype(np.float64)
    b = (d * u).sum(axis=0)
    dd = (u * u).sum(axis=0)
    c2 = (d * d).sum(axis=0) - float(radius) ** 2
    disc = b * b - c2 * dd
    t = c2 / (b + np.sqrt(np.maximum(disc, 0.0)))
    return t, disc, b
