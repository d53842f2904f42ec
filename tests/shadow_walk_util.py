"""helpers of the shadow walk's tests (test_shadow_walk_statement.py, test_gpu_shadow_walk*.py): shadow_walk_np, the float32 numpy
statement of rls_shadow_walk_begin / rls_shadow_walk_step (include/rlshaders_amd_shadow_walk.h), and two host tracers over
parallel planes and spheres built on walk_util's trace_plane_np / trace_sphere_np -- a nearest-hit tracer from a step's own origin
and maxdist that logs what every queue ray visited, and an all-hits tracer of the original rays.  pytest does not collect this
module."""
import numpy as np

from walk_util import length_np, trace_plane_np, trace_sphere_np

F = np.float32
TMIN = F(1e-3)                             # the tracers' self-hit guard: a root at or below it is the surface the ray stands on


class Found:
    """the nearest hit of every listed ray, host side: hit uint8 [m], t float32 [m], P float32 [3, m], opacity float32 [3, m] per
    entry -- or, with index int32 [m], a table [3, table_count]"""

    def __init__(self, hit, t, P, opacity, index=None):
        self.hit = np.array(hit, np.uint8, order="C")              # (copies: a broadcast view is not writable)
        self.t = np.array(t, F, order="C")
        self.P = np.array(P, F, order="C")
        self.opacity = np.array(opacity, F, order="C")
        self.index = None if index is None else np.array(index, np.int32, order="C")

    def entries(self, m):
        """the opacity of the first m entries, [3, m]"""
        if self.index is None:
            return self.opacity[:, :m]
        e = np.minimum(self.index[:m].astype(np.int64) & 0xFFFFFFFF, self.opacity.shape[1] - 1)
        return self.opacity[:, e]


class shadow_walk_np:
    """The statement of the walk.  After the constructor (rls_shadow_walk_begin) and after every step: ray, origin, dir, maxdist,
    steps are the active list, T [3, rays] the visibility planes; rays at or past the device count hold `fill`.  count: the value
    of the device count, None where there is none."""

    def __init__(self, O, point, dirs, maxdist, max_steps, base=None, via=None, count=None, fill=0.0):
        rays = maxdist.shape[0]
        R = rays if count is None else min(rays, max(int(count), 0))
        self.rays, self.walked, self.max_steps = rays, R, max_steps
        self.T = np.full((3, rays), fill, F)
        self.T[:, :R] = F(1) if base is None else np.asarray(base, F)[:, :R]
        with np.errstate(invalid="ignore"):
            active = maxdist[:R] > 0                               # a NaN is not active
        self.ray = np.flatnonzero(active).astype(np.uint32)
        src = np.asarray(point, np.int64)[self.ray.astype(np.int64)] & 0xFFFFFFFF
        if via is not None:
            src = np.asarray(via, np.int64)[src]
        self.origin = np.ascontiguousarray(np.asarray(O, F)[:, src])
        self.dir = np.ascontiguousarray(dirs[:, :R][:, active], F)
        self.maxdist = np.ascontiguousarray(maxdist[:R][active], F)
        self.steps = np.full(len(self.ray), max_steps, np.uint8)
        self.taken = 0

    @property
    def active(self):
        return len(self.ray)

    def step(self, found):
        m, j = self.active, self.ray.astype(np.int64)
        hit = found.hit[:m] != 0
        o = found.entries(m)
        steps = self.steps.astype(np.int64) - hit                  # a ray without a hit retires: its steps are not read again
        with np.errstate(invalid="ignore", over="ignore"):
            T = (self.T[:, j] * (F(1) - o).astype(F)).astype(F)
            left = (self.maxdist - found.t[:m]).astype(F)
            black = (T[0] == 0) & (T[1] == 0) & (T[2] == 0)
            s = hit & (steps > 0) & ~(left <= 0) & ~black
        self.T[:, j[hit]] = T[:, hit]
        self.ray = self.ray[s]
        self.origin = np.ascontiguousarray(found.P[:, :m][:, s])
        self.dir = np.ascontiguousarray(self.dir[:, s])
        self.maxdist = np.ascontiguousarray(left[s])
        self.steps = steps[s].astype(np.uint8)
        self.taken += 1
        return self


# ---- the tracers: parallel planes and spheres; surface s is plane s, then sphere s - len(planes) ---------------------------------
class Scene:
    """planes: [(point, normal)], spheres: [(center, radius)]"""

    def __init__(self, planes=(), spheres=()):
        self.planes, self.spheres = list(planes), list(spheres)

    @property
    def surfaces(self):
        return len(self.planes) + len(self.spheres)

    def roots(self, origin, dirs, maxdist):
        """every root of every ray in (TMIN, maxdist] -> (t [K, m] with inf where there is none, surface [K], P [3, K, m])"""
        m = origin.shape[1]
        ts, surf, Ps = [], [], []
        found = [(s, trace_plane_np(p, n, origin, dirs, maxdist)) for s, (p, n) in enumerate(self.planes)]
        found += [(len(self.planes) + s, trace_sphere_np(c, r, origin, dirs, maxdist)) for s, (c, r) in enumerate(self.spheres)]
        for s, (cnt, hP, _) in found:
            for k in range(hP.shape[1]):
                t = length_np((hP[:, k] - origin).astype(F))
                with np.errstate(invalid="ignore"):
                    ok = (k < cnt) & (t > TMIN)
                ts.append(np.where(ok, t, F(np.inf)).astype(F))
                surf.append(s)
                Ps.append(hP[:, k])
        if not ts:
            return np.full((1, m), np.inf, F), np.zeros(1, np.int64), np.zeros((3, 1, m), F)
        return np.stack(ts), np.asarray(surf, np.int64), np.stack(Ps, axis=1)


class nearest_tracer:
    """what a wavefront renderer has: the closest hit in (0, maxdist] from the step's own origin, t the distance from that origin
    to the hit, and the surface's opacity -- entry `surface` of `table` [3, surfaces], by index or per entry.  visited[j]: the
    surfaces queue ray j met, in order."""

    def __init__(self, scene, table, rays, indexed=True):
        self.scene, self.table, self.indexed = scene, np.ascontiguousarray(table, F), indexed
        self.visited = [[] for _ in range(rays)]

    def __call__(self, ray, origin, dirs, maxdist):
        t, surf, P = self.scene.roots(origin, dirs, maxdist)
        m = origin.shape[1]
        k = np.argmin(t, axis=0)
        at = np.arange(m)
        tn = t[k, at]
        hit = np.isfinite(tn)
        s = surf[k]
        for j, sj in zip(ray[hit].astype(np.int64), s[hit]):
            self.visited[j].append(int(sj))
        tn = np.where(hit, tn, F(0)).astype(F)
        Pn = np.where(hit, P[:, k, at], F(0)).astype(F)
        if self.indexed:
            return Found(hit, tn, Pn, self.table, index=s.astype(np.int32))
        return Found(hit, tn, Pn, self.table[:, s])

    def hits(self, max_hits=None):
        """the log as rls_shadow_hits reads it -> (count uint8 [rays], index uint32 [max_hits * rays], max_hits)"""
        rays = len(self.visited)
        K = max([len(v) for v in self.visited] + [1]) if max_hits is None else max_hits
        count = np.array([len(v) for v in self.visited], np.uint8)
        index = np.zeros((K, rays), np.uint32)
        for j, v in enumerate(self.visited):
            index[:len(v), j] = v
        return count, index.reshape(-1), K


def all_hits(scene, origin, dirs, maxdist):
    """every surface every ORIGINAL ray crosses in (TMIN, maxdist], nearest first -> (count [rays], surface [K, rays])"""
    t, surf, _ = scene.roots(origin, dirs, maxdist)
    order = np.argsort(t, axis=0, kind="stable")
    ts = np.take_along_axis(t, order, axis=0)
    return np.isfinite(ts).sum(axis=0), surf[order]


def run_np(w, tracer):
    """the walk to its end on the host -> the active count before every step"""
    counts = []
    while w.active and w.taken < w.max_steps:
        counts.append(w.active)
        w.step(tracer(w.ray, w.origin, w.dir, w.maxdist))
    return counts


# ---- the rules, each on a stream made for it: shared by the CPU statement test and the GPU test -----------------------------------
def _begin(n, maxdist=None, **kw):
    """n rays from the origin along +x, ray j of point j, reach 1"""
    d = dict(O=np.zeros((3, n), F), point=np.arange(n, dtype=np.int32), dirs=np.tile(np.array([[1.0], [0.0], [0.0]], F), (1, n)),
             maxdist=np.ones(n, F) if maxdist is None else np.asarray(maxdist, F), max_steps=4, base=None, count=None)
    d.update(kw)
    return d


def _found(m, opacity=0.0, t=0.25, hit=1, x=None):
    """m entries: opacity a scalar, [m] (every channel) or [3, m]; t and hit scalars or [m]"""
    o = np.broadcast_to(np.asarray(opacity, F), (3, m)) if np.ndim(opacity) < 2 else np.asarray(opacity, F)
    P = np.zeros((3, m), F)
    P[0] = np.arange(m) if x is None else x
    return Found(np.broadcast_to(np.asarray(hit, np.uint8), (m,)), np.broadcast_to(np.asarray(t, F), (m,)), P, o)


def rule_streams():
    """name -> (the arguments of shadow_walk_np, the Found of every step)"""
    one, nan, inf = F(1), F(np.nan), F(np.inf)
    s = {}
    # 1 in every channel ends the ray at T = +0; 1 in one channel does not; the third entry misses
    o = np.array([[1, 1, 0.5], [1, 0.25, 0.5], [1, 0.25, 0.5]], F)
    s["opaque"] = (_begin(3), [_found(3, o, hit=[1, 1, 0]), _found(1, 0.5)])
    # T = -0 in every channel ends the ray as +0 does (base -1 under an opacity of 1)
    s["minus_zero_T"] = (_begin(2, base=np.array([[-1, -1], [-1, 1], [-1, -1]], F)), [_found(2, 1.0), _found(0)])
    # no clamp: -0, +0, above 1, NaN, +inf, -inf propagate as the fold's operation gives them, and none of them ends a ray
    hostile = np.array([-0.0, 0.0, 1.5, nan, inf, -inf], F)
    s["hostile_opacity"] = (_begin(6), [_found(6, hostile), _found(6, 0.5), _found(6, hostile[::-1].copy())])
    # t: 0 and a negative t do not end a ray, a NaN left does not either
    s["t"] = (_begin(3), [_found(3, 0.25, t=np.array([0.0, -2.0, nan], F)), _found(3, 0.25, t=0.5)])
    # left one ulp either side of 0, and 0 itself
    t = np.array([np.nextafter(one, F(0)), one, np.nextafter(one, F(2))], F)
    s["left_ulp"] = (_begin(3), [_found(3, 0.25, t=t), _found(1, 0.25, t=0.0)])
    # the budget: a ray whose steps run out keeps the T it has
    for k in (1, 2, 255):
        s[f"budget_{k}"] = (_begin(2, max_steps=k), [_found(2, [0.0, 0.25], t=0.0)] * k)
    # begin: maxdist 0, negative and NaN are not listed and keep base
    base = np.arange(15, dtype=F).reshape(3, 5) * F(0.125)
    s["begin_maxdist"] = (_begin(5, maxdist=[0.0, -1.0, nan, 1.0, inf], base=base), [_found(2, 0.5)])
    # a device count below rays, above rays, negative
    for name, c in (("count_below", 3), ("count_above", 9), ("count_negative", -2)):
        s[name] = (_begin(5, count=c), [_found(5, 0.5)])
    # all lanes, one lane of every wavefront, no lane survive; then a last step that keeps the one lane of the last wavefront
    n = 3 * 64 + 5
    lane = (np.arange(n) % 64 == 7).astype(np.uint8)
    m = int(lane.sum())
    s["lanes"] = (_begin(n, max_steps=8), [_found(n, 0.125, t=0.0), _found(n, 0.125, t=0.0, hit=lane),
                                            _found(m, 0.125, t=0.0, hit=(np.arange(m) == m - 1).astype(np.uint8)),
                                            _found(1, 0.125, t=0.0, hit=0)])
    return s
