"""helpers of the probe walk's tests (test_gpu_walk.py, test_gpu_walk_edges.py, test_walk_statement.py): walk_np, the float32
numpy statement of rls_walk_begin / rls_walk_step (include/rlshaders_amd_walk.h), and two host tracers over the analytic plane
and sphere of trace_sss_util -- a nearest-hit tracer from a step's own origin and maxdist, and a cumulative tracer that keeps
the original ray and hands out its roots one by one.  pytest does not collect this module."""
import numpy as np

from trace_sss_util import EPS, trace_plane_np, trace_sphere_np

TRIALS = 12                                # RLS_WALK_TRIALS
F = np.float32


def length_np(v):
    """sqrt((x x + y y) + z z) in float32"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(((v[0] * v[0] + v[1] * v[1]).astype(F) + v[2] * v[2]).astype(F)).astype(F)


def dot_np(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return ((a[0] * b[0] + a[1] * b[1]).astype(F) + a[2] * b[2]).astype(F)


class Found:
    """the nearest hit of every listed ray, host side: hit uint8 [m], t float32 [m], P, N, Ns float32 [3, m], object int32 [m] or None"""

    def __init__(self, hit, t, P, N, Ns, object=None):
        self.hit = np.ascontiguousarray(hit, np.uint8)
        self.t = np.ascontiguousarray(t, F)
        self.P, self.N, self.Ns = (np.ascontiguousarray(a, F) for a in (P, N, Ns))
        self.object = None if object is None else np.ascontiguousarray(object, np.int32)


class walk_np:
    """The statement of the walk.  After the constructor (rls_walk_begin) and after every step: ray, origin, dir, maxdist, trials
    are the active list, count / hP / hN the hits in rls_probe_hits' layout; slots never written hold `fill`."""

    def __init__(self, origin, dirs, maxdist, P, spp, own=None, max_hits=12, foreign="stop", point=None, fill=0.0, stride=None):
        rays = maxdist.shape[0]
        stride = rays if stride is None else stride
        self.rays, self.max_hits, self.foreign = rays, max_hits, foreign
        self.point = (np.arange(rays) // spp) if point is None else np.asarray(point, np.int64)
        self.P0 = np.ascontiguousarray(P, F)[:, self.point] if rays else np.zeros((3, 0), F)
        self.own = None if own is None else np.asarray(own, np.int32)[self.point]
        self.count = np.zeros(rays, np.uint8)
        self.hP = np.full((3, max_hits, stride), fill, F)
        self.hN = np.full((3, max_hits, stride), fill, F)
        with np.errstate(invalid="ignore"):
            active = maxdist > 0                                   # a NaN is not active
        self.ray = np.flatnonzero(active).astype(np.uint32)
        self.origin = np.ascontiguousarray(origin[:, active], F)
        self.dir = np.ascontiguousarray(dirs[:, active], F)
        self.maxdist = np.ascontiguousarray(maxdist[active], F)
        self.trials = np.full(len(self.ray), TRIALS, np.uint8)
        self.steps = 0

    @property
    def active(self):
        return len(self.ray)

    def step(self, found):
        m, j = self.active, self.ray.astype(np.int64)
        hit = found.hit[:m] != 0
        t, fP, fN, fNs = found.t[:m], found.P[:, :m], found.N[:, :m], found.Ns[:, :m]
        cnt = self.count[j].astype(np.int64)
        prev = np.where(cnt > 0, self.hP[:, np.maximum(cnt - 1, 0), j], self.P0[:, j])
        trials = self.trials.astype(np.int64) - hit                # a ray without a hit retires: its trials are not read again
        other = np.zeros(m, bool) if self.own is None else hit & (found.object[:m] != self.own[j])
        with np.errstate(invalid="ignore", over="ignore"):
            dist = length_np((prev - fP).astype(F))
            accepted = hit & ~other & (dist > EPS)
            left = np.where(accepted, (self.maxdist - t).astype(F), self.maxdist).astype(F)
            flip = dot_np(fN, fNs) < 0
        aligned = np.where(flip, -fNs, fNs).astype(F)
        a = np.flatnonzero(accepted)
        self.hP[:, cnt[a], j[a]] = fP[:, a]
        self.hN[:, cnt[a], j[a]] = aligned[:, a]
        self.count[j[a]] = (cnt[a] + 1).astype(np.uint8)
        with np.errstate(invalid="ignore"):
            s = hit & (trials > 0) & ~(left <= 0) & (cnt + accepted < self.max_hits)
        if self.foreign == "stop":
            s &= ~other
        self.ray = self.ray[s]
        self.origin = np.ascontiguousarray(fP[:, s])
        self.dir = np.ascontiguousarray(self.dir[:, s])
        self.maxdist = np.ascontiguousarray(left[s])
        self.trials = trials[s].astype(np.uint8)
        self.steps += 1
        return self


# ---- the tracers: the analytic plane (geometry 0) and sphere of trace_sss_util ---------------------------------------------------
def _scene_roots(scene, origin, dirs, maxdist):
    """every root of the rays in (0, maxdist], ascending -> (count, P [3, K, m], N [3, K, m]); scene: oracle_lib.make_scene's"""
    if scene.geometry == 0:
        return trace_plane_np(scene.plane_point[:], scene.plane_normal[:], origin, dirs, maxdist)
    return trace_sphere_np(scene.sphere_center[:], scene.sphere_radius, origin, dirs, maxdist)


class nearest_tracer:
    """what a wavefront renderer has: the closest hit in (0, maxdist] from the step's own origin; t is the distance from that
    origin to the hit"""

    def __init__(self, scene):
        self.scene = scene

    def __call__(self, ray, origin, dirs, maxdist):
        cnt, hP, hN = _scene_roots(self.scene, origin, dirs, maxdist)
        P, N = hP[:, 0], hN[:, 0]
        return Found(cnt > 0, length_np((P - origin).astype(F)), P, N, N)


class cumulative_tracer:
    """keeps the ORIGINAL ray of every queue entry: a query for queue ray j returns the next root of that ray beyond the last one
    it returned, t the difference of the two roots' distances from the original origin.  The roots are orc_scene_trace's of
    the whole ray -- the list trace_sss_util.trace_queue reports -- so the walk over this tracer visits exactly that list."""

    def __init__(self, scene, origin, dirs, maxdist):
        self.cnt, self.hP, self.hN = _scene_roots(scene, origin, dirs, maxdist)
        self.origin = origin
        self.given = np.zeros(len(maxdist), np.int64)
        self.last = np.zeros(len(maxdist), F)

    def __call__(self, ray, origin, dirs, maxdist):
        j = ray.astype(np.int64)
        k = self.given[j]
        hit = k < self.cnt[j]
        kk = np.minimum(k, self.hP.shape[1] - 1)
        P, N = self.hP[:, kk, j], self.hN[:, kk, j]
        far = length_np((P - self.origin[:, j]).astype(F))
        t = (far - self.last[j]).astype(F)
        self.given[j[hit]] += 1
        self.last[j[hit]] = far[hit]
        return Found(hit, t, P, N, N)


def run_np(w, tracer):
    """the walk to its end on the host -> the active count before every step"""
    counts = []
    while w.active and w.steps < TRIALS:
        counts.append(w.active)
        w.step(tracer(w.ray, w.origin, w.dir, w.maxdist))
    return counts
