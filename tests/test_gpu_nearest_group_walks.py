"""-m gpu: the walks through a group (nearest_group.tracer), with no host tracer between the device calls.

1. rlSss probe rays walked through TWO instances of one icosphere about the points, the second 1.15 times the first about the
   same centre (turned a little): count, P and N of the hits equal walk_np (tests/walk_util.py) over group_np bit for bit, the
   pair last / last_instance carried across the steps in both.  A ray that leaves triangle i of the inner instance meets the
   outer instance next, often in ITS triangle i (the two are nearly concentric): that hit must not be skipped -- the skip is the
   pair (instance, prim), never the prim alone.
2. rlGgx and rlDisney light-loop shadow rays walked under two overlapping translucent instances of one quad (surface bases 0 and
   1, the same two prim ids stacked over each other) and an opaque instance of a sphere (base 3): the visibility equals
   shadow_walk_np over group_np, rays behind the sphere are black, and the rays through both quads visited the same prim id in
   two instances."""
import numpy as np
import pytest
import torch

import cases
import nearest_group_util as G
import nearest_util as U
from nearest_util import F, NO_PRIM
from shadow_walk_util import Found as ShadowFound, shadow_walk_np
from shadow_walk_util import run_np as shadow_run_np
from test_gpu_nearest_group import DeviceGroup
from test_walk_statement import SEED, setting
from trace_sss_util import same_bits_or_both_nan
from walk_util import Found as WalkFound, run_np, walk_np

pytestmark = pytest.mark.gpu


def _host(t):
    return t.detach().cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx():
    import rlshaders_amd as R
    from rlshaders_amd import nearest_group, shadow_walk, walk
    walk.load(), shadow_walk.load(), nearest_group.load()           # (a missing library is an error, not a build)
    c = R.Context(0)
    yield c
    c.close()


class group_np_tracer:
    """nearest hits of a walk's list by group_np, the pair (last_instance, last) carried by queue ray across steps; log: every
    call's ids and Hits"""

    def __init__(self, insts, rays):
        self.insts, self.log = insts, []
        self.last, self.last_instance = np.full(rays, NO_PRIM, np.uint32), np.full(rays, G.NO_INSTANCE, np.uint32)

    def __call__(self, ray, origin, dirs, maxdist):
        j = np.asarray(ray).astype(np.int64)
        h = G.group_np(self.insts, origin, dirs, maxdist, (self.last_instance[j], self.last[j]))
        hit = h.hit != 0
        self.last[j[hit]], self.last_instance[j[hit]] = h.prim[hit], h.instance[hit]
        self.log.append((j.copy(), h))
        return h


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])


# ---- 1. the probe walk -----------------------------------------------------------------------------------------------------------------
class walk_tracer(group_np_tracer):
    def __call__(self, ray, origin, dirs, maxdist):
        h = super().__call__(ray, origin, dirs, maxdist)
        return WalkFound(h.hit, h.t, h.P, h.N, h.Ns)


@pytest.mark.parametrize("n,spp_n", [(22, 3), (67, 2)])
def test_probes_walked_through_two_instances(ctx, n, spp_n):
    import rlshaders_amd as R
    from rlshaders_amd import nearest_group, trace, walk
    case, _ = setting("sphere", n)
    P = case["P"]
    s = R.SssSampler(ctx, _dev(case["N"]), _dev(case["T"]), _dev(case["albedo"]), _dev(case["dist"]), has_dPdu=True)
    q = trace.sss_probe_rays(s, _dev(P), spp_n, SEED)
    origin, dirs, maxdist = _host(q.origin), _host(q.dir), _host(q.maxdist)
    centre = P.astype(np.float64).mean(axis=1)
    reach = float(np.median(maxdist[maxdist > 0])) if (maxdist > 0).any() else 1.0
    radius = float(np.linalg.norm(P.astype(np.float64).T - centre, axis=1).max()) + 0.15 * reach
    mesh = U.icosphere(2)
    insts = [G.Inst(mesh, G.affine(radius * np.eye(3), centre), base=0),
             G.Inst(mesh, G.affine(1.15 * radius * rot_z(0.01) @ np.diag([1.0, 1.02, 0.98]), centre), base=7)]
    g = DeviceGroup(ctx, insts)
    try:
        tracer = nearest_group.tracer(g.group)
        w = walk.run(q, _dev(P), tracer)
        wn = walk_np(origin, dirs, maxdist, P, spp_n * spp_n)
        tn = walk_tracer(insts, len(maxdist))
        counts = run_np(wn, tn)
        assert w.active == 0 and wn.active == 0 and len(counts) >= 2
        np.testing.assert_array_equal(_host(w.hit_count), wn.count)
        live = np.arange(wn.max_hits)[:, None] < wn.count[None, :]
        same_bits_or_both_nan(_host(w.hit_P)[:, live], wn.hP[:, live], "hits.P")
        same_bits_or_both_nan(_host(w.hit_N)[:, live], wn.hN[:, live], "hits.N")
        np.testing.assert_array_equal(_host(tracer.last).view(np.uint32)[:len(maxdist)], tn.last)
        np.testing.assert_array_equal(_host(tracer.last_instance).view(np.uint32)[:len(maxdist)], tn.last_instance)
        # a second step's rays start ON the triangle they hit: none meets (instance, prim) again, some meet the same prim id of
        # the OTHER instance
        (j0, h0), (j1, h1) = tn.log[0], tn.log[1]
        at = np.searchsorted(j0, j1)
        assert np.array_equal(j0[at], j1)
        same_prim = (h1.hit != 0) & (h1.prim == h0.prim[at])
        assert not np.any(same_prim & (h1.instance == h0.instance[at])) and np.any(same_prim & (h1.instance != h0.instance[at]))
        w2 = walk.run(q, _dev(P), tracer.reset())                    # the same tracer serves a second walk after reset()
        assert torch.equal(w2.hit_count, w.hit_count)
    finally:
        g.close()


# ---- 2. the shadow walk ----------------------------------------------------------------------------------------------------------------
def shadow_instances():
    quad = U.Mesh([(-20, -20, 0), (20, -20, 0), (20, 20, 0), (-20, 20, 0)], [(0, 1, 2), (0, 2, 3)], surface=[0, 0])
    ball = U.icosphere(2)
    ball.surface = np.zeros(ball.nt, np.uint32)
    return [G.Inst(quad, G.affine(rot_z(0.3) @ np.diag([1.5, 0.8, 1.0]), (0.5, -0.25, 1.2)), base=0),
            G.Inst(quad, G.affine(rot_z(0.3) @ np.diag([1.5, 0.8, 1.0]), (0.5, -0.25, 1.4)), base=1),
            G.Inst(ball, G.affine(0.3 * rot_z(1.0) @ np.diag([1.0, 1.2, 0.9]), (2.0, 2.0, 1.75)), base=3)]


@pytest.fixture(scope="module")
def T():
    from rlshaders_amd import trace
    trace.load()
    return trace


class shadow_tracer(group_np_tracer):
    def __init__(self, insts, rays, table):
        super().__init__(insts, rays)
        self.table, self.visited = table, [[] for _ in range(rays)]

    def __call__(self, ray, origin, dirs, maxdist):
        h = super().__call__(ray, origin, dirs, maxdist)
        hit = h.hit != 0
        for j, s, i, p in zip(np.asarray(ray).astype(np.int64)[hit], h.surface[hit], h.instance[hit], h.prim[hit]):
            self.visited[j].append((int(s), int(i), int(p)))
        return ShadowFound(h.hit, h.t, h.P, self.table, index=h.surface.view(np.int32))


@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_light_loop_shadow_rays_walked_through_the_group(ctx, gpu, oracle, T, node):
    from rlshaders_amd import nearest_group, shadow_walk
    from test_gpu_shadow_walk import SEED as LSEED, SPP_N, batch, surface_table
    b, lights = batch(T, gpu, oracle, node)
    q = b.emit(lights, SPP_N, LSEED)
    rays = q.count
    table = surface_table(T, gpu)
    insts = shadow_instances()
    g = DeviceGroup(gpu, insts)
    try:
        tracer = nearest_group.tracer(g.group, opacity=table, keep=True)
        w = shadow_walk.run(q, b.P, tracer, max_steps=12)
        got = _host(w.visibility)[:, :rays]
        cap = q.capacity
        wn = shadow_walk_np(_host(b.P), _host(q._point), _host(q._dir), _host(q._maxdist), 12, count=rays)
        tn = shadow_tracer(insts, cap, _host(table))
        steps = shadow_run_np(wn, tn)
        assert w.active == 0 and wn.active == 0 and len(steps) >= 3
        cases.assert_same_bits(got, wn.T[:, :rays], (node, "visibility against the statement"))
        # what the DEVICE visited, call by call: the statement's (surface, instance, prim) in the same order
        seen = [[] for _ in range(cap)]
        for m, ray, f in tracer.found:
            hit = _host(f.hit)[:m] != 0
            for j, s_, i, p in zip(_host(ray).view(np.uint32).astype(np.int64)[hit], _host(f.surface)[:m][hit], _host(f.instance)[:m][hit],
                                   _host(f.prim)[:m][hit]):
                seen[j].append((int(s_), int(i), int(p)))
        assert seen == tn.visited
        behind = np.array([any(v[0] == 3 for v in vs) for vs in tn.visited[:rays]])
        assert behind.any() and (got[:, behind].view(np.uint32) == 0).all() and (got[:, ~behind] > 0).all()
        # through both quads: the same prim id in instance 0, then in instance 1 -- the second is not skipped
        both = [vs for vs in tn.visited[:rays] if len(vs) >= 2 and vs[0][1] == 0 and vs[1][1] == 1]
        assert len(both) > 10 and any(vs[0][2] == vs[1][2] for vs in both)
    finally:
        g.close()
