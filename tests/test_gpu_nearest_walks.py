"""-m gpu: the consumers of the nearest-hit library, with no host tracer between the device calls.

1. rlSss probe rays (n up to 67 points, spp_n 1 .. 3) walked through an icosphere about the points by ``walk.run`` over
   ``nearest.tracer``: count, P and N of the hits equal walk_np (tests/walk_util.py) over the numpy statement (tests/nearest_util.py)
   bit for bit, `last` carried across the steps in both.
2. rlGgx and rlDisney light-loop shadow rays walked under two tinted quads and an opaque sphere, `surface` indexing an opacity
   table: the visibility equals shadow_walk_np over the statement, and rls_trace_shadow_visibility over the hits the device
   visited; the resolves on it equal the resolves on the fold, as tests/test_gpu_shadow_walk.py checks them.
3. a glossy queue's rays traced (via = point over P, no maxdist), routed by the bin plane and gathered from the found planes:
   every routed and gathered plane, and the resolve over a radiance looked up by surface, equal the same calls fed by the numpy
   statement."""
import numpy as np
import pytest
import torch

import cases
import nearest_util as U
from nearest_util import F, NO_PRIM
from shadow_walk_util import Found as ShadowFound, shadow_walk_np
from shadow_walk_util import run_np as shadow_run_np
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
    from rlshaders_amd import nearest, shadow_walk, walk
    walk.load(), shadow_walk.load(), nearest.load()                  # (a missing library is an error, not a build)
    c = R.Context(0)
    yield c
    c.close()


def device_scene(ctx, mesh, leaf=0):
    from rlshaders_amd import nearest
    return nearest.Scene(ctx, mesh.V, mesh.tri, surface=mesh.surface, normals=mesh.normals, leaf_size=leaf)


# ---- 1. the probe walk ---------------------------------------------------------------------------------------------------------------
class walk_tracer(U.np_tracer):
    def __call__(self, ray, origin, dirs, maxdist):
        h = super().__call__(ray, origin, dirs, maxdist)
        return WalkFound(h.hit, h.t, h.P, h.N, h.Ns)


@pytest.mark.parametrize("n,spp_n", [(1, 1), (22, 3), (67, 1), (67, 2), (40, 3)])
def test_probes_walked_through_the_icosphere(ctx, n, spp_n):
    import rlshaders_amd as R
    from rlshaders_amd import nearest, trace, walk
    case, _ = setting("sphere", n)
    P = case["P"]
    s = R.SssSampler(ctx, _dev(case["N"]), _dev(case["T"]), _dev(case["albedo"]), _dev(case["dist"]), has_dPdu=True)
    q = trace.sss_probe_rays(s, _dev(P), spp_n, SEED)
    origin, dirs, maxdist = _host(q.origin), _host(q.dir), _host(q.maxdist)
    centre = P.astype(np.float64).mean(axis=1)
    reach = float(np.median(maxdist[maxdist > 0])) if (maxdist > 0).any() else 1.0
    # the points inside, the wall within the probes' reach of most of them: a ray meets the wall from the inside and, moved on to
    # its hit, must not meet the triangle it stands on again
    radius = float(np.linalg.norm(P.astype(np.float64).T - centre, axis=1).max()) + 0.25 * reach
    mesh = U.icosphere(2, radius=radius, center=centre)
    scene = device_scene(ctx, mesh)
    tracer = nearest.tracer(scene)
    w = walk.run(q, _dev(P), tracer)
    wn = walk_np(origin, dirs, maxdist, P, spp_n * spp_n)
    tn = walk_tracer(mesh, len(maxdist))
    counts = run_np(wn, tn)
    assert w.active == 0 and wn.active == 0
    np.testing.assert_array_equal(_host(w.hit_count), wn.count)
    live = np.arange(wn.max_hits)[:, None] < wn.count[None, :]
    same_bits_or_both_nan(_host(w.hit_P)[:, live], wn.hP[:, live], "hits.P")
    same_bits_or_both_nan(_host(w.hit_N)[:, live], wn.hN[:, live], "hits.N")
    np.testing.assert_array_equal(_host(tracer.last).view(np.uint32)[:len(maxdist)], tn.last)
    # the same tracer serves a second walk after reset(): the same hits, `last` having forgotten where the first walk ended
    w2 = walk.run(q, _dev(P), tracer.reset())
    assert torch.equal(w2.hit_count, w.hit_count)
    same_bits_or_both_nan(_host(w2.hit_P)[:, live], wn.hP[:, live], "hits.P of the second walk")
    if n > 1:
        assert wn.count.max() >= 1 and len(counts) >= 2, (counts, wn.count.max())
        # a second step's rays start ON the triangle they hit: by `last` none of them meets it again
        (j0, h0), (j1, h1) = tn.log[0], tn.log[1]
        at = np.searchsorted(j0, j1)
        assert np.array_equal(j0[at], j1) and not np.any((h1.hit != 0) & (h1.prim == h0.prim[at]))
    scene.close()


def test_probe_walk_with_objects(ctx):
    """own and object = surface: a wall of another object stops the walk (RLS_WALK_FOREIGN_STOPS), as walk_np says"""
    import rlshaders_amd as R
    from rlshaders_amd import nearest, trace, walk
    n, spp_n = 30, 2
    case, _ = setting("sphere", n)
    P = case["P"]
    s = R.SssSampler(ctx, _dev(case["N"]), _dev(case["T"]), _dev(case["albedo"]), _dev(case["dist"]), has_dPdu=True)
    q = trace.sss_probe_rays(s, _dev(P), spp_n, SEED)
    origin, dirs, maxdist = _host(q.origin), _host(q.dir), _host(q.maxdist)
    centre = P.astype(np.float64).mean(axis=1)
    radius = float(np.linalg.norm(P.astype(np.float64).T - centre, axis=1).max()) + 0.25 * float(np.median(maxdist[maxdist > 0]))
    mesh = U.icosphere(2, radius=radius, center=centre)
    mesh.surface = (np.arange(mesh.nt) % 2).astype(np.uint32)        # every other triangle belongs to object 1
    own = np.zeros(n, np.int32)
    scene = device_scene(ctx, mesh)
    w = walk.run(q, _dev(P), nearest.tracer(scene, objects=True), own=_dev(own))

    class with_objects(U.np_tracer):
        def __call__(self, *a):
            h = U.np_tracer.__call__(self, *a)
            return WalkFound(h.hit, h.t, h.P, h.N, h.Ns, object=h.surface.view(np.int32))

    wn = walk_np(origin, dirs, maxdist, P, spp_n * spp_n, own=own)
    run_np(wn, with_objects(mesh, len(maxdist)))
    np.testing.assert_array_equal(_host(w.hit_count), wn.count)
    live = np.arange(wn.max_hits)[:, None] < wn.count[None, :]
    same_bits_or_both_nan(_host(w.hit_P)[:, live], wn.hP[:, live], "hits.P")
    assert 0 < (wn.count > 0).sum() < len(maxdist)
    scene.close()


# ---- 2. the shadow walk ----------------------------------------------------------------------------------------------------------------
def shadow_mesh():
    """two quads at z = 1.2 and z = 1.4 (surfaces 0 and 1, tinted) and a sphere of radius 0.3 about (2, 2, 1.75) (surface 3, opaque;
    surface 2 of the table is not in the scene)"""
    s = U.icosphere(2, radius=0.3, center=(2.0, 2.0, 1.75), surface=3)
    V, T, S = [s.V], [s.tri], [s.surface]
    for k, z in enumerate((1.2, 1.4)):
        base = sum(len(v) for v in V)
        V.append(np.array([(-20, -20, z), (20, -20, z), (20, 20, z), (-20, 20, z)], F))
        T.append(np.array([(0, 1, 2), (0, 2, 3)], np.uint32) + base)
        S.append(np.full(2, k, np.uint32))
    return U.Mesh(np.concatenate(V), np.concatenate(T), surface=np.concatenate(S))


@pytest.fixture(scope="module")
def T():
    from rlshaders_amd import trace
    trace.load()
    return trace


class shadow_tracer(U.np_tracer):
    def __init__(self, mesh, rays, table):
        super().__init__(mesh, rays)
        self.table, self.visited = table, [[] for _ in range(rays)]

    def __call__(self, ray, origin, dirs, maxdist):
        h = super().__call__(ray, origin, dirs, maxdist)
        for j, s in zip(np.asarray(ray).astype(np.int64)[h.hit != 0], h.surface[h.hit != 0]):
            self.visited[j].append(int(s))
        return ShadowFound(h.hit, h.t, h.P, self.table, index=h.surface.view(np.int32))


@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_light_loop_shadow_rays_walked_through_the_mesh(ctx, gpu, oracle, T, node):
    from rlshaders_amd import nearest, shadow_walk
    from test_gpu_shadow_walk import SEED as LSEED, SPP_N, batch, surface_table
    b, lights = batch(T, gpu, oracle, node)
    q = b.emit(lights, SPP_N, LSEED)
    rays = q.count
    table = surface_table(T, gpu)
    mesh = shadow_mesh()
    scene = device_scene(gpu, mesh)
    tracer = nearest.tracer(scene, opacity=table, keep=True)
    w = shadow_walk.run(q, b.P, tracer, max_steps=12)
    got = _host(w.visibility)[:, :rays]
    # the statement's walk over the numpy tracer
    cap = q.capacity
    wn = shadow_walk_np(_host(b.P), _host(q._point), _host(q._dir), _host(q._maxdist), 12, count=rays)
    tn = shadow_tracer(mesh, cap, _host(table))
    steps = shadow_run_np(wn, tn)
    assert w.active == 0 and wn.active == 0 and len(steps) >= 3
    cases.assert_same_bits(got, wn.T[:, :rays], (node, "visibility against the statement"))
    # the fold over the hits the DEVICE visited: its own found planes, call by call
    K = len(tracer.found)
    count, index = np.zeros(cap, np.uint8), np.zeros((K, cap), np.int32)
    for m, ray, f in tracer.found:
        j = _host(ray).view(np.uint32).astype(np.int64)[_host(f.hit)[:m] != 0]
        index[count[j], j] = _host(f.surface)[:m][_host(f.hit)[:m] != 0]
        count[j] += 1
    assert [len(v) for v in tn.visited] == list(count) and count.max() >= 3
    hits = T.ShadowHits(_dev(count), table, K, stride=cap, index=_dev(index.reshape(-1)))
    folded = T.shadow_visibility(gpu, rays, hits)
    cases.assert_same_bits(got, _host(folded)[:, :rays], (node, "visibility against the fold"))
    behind = np.array([3 in v for v in tn.visited[:rays]])
    assert behind.any() and (got[:, behind].view(np.uint32) == 0).all() and (got[:, ~behind] > 0).all()
    walked, listed = q.resolve(w.visibility), q.resolve(folded)
    for k, name in enumerate(("direct_diffuse", "direct_specular")):
        cases.assert_same_bits(_host(walked[k]), _host(listed[k]), (node, name))
    assert (_host(walked[0]) < b.analytic(lights, SPP_N, LSEED)[0]).any()
    scene.close()


# ---- 3. a glossy queue traced, routed, gathered -------------------------------------------------------------------------------------------
def test_glossy_rays_traced_routed_and_gathered(ctx, gpu, oracle, T):
    from rlshaders_amd import nearest
    from test_gpu_shadow_walk import batch
    b, _ = batch(T, gpu, oracle, "ggx")
    q = T.glossy_rays(b.s, 2, 77)
    rays = q.count
    mesh = shadow_mesh()
    # the lower quad about the points' centre, its two triangles two surfaces: the hits fall either side of its diagonal
    lower = mesh.tri[-4, 0]
    mesh.V[lower:lower + 4, :2] += _host(b.P)[:2].mean(axis=1)
    mesh.surface[-4:] = (0, 1, 2, 2)
    scene = device_scene(gpu, mesh)
    bins = np.array([1, 0, 255, 1], np.uint8)                        # the lower quad's halves shade in two nodes, the upper in none
    n_bins = 2
    f = scene.hits(nearest.Rays(b.P, q._dir, via=q._point, rays=rays), bin_of_surface=_dev(bins))
    P, dirs, point = _host(b.P), _host(q._dir)[:, :rays], _host(q._point)[:rays].astype(np.int64)
    h = U.nearest_np(mesh, P[:, point], dirs)
    assert h.hit.any() and not h.hit.all()
    want_bin = np.where(h.hit != 0, bins[np.minimum(h.surface, 3)], 255).astype(np.uint8)
    np.testing.assert_array_equal(_host(f.bins()), want_bin)
    # the same routing and gathering fed by the numpy statement's planes
    names = ("P", "N", "Ns", "T", "wo", "surface", "u", "v")
    fed = [_dev(getattr(h, k).view(np.int32) if k == "surface" else getattr(h, k)) for k in names]
    assert len(f.gatherable()) == len(fed)
    r_dev, r_np = T.route_hits(gpu, f.bins(), n_bins), T.route_hits(gpu, _dev(want_bin), n_bins)
    np.testing.assert_array_equal(_host(r_dev.offsets), _host(r_np.offsets))
    np.testing.assert_array_equal(_host(r_dev.order), _host(r_np.order))
    for bin_ in range(n_bins):
        a, c = r_dev.gather(bin_, *f.gatherable()), r_np.gather(bin_, *fed)
        assert a[0].shape[-1] == int((want_bin == bin_).sum()) > 0
        for k, x, y in zip(names, a, c):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (bin_, k)
    # a radiance per ray looked up by what it hit, scattered back through the routes, resolved: every AOV equal
    outs = []
    for r, surf in ((r_dev, f.surface), (r_np, fed[5])):
        L = torch.zeros(3, q.capacity, device="cuda")
        for bin_ in range(n_bins):
            (s_,) = r.gather(bin_, surf)
            r.scatter(bin_, torch.stack([(s_ + 1).float() * 0.25, (s_ + 2).float() * 0.125, torch.ones_like(s_).float()]).contiguous(), L)
        r.fill_misses((0.5, 0.25, 0.125), L)
        outs.append(q.resolve(L))
    res_a, res_b = (o if isinstance(o, (tuple, list)) else (o,) for o in outs)
    for x, y in zip(res_a, res_b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    scene.close()
