"""-m gpu: the any-hit query against the shadow walk it shortens (include/rlshaders_amd_nearest_any.h, AGAINST THE FULL WALK), on
the light loops' shadow queues of the rlGgx and rlDisney batches of test_gpu_shadow_walk.py through the mesh of
test_gpu_nearest_walks.py (two tinted quads, an opaque sphere).

  (a) an all-ones opacity table: the one launch's visibility equals shadow_walk.run's final T bit for bit at max_steps 1 and 12,
      without a flag table and with the flags of the all-ones table, and the queue's resolve of the two is bit-identical;
  (b) the mixed table: nearest_any.shadow (the launch, then the walk begun on the reach plane) equals the full walk on every ray
      of state 0 or 2; the rays it walked are count(state == 2), fewer than the queue holds; the states are any_np's;
  (c) the blocked rays: all-zero bits from the two-phase route, and all-zero bits from the full walk wherever the numpy walk
      visited an opaque surface; the blocked rays left out of that comparison are at most 1 % -- checked numpy against numpy;
  the list route of a trace.HitQueues (origins through an int64 via) equals the direct route on the same rays."""
import numpy as np
import pytest
import torch

import cases
import nearest_any_util as A
import nearest_util as U
from nearest_any_util import BLOCKED, CLEAR, VEILED, any_np
from nearest_util import F
from shadow_walk_util import run_np as shadow_run_np
from shadow_walk_util import shadow_walk_np
from test_gpu_nearest_walks import _dev, _host, device_scene, shadow_mesh, shadow_tracer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    from rlshaders_amd import nearest_any, trace
    trace.load(), nearest_any.load()                                 # (a missing library is an error, not a build)
    return trace


def _bits(t, rays):
    return np.ascontiguousarray(_host(t)[:, :rays]).view(np.uint32)


def queue_rays(b, q):
    from rlshaders_amd import nearest
    return nearest.Rays(b.P, q._dir, maxdist=q._maxdist, via=q._point, count=q.offsets[q.n:], rays=q.capacity)


@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_all_opaque_is_the_walks_visibility_bit_for_bit(gpu, oracle, T, node):
    from rlshaders_amd import nearest, nearest_any, shadow_walk
    from test_gpu_shadow_walk import SEED, SPP_N, batch
    b, lights = batch(T, gpu, oracle, node)
    q = b.emit(lights, SPP_N, SEED)
    rays = q.count
    mesh = shadow_mesh()
    scene = device_scene(gpu, mesh)
    ones = torch.ones(3, 4, device="cuda")
    flags = nearest_any.opaque_flags(gpu, ones)
    assert _host(flags).tolist() == [1, 1, 1, 1]
    f0 = nearest_any.hits(scene, queue_rays(b, q))                   # no table
    f1 = nearest_any.hits(scene, queue_rays(b, q), opaque=flags)
    state = _host(f0.state)[:rays]
    assert np.array_equal(state, _host(f1.state)[:rays]) and np.array_equal(_bits(f0.visibility, rays), _bits(f1.visibility, rays))
    assert (state == BLOCKED).sum() > rays // 4 and not (state == VEILED).any()
    assert not _host(f0.reach)[:rays].view(np.uint32).any()
    P, point = _host(b.P), _host(q._point)[:rays].astype(np.int64)
    want = any_np(mesh, P[:, point], _host(q._dir)[:, :rays], _host(q._maxdist)[:rays])
    assert np.array_equal(state, want.state) and np.array_equal(_bits(f0.visibility, rays), A.bits(want.visibility))
    mine = q.resolve(f0.visibility)
    for max_steps in (1, 12):
        w = shadow_walk.run(q, b.P, nearest.tracer(scene, opacity=ones), max_steps=max_steps)
        assert w.active == 0
        assert np.array_equal(_bits(f0.visibility, rays), _bits(w.visibility, rays)), max_steps
        walked = q.resolve(w.visibility)
        for k, name in enumerate(("direct_diffuse", "direct_specular")):
            cases.assert_same_bits(_host(mine[k]), _host(walked[k]), (node, max_steps, name))
    assert (_host(mine[0]) < b.analytic(lights, SPP_N, SEED)[0]).any()
    scene.close()


@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_the_two_phase_route_against_the_full_walk(gpu, oracle, T, node):
    from rlshaders_amd import nearest, nearest_any, shadow_walk
    from test_gpu_shadow_walk import SEED, SPP_N, batch, surface_table
    b, lights = batch(T, gpu, oracle, node)
    q = b.emit(lights, SPP_N, SEED)
    rays, cap = q.count, q.capacity
    table = surface_table(T, gpu)
    mesh = shadow_mesh()
    scene = device_scene(gpu, mesh)
    s = nearest_any.shadow(q, b.P, scene, table, max_steps=12)
    full = shadow_walk.run(q, b.P, nearest.tracer(scene, opacity=table), max_steps=12)
    assert s.walk.active == 0 and full.active == 0
    assert _host(s.flags).tolist() == [0, 0, 0, 1]                   # three tinted surfaces and the opaque sphere
    state = _host(s.state)[:rays]
    # the states are the statement's
    P, point = _host(b.P), _host(q._point)[:rays].astype(np.int64)
    dirs, maxdist = _host(q._dir)[:, :rays], _host(q._maxdist)[:rays]
    want = any_np(mesh, P[:, point], dirs, maxdist, flags=_host(s.flags))
    assert np.array_equal(state, want.state)
    assert np.array_equal(_host(s.reach)[:rays].view(np.uint32), A.bits(want.reach))
    # (b) clear and veiled rays: the full walk's bytes; the walk was begun on the veiled rays alone
    two, whole = _bits(s.visibility, rays), _bits(full.visibility, rays)
    open_ = state != BLOCKED
    assert np.array_equal(two[:, open_], whole[:, open_])
    veiled = int((state == VEILED).sum())
    assert s.walked == veiled and 0 < veiled < rays
    # (c) blocked rays: zero here; zero in the full walk where the numpy walk met the opaque surface
    blocked = state == BLOCKED
    assert blocked.any() and not two[:, blocked].any()
    wn = shadow_walk_np(P, _host(q._point), _host(q._dir), _host(q._maxdist), 12, count=rays)
    tn = shadow_tracer(mesh, cap, _host(table))
    shadow_run_np(wn, tn)
    met = np.array([3 in v for v in tn.visited[:rays]])
    cases.assert_same_bits(_host(full.visibility)[:, :rays], wn.T[:, :rays], (node, "the full walk against the statement"))
    compared = blocked & met
    assert not whole[:, compared].any() and not A.bits(wn.T[:, :rays])[:, compared].any()
    left_out = blocked & ~met                                        # numpy against numpy: the scene and queue stay within the cap
    print(f"{node}: rays {rays} clear {(state == CLEAR).sum()} blocked {blocked.sum()} veiled {veiled} left out {left_out.sum()}")
    assert left_out.sum() * 100 <= blocked.sum(), (left_out.sum(), blocked.sum())
    scene.close()


def test_the_hit_queues_list_route_equals_the_direct_route(gpu):
    """the shadow queue of trace.sss_hit_rays: its origins go through via = hit_element, so shadow() lists the rays with the
    walk's begin and queries the list; the same rays as a RawQueue over gathered origins take the direct route"""
    import rlshaders_amd as R
    from rlshaders_amd import nearest, nearest_any, shadow_walk, trace
    from test_gpu_walk import sampler, scene_pair, walked_hits
    n, spp_n = 60, 2
    case, so, _ = scene_pair("plane", n, use_cavity_fade=True)
    s = sampler(gpu, case)
    P = _dev(case["P"])
    pq = trace.sss_probe_rays(s, P, spp_n, 4242)
    cnt, hP, hN, _ = walked_hits(gpu, pq, case, so, spp_n)
    light = R.make_light(center=(0.5, 0.5, 4.0), radius=1.0, radiance=(2.0, 1.5, 1.0), mis_mode=0)
    hq = trace.sss_hit_rays(s, P, pq, cnt, hP, hN, light, 2, 7, use_cavity_fade=True)
    rays, cap = hq.shadow_count, hq.shadow_capacity
    assert rays > n
    O = hP.reshape(3, -1)
    # a tinted quad at z = 2 (surface 0) and an opaque sphere below the light (surface 1)
    ball = U.icosphere(2, radius=0.6, center=(0.5, 0.5, 2.8), surface=1)
    nv = ball.V.shape[0]
    V = np.concatenate([ball.V, np.array([(-20, -20, 2), (20, -20, 2), (20, 20, 2), (-20, 20, 2)], F)])
    tri = np.concatenate([ball.tri, np.array([(0, 1, 2), (0, 2, 3)], np.uint32) + nv])
    mesh = U.Mesh(V, tri, surface=np.concatenate([ball.surface, np.zeros(2, np.uint32)]))
    scene = device_scene(gpu, mesh)
    table = _dev(np.array([[0.25, 1.0], [0.5, 1.0], [0.75, 1.0]], F))
    a = nearest_any.shadow(hq, O, scene, table, max_steps=6)
    # the direct route: every ray's origin gathered on the host
    via, point = _host(hq._hit_element), _host(hq._spoint)[:rays].astype(np.int64)
    start = np.zeros((3, cap), F)
    start[:, :rays] = _host(O)[:, via[point]]
    raw = shadow_walk.RawQueue(hq._sdir, hq._smaxdist, torch.arange(cap, dtype=torch.int32, device="cuda"),
                               hq.shadow_offsets[hq.hit_capacity:])
    b = nearest_any.shadow(raw, _dev(start), scene, table, max_steps=6, ctx=gpu)
    assert np.array_equal(_host(a.state)[:rays], _host(b.state)[:rays]) and a.walked == b.walked
    assert np.array_equal(_bits(a.visibility, rays), _bits(b.visibility, rays))
    assert np.array_equal(_host(a.reach)[:rays].view(np.uint32), _host(b.reach)[:rays].view(np.uint32))
    state = _host(a.state)[:rays]
    want = any_np(mesh, start[:, :rays], _host(hq._sdir)[:, :rays], _host(hq._smaxdist)[:rays], flags=np.array([0, 1], np.uint8))
    assert np.array_equal(state, want.state) and (state != CLEAR).any()
    full = shadow_walk.run(hq, O, nearest.tracer(scene, opacity=table), via=hq._hit_element, max_steps=6)
    open_ = state != BLOCKED
    assert np.array_equal(_bits(a.visibility, rays)[:, open_], _bits(full.visibility, rays)[:, open_])
    scene.close()
