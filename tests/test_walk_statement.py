"""CPU: the probe walk's statement (tests/walk_util.py, walk_np) against the oracle's analytic scene, both host code.  Over the
cumulative tracer the walk must visit, for EVERY ray, the list orc_scene_trace reports for it (trace_sss_util.trace_queue) with
the hits within AI_EPSILON of the previous accepted position removed -- the premise of the end-to-end tests of
tests/test_gpu_walk.py, which hold the device's walk to rls_sss_integrate_scatter bit for bit.  And the rules nobody would guess,
each on a stream made for it."""
import numpy as np
import pytest

import oracle_lib as O
from trace_sss_util import EPS, plane_case, sphere_case, trace_queue
from walk_util import TRIALS, Found, cumulative_tracer, length_np, nearest_tracer, run_np, walk_np

SEED = 4242
SPHERE = dict(geometry="sphere", sphere_center=(0.3, -0.2, 0.1), sphere_radius=0.35, light_dir=(0.0, 0.6, 0.8),
              light_color=(1.5, 1.0, 0.25))


def setting(kind, n, **flags):
    """(case, the oracle's scene) of the plane or the sphere of tests/test_gpu_trace_sss.py; flags: make_scene's other arguments"""
    if kind == "plane":
        case, nrm = plane_case(n)
        return case, O.make_scene(geometry="plane", plane_point=(0.5, -1.0, 0.25), plane_normal=tuple(nrm), light_dir=tuple(nrm),
                                  light_color=(1.0, 0.5, 2.0), **flags)
    return sphere_case(n), O.make_scene(**SPHERE, **flags)


def oracle_queue(case, spp_n, first=0):
    """integrateScatter's probe rays from the oracle's getProbeRay, dense and point-major -> origin, dir [3, rays], maxdist"""
    n, spp = case["P"].shape[1], spp_n * spp_n
    o = O.Sss(n, case["dist"], case["albedo"], N=case["N"], T=case["T"], has_dPdu=True)
    origin, dirs, maxdist = np.zeros((3, n, spp), np.float32), np.zeros((3, n, spp), np.float32), np.zeros((n, spp), np.float32)
    for s in range(spp):
        rx, ry = O.batch_sample_02(SEED, first, n, 0, s)
        ref = o.probe(rx, ry)
        origin[:, :, s] = (case["P"] + ref["origin"]).astype(np.float32)
        dirs[:, :, s], maxdist[:, s] = ref["dir"], ref["maxdist"]
    return origin.reshape(3, -1), dirs.reshape(3, -1), maxdist.reshape(-1)


def list_without_duplicates(P0, cnt, hP, hN, max_hits):
    """a reported hit list with the hits the walk's distance test refuses removed -> (count, P, N) as the walk stores them"""
    rays = len(cnt)
    out_c, out_P, out_N = np.zeros(rays, np.uint8), np.zeros((3, max_hits, rays), np.float32), np.zeros((3, max_hits, rays), np.float32)
    prev = P0.copy()
    for k in range(hP.shape[1]):
        alive = (k < cnt) & (out_c < max_hits)
        moved = alive & (length_np((prev - hP[:, k]).astype(np.float32)) > EPS)
        j = np.flatnonzero(moved)
        out_P[:, out_c[j], j], out_N[:, out_c[j], j] = hP[:, k, j], hN[:, k, j]
        out_c[j] += 1
        prev = np.where(moved, hP[:, k], prev)
    return out_c, out_P, out_N


def check_walk_visits_the_scene_list(scene, origin, dirs, maxdist, P, spp, max_hits=TRIALS):
    """every ray: walk_np over the cumulative tracer = orc_scene_trace's list minus the within-epsilon hits"""
    rays = len(maxdist)
    w = walk_np(origin, dirs, maxdist, P, spp, max_hits=max_hits)
    counts = run_np(w, cumulative_tracer(scene, origin, dirs, maxdist))
    assert w.active == 0 and len(counts) <= 3
    cnt, hP, hN = trace_queue(scene, origin, dirs, maxdist)
    want_c, want_P, want_N = list_without_duplicates(P[:, np.arange(rays) // spp], cnt, hP, hN, max_hits)
    np.testing.assert_array_equal(w.count, want_c)
    assert np.array_equal(w.hP.view(np.uint32), want_P.view(np.uint32))
    assert np.array_equal(w.hN.view(np.uint32), want_N.view(np.uint32))
    return w


@pytest.mark.parametrize("spp_n", [1, 2, 3])
@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_walk_over_the_cumulative_tracer_visits_the_scene_list(kind, spp_n):
    n = 300
    case, scene = setting(kind, n)
    origin, dirs, maxdist = oracle_queue(case, spp_n)
    w = check_walk_visits_the_scene_list(scene, origin, dirs, maxdist, case["P"], spp_n * spp_n)
    assert int(w.count.sum()) > len(maxdist) // 4                   # the walk found something


def test_nearest_tracer_walk_ends_within_the_budget():
    """from a hit's own position the sphere is found again at t ~ 0: hits the distance test refuses, trials that run out"""
    case, scene = setting("sphere", 200)
    origin, dirs, maxdist = oracle_queue(case, 2)
    w = walk_np(origin, dirs, maxdist, case["P"], 4)
    counts = run_np(w, nearest_tracer(scene))
    assert w.active == 0 and len(counts) <= TRIALS and int(w.count.max()) >= 1


def _stream(n, P0=None):
    P0 = np.zeros((3, n), np.float32) if P0 is None else P0
    origin = P0 + np.float32(0.25)
    dirs = np.tile(np.array([[1.0], [0.0], [0.0]], np.float32), (1, n))
    return P0, origin, dirs, np.ones(n, np.float32)


def test_budget_of_twelve_trials_and_the_last_accepted_position():
    n = 5
    P0, origin, dirs, maxdist = _stream(n)
    w = walk_np(origin, dirs, maxdist, P0, 1)
    same = Found(np.ones(n), np.zeros(n), P0, dirs, dirs)
    for step in range(TRIALS):
        assert w.active == n and int(w.trials[0]) == TRIALS - step
        w.step(same)                                                # a hit ON prev: refused, the ray moves on, a trial is spent
    assert w.active == 0 and w.steps == TRIALS and not w.count.any()
    # the distance is to the last ACCEPTED position: steps of 0.6 epsilon are refused one after another
    w = walk_np(origin, dirs, maxdist, P0, 1)
    for step in range(1, 4):
        P = P0.copy()
        P[0] += np.float32(0.6e-4 * step)
        w.step(Found(np.ones(n), np.zeros(n), P, dirs, dirs))
    np.testing.assert_array_equal(w.count, 1)                       # only 1.2 epsilon was accepted; 1.8 is 0.6 from it
    assert np.all(w.hP[0, 0] == np.float32(1.2e-4))


def test_maxdist_shrinks_at_accepted_hits_only_and_ends_the_walk():
    n = 4
    P0, origin, dirs, maxdist = _stream(n)
    w = walk_np(origin, dirs, maxdist, P0, 1)
    t = np.array([0.25, 1.0, 2.0, np.nan], np.float32)
    w.step(Found(np.ones(n), t, P0, dirs, dirs))                    # refused: nothing is subtracted
    np.testing.assert_array_equal(w.maxdist, 1.0)
    P = P0 + np.float32(1.0)
    w.step(Found(np.ones(n), t, P, dirs, dirs))
    np.testing.assert_array_equal(w.ray, [0, 3])                    # left 0 and left < 0 end the walk, a NaN left does not
    assert w.maxdist[0] == np.float32(0.75) and np.isnan(w.maxdist[1])


def test_foreign_hits_and_inactive_rays():
    n = 6
    P0, origin, dirs, maxdist = _stream(n)
    maxdist[:3] = [0.0, -1.0, np.nan]                               # never listed
    own = np.arange(n, dtype=np.int32)
    P = P0 + np.float32(1.0)
    hit = Found(np.ones(3), np.full(3, 0.5), P[:, 3:], dirs[:, 3:], -dirs[:, 3:], object=np.array([3, 9, 5], np.int32))
    stop = walk_np(origin, dirs, maxdist, P0, 1, own=own).step(hit)
    np.testing.assert_array_equal(stop.ray, [3, 5])
    skip = walk_np(origin, dirs, maxdist, P0, 1, own=own, foreign="skip").step(hit)
    np.testing.assert_array_equal(skip.ray, [3, 4, 5])
    np.testing.assert_array_equal(skip.count, [0, 0, 0, 1, 0, 1])
    np.testing.assert_array_equal(skip.maxdist, np.array([0.5, 1.0, 0.5], np.float32))
    np.testing.assert_array_equal(skip.trials, TRIALS - 1)
    assert np.all(skip.hN[0, 0, [3, 5]] == 1.0)                     # Ns = -dir against N = dir: flipped
