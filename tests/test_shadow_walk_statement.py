"""CPU: the shadow walk's statement (tests/shadow_walk_util.py, shadow_walk_np) against the fold it replaces, both host code.  For
EVERY ray the statement run over a nearest-hit tracer must give the visibility rls_trace_shadow_visibility's restatement
(trace_opacity_util.fold) gives over the hits that ray visited, in order, bit for bit with NaN compared as NaN -- the premise of
tests/test_gpu_shadow_walk.py, which holds the device's walk to the statement.  And the rules, each on a stream made for it."""
import numpy as np
import pytest

from shadow_walk_util import F, Scene, all_hits, nearest_tracer, rule_streams, run_np, shadow_walk_np
from trace_opacity_util import HOSTILE, fold, same_bits

SLABS = [((0.0, 0.0, z), (0.0, 0.0, 1.0)) for z in (0.5, 0.8, 1.1)]
SPHERE = ((-1.5, 0.75, 1.6), 0.45)
LIGHTS = np.array([[-4.0, 2.0, 3.0], [6.0, 1.0, 2.0]], F)
# three tinted slabs and the opaque sphere
TABLE = np.array([[0.25, 0.5, 0.125, 1.0], [0.5, 0.5, 0.25, 1.0], [0.75, 0.5, 0.0, 1.0]], F)


def light_rays(n, seed=7):
    """n points about the origin, a ray each towards a point in either light -> O, point, dirs, maxdist"""
    rng = np.random.default_rng(seed)
    O = ((rng.random((3, n), F) - F(0.5)) * F(0.5)).astype(F)
    O[2] *= F(0.1)
    point = np.repeat(np.arange(n, dtype=np.int32), 2)
    to = (LIGHTS[np.tile(np.arange(2), n)].T + (rng.random((3, 2 * n), F) - F(0.5)) * F(1.2)).astype(F)
    d = (to - O[:, point]).astype(F)
    ln = np.sqrt((d * d).sum(axis=0)).astype(F)
    return O, point, (d / ln).astype(F), ln


def walked(table, max_steps, indexed, n=150, base=None):
    O, point, dirs, maxdist = light_rays(n)
    scene = Scene(SLABS, [SPHERE])
    tracer = nearest_tracer(scene, table, len(maxdist), indexed)
    w = shadow_walk_np(O, point, dirs, maxdist, max_steps, base=base)
    counts = run_np(w, tracer)
    return w, tracer, counts, scene, (O[:, point], dirs, maxdist)


def folded(tracer, table, rays, base=None):
    count, index, K = tracer.hits()
    return fold(rays, count, table, K, rays, index=index, base=base)


@pytest.mark.parametrize("indexed", [True, False])
@pytest.mark.parametrize("max_steps", [1, 2, 12])
def test_statement_over_nearest_hits_is_the_fold_over_the_visited_hits(max_steps, indexed):
    w, tracer, counts, scene, (origin, dirs, maxdist) = walked(TABLE, max_steps, indexed)
    rays = len(maxdist)
    assert w.active == 0 and len(counts) <= max_steps
    assert same_bits(w.T, folded(tracer, TABLE, rays))
    # what a ray visited: the surfaces of the whole ray, nearest first, up to the opaque sphere or the budget
    cnt, surf = all_hits(scene, origin, dirs, maxdist)
    for j in range(rays):
        want = []
        for s in surf[:cnt[j], j]:
            want.append(int(s))
            if s == 3 or len(want) == max_steps:
                break
        assert tracer.visited[j] == want, j
    assert max_steps < 4 or (any(3 in v for v in tracer.visited) and any(len(v) == 3 and 3 not in v for v in tracer.visited))


def test_a_ray_behind_the_opaque_sphere_is_black_and_retired_there():
    w, tracer, counts, _, _ = walked(TABLE, 12, True)
    behind = [j for j, v in enumerate(tracer.visited) if v and v[-1] == 3]
    assert behind
    assert np.all(w.T[:, behind].view(np.uint32) == 0)              # +0 exactly
    clear = [j for j, v in enumerate(tracer.visited) if 3 not in v]
    assert np.all(w.T[:, clear] > 0)


def test_hostile_table_and_base_propagate_as_in_the_fold():
    table = np.stack([HOSTILE[[0, 5, 7, 2]], HOSTILE[[1, 8, 14, 9]], HOSTILE[[3, 4, 10, 6]]]).astype(F)
    rays = 300
    base = (np.random.default_rng(3).random((3, rays), F) * F(2) - F(0.5)).astype(F)
    w, tracer, _, _, _ = walked(table, 12, True, base=base)
    assert same_bits(w.T, folded(tracer, table, rays, base=base))
    assert np.isnan(w.T).any() and np.isinf(w.T).any()


# ---- the rules -------------------------------------------------------------------------------------------------------------------
def run_stream(name):
    begin, founds = rule_streams()[name]
    w = shadow_walk_np(**begin)
    lists = [w.ray.copy()]
    for f in founds:
        w.step(f)
        lists.append(w.ray.copy())
    return w, lists


def test_opacity_one_ends_a_ray_only_in_all_channels():
    w, lists = run_stream("opaque")
    assert [l.tolist() for l in lists] == [[0, 1, 2], [1], [1]]
    assert np.all(w.T[:, 0].view(np.uint32) == 0)
    np.testing.assert_array_equal(w.T[:, 1], np.array([0.0, 0.375, 0.375], F))
    np.testing.assert_array_equal(w.T[:, 2], 1.0)                   # no hit: the ray retires with the T it has


def test_minus_zero_ends_a_ray_as_plus_zero_does():
    w, lists = run_stream("minus_zero_T")
    assert [l.tolist() for l in lists] == [[0, 1], [], []]
    assert np.all(np.signbit(w.T[:, 0])) and np.all(w.T == 0)


def test_no_clamp():
    w, lists = run_stream("hostile_opacity")
    assert all(l.tolist() == list(range(6)) for l in lists[:-1])
    begin, founds = rule_streams()["hostile_opacity"]
    o = np.stack([f.opacity for f in founds], axis=1)              # [3, steps, rays]
    assert same_bits(w.T, fold(6, np.full(6, 3, np.uint8), o.reshape(3, -1), 3, 6))
    assert np.isnan(w.T[0, [2, 3]]).all() and np.isinf(w.T[0, [0, 1, 4, 5]]).all()


def test_t_zero_negative_and_nan_do_not_end_a_ray():
    w, lists = run_stream("t")
    assert [l.tolist() for l in lists] == [[0, 1, 2]] * 3
    assert w.maxdist[0] == 0.5 and w.maxdist[1] == 2.5 and np.isnan(w.maxdist[2])


def test_left_one_ulp_either_side_of_zero():
    w, lists = run_stream("left_ulp")
    assert [l.tolist() for l in lists] == [[0, 1, 2], [0], [0]]
    assert w.maxdist[0] == F(2.0 ** -24)


@pytest.mark.parametrize("k", [1, 2, 255])
def test_budget(k):
    begin, founds = rule_streams()[f"budget_{k}"]
    w = shadow_walk_np(**begin)
    for step in range(k):
        assert w.active == 2 and int(w.steps[0]) == k - step
        w.step(founds[step])
    assert w.active == 0
    want = F(1)
    for _ in range(k):
        want = F(want * F(0.75))
    assert w.T[0, 0] == 1 and w.T[0, 1] == want and want > 0        # out of steps, not black: the T it has


def test_begin_lists_positive_maxdist_only_and_the_rest_keep_base():
    begin, _ = rule_streams()["begin_maxdist"]
    w = shadow_walk_np(**begin)
    assert w.ray.tolist() == [3, 4] and w.steps.tolist() == [4, 4]
    assert same_bits(w.T, begin["base"])
    w, _ = run_stream("begin_maxdist")
    assert same_bits(w.T[:, :3], begin["base"][:, :3]) and same_bits(w.T[:, 3:], begin["base"][:, 3:] * F(0.5))


@pytest.mark.parametrize("name,listed", [("count_below", 3), ("count_above", 5), ("count_negative", 0)])
def test_device_count(name, listed):
    begin, _ = rule_streams()[name]
    w = shadow_walk_np(fill=-7.0, **begin)
    assert w.ray.tolist() == list(range(listed))
    assert np.all(w.T[:, :listed] == 1) and np.all(w.T[:, listed:] == -7)   # nothing at or past the count is written


def test_lanes():
    _, lists = run_stream("lanes")
    assert [len(l) for l in lists] == [197, 197, 3, 1, 0] and lists[2].tolist() == [7, 71, 135] and lists[3].tolist() == [135]
