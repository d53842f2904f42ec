"""-m gpu: the grid and plane edges of the any-hit launch (librls_nearest_any.so), as test_gpu_nearest_group_edges.py has them for
the group query.
  A. two and a half grid rounds on a context capped at one workgroup per CU (RLS_BLOCKS_PER_CU=1) and a last tile of ONE ray,
     with a mixed flag table under surfaces past it, a permuted ray plane (visibility, reach and last go by ray id), a base and
     reaches: the bytes of every plane equal the default context's, and any_np's (tests/nearest_any_util.py) on windows about the
     round boundaries and the tail;
  B. every subset of the optional planes {via, maxdist, ray, last, visibility, base (only with visibility), reach} -- the kernel
     tests them through one bit mask inside its tile loop -- at 300 rays on the icosphere with mixed flags: 96 launches, each
     held to any_np; planes not asked for are absent, the sentinel guards intact, `last` unchanged.
Every plane lives inside a sentinel-filled buffer (test_gpu_nearest.Guarded)."""
import itertools

import numpy as np
import pytest
import torch

import rlshaders_amd as R
import nearest_any_util as A
import nearest_util as U
from nearest_any_util import BLOCKED, CLEAR, VEILED, any_np
from nearest_util import F, NO_PRIM
from test_gpu_nearest import Guarded, _dev, _host, _ids, mixed_rays
from test_gpu_nearest_any import SENT32, base_of, bits

pytestmark = pytest.mark.gpu
TILE = 256
FLAGS = np.array([1, 0, 0, 1], np.uint8)                             # surfaces 4 and 5 read the last entry


@pytest.fixture(scope="module")
def ctx():
    from rlshaders_amd import nearest_any
    nearest_any.load()                                               # (a missing library is an error, not a build)
    c = R.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def one_block_per_cu():
    """a context whose grids are capped at one workgroup per CU (RLS_BLOCKS_PER_CU, read at context creation)"""
    mp = pytest.MonkeyPatch()
    mp.setenv("RLS_BLOCKS_PER_CU", "1")
    try:
        c = R.Context(0)
    finally:
        mp.undo()
    yield c
    c.close()


@pytest.fixture(scope="module")
def sphere(ctx):
    """the icosphere with surfaces 0 .. 5 by triangle, and its scene"""
    from rlshaders_amd import nearest
    ico = U.icosphere(2)
    mesh = U.Mesh(ico.V, ico.tri, surface=(np.arange(ico.nt) % 6).astype(np.uint32), normals=ico.normals)
    scene = nearest.Scene(ctx, mesh.V, mesh.tri, surface=mesh.surface, normals=mesh.normals)
    yield mesh, scene
    scene.close()


def launch(scene, o, d, m, last0, base, ids, width, use_ctx, via=None, table=None, visibility=True, reach=True):
    """one guarded launch -> (Found, state, visibility, reach, the visibility plane's bytes ahead of the launch); last0, base: by
    ray id over `width` entries, or None.  The guards are checked here, and that last and base were read, never written."""
    from rlshaders_amd import nearest, nearest_any
    n = d.shape[1]
    alloc = Guarded()
    state = alloc((n,), torch.uint8)
    vis = alloc((3, width), torch.float32) if visibility else None
    rch = alloc((width,), torch.float32) if reach else None
    last = None
    if last0 is not None:
        last = alloc((width,), torch.int32)
        last.copy_(_ids(last0))
    base_t = None
    if base is not None:
        base_t = alloc((3, width), torch.float32)
        base_t.copy_(_dev(base))
    vis0 = None if vis is None else bits(vis).copy()
    r = nearest.Rays(_dev(o if table is None else table), _dev(d), None if m is None else _dev(m), via=None if via is None else _ids(via),
                     ray=None if ids is None else _ids(ids), rays=n)
    f = nearest_any.hits(scene, r, opaque=_dev(FLAGS), base=base_t, last=last, state=state, visibility=vis if visibility else False,
                         reach=rch if reach else False, ctx=use_ctx)
    torch.cuda.synchronize()
    alloc.check()
    if last is not None:
        assert np.array_equal(_host(last).view(np.uint32), np.asarray(last0).astype(np.uint32))      # read, never written
    if base_t is not None:
        assert np.array_equal(bits(base_t), A.bits(base))
    return f, state, vis, rch, vis0


# ---- A ----------------------------------------------------------------------------------------------------------------------------------
def test_two_and_a_half_grid_rounds_and_a_last_tile_of_one_ray(ctx, one_block_per_cu, sphere):
    mesh, scene = sphere
    cu = one_block_per_cu.device_info()["compute_units"]
    grid = (cu + 7) // 8 * 8                                        # the workgroups of a capped launch
    n = 2 * grid * TILE + grid * TILE // 2 + 1                      # the last tile holds one ray
    assert n % TILE == 1 and n / TILE / grid >= 2.4
    bo, bd, bm, bs = mixed_rays(mesh, 4096, 43)
    reps = -(-n // 4096)
    o, d = np.tile(bo, (1, reps))[:, :n].copy(), np.tile(bd, (1, reps))[:, :n].copy()
    m, skip = np.tile(bm, reps)[:n].copy(), np.tile(bs, reps)[:n].copy()
    o += (np.arange(n, dtype=F) * F(1e-6))[None, :]                 # no two rays alike
    rng = np.random.default_rng(44)
    width = n + 40
    ids = rng.permutation(width)[:n].astype(np.uint32)               # visibility, reach and last go by these
    last0 = np.full(width, NO_PRIM, np.uint32)
    last0[ids] = skip
    base = base_of(rng, width)
    _, sa, va, ra, _ = launch(scene, o, d, m, last0, base, ids, width, ctx)
    _, sb, vb, rb, vis0 = launch(scene, o, d, m, last0, base, ids, width, one_block_per_cu)
    assert np.array_equal(_host(sa), _host(sb)) and np.array_equal(bits(va), bits(vb)) and np.array_equal(bits(ra), bits(rb))
    state = _host(sb)
    assert (state == BLOCKED).mean() > 0.2 and (state == VEILED).mean() > 0.05 and (state == CLEAR).mean() > 0.05
    unused = np.ones(width, bool)
    unused[ids] = False
    assert unused.sum() == 40 and np.array_equal(bits(vb)[:, unused], vis0[:, unused]) and (bits(rb)[unused] == SENT32).all()
    for lo in [max(k * grid * TILE - 256, 0) for k in (1, 2)] + [n - 512]:
        hi = min(lo + 512, n)
        at = ids[lo:hi].astype(np.int64)
        want = any_np(mesh, o[:, lo:hi], d[:, lo:hi], m[lo:hi], skip[lo:hi], flags=FLAGS, base=base, ray=at, ids=width)
        assert np.array_equal(state[lo:hi], want.state), (lo, np.flatnonzero(state[lo:hi] != want.state)[:8])
        assert np.array_equal(bits(vb)[:, at], A.bits(want.visibility)[:, at]) and np.array_equal(bits(rb)[at], A.bits(want.reach)[at]), lo
        assert len(set(want.state)) == 3


# ---- B ----------------------------------------------------------------------------------------------------------------------------------
N = 300
WIDTH = 400


@pytest.fixture(scope="module")
def subset_stream(sphere):
    """300 rays, a permuted ray plane over 400 ids, a `last` plane by id and by entry, a via table, and the statement's states
    for the four (maxdist, last) combinations the states depend on"""
    mesh, _ = sphere
    o, d, m, skip = mixed_rays(mesh, N, 47)
    rng = np.random.default_rng(48)
    ids = rng.permutation(WIDTH)[:N].astype(np.uint32)
    perm = rng.permutation(N).astype(np.uint32)
    table = np.empty_like(o)
    table[:, perm] = o                                               # the origins in another order: via[k] = perm[k]
    states = {(md, la): any_np(mesh, o, d, m if md else None, skip if la else None, flags=FLAGS).state for md in (0, 1) for la in (0, 1)}
    full = any_np(mesh, o, d, m, skip, flags=FLAGS, ray=ids.astype(np.int64), ids=WIDTH)     # (derived is any_np's own tail)
    again = A.derived(states[1, 1], m, None, ids.astype(np.int64), WIDTH)
    assert np.array_equal(A.bits(full.visibility), A.bits(again.visibility)) and np.array_equal(A.bits(full.reach), A.bits(again.reach))
    assert len({s.tobytes() for s in states.values()}) == 4          # a reach and a skip each change something
    for s in states.values():
        assert (s == BLOCKED).sum() > 100 and (s == VEILED).sum() > 20 and (s == CLEAR).sum() > 10
    return o, d, m, skip, ids, perm, table, states


OPTIONAL = ("via", "maxdist", "ray", "last", "reach")


@pytest.mark.parametrize("derived", ["state alone", "visibility", "visibility over a base"])
def test_every_subset_of_the_optional_planes(ctx, sphere, subset_stream, derived):
    mesh, scene = sphere
    o, d, m, skip, ids, perm, table, states = subset_stream
    rng = np.random.default_rng(49)
    for pick in itertools.product((0, 1), repeat=len(OPTIONAL)):
        has = dict(zip(OPTIONAL, pick))
        width = WIDTH if has["ray"] else N
        ray = ids.astype(np.int64) if has["ray"] else np.arange(N, dtype=np.int64)
        last0 = None
        if has["last"]:
            last0 = rng.integers(0, mesh.nt, width).astype(np.uint32)                # ids no entry names hold other triangles
            last0[ray] = skip
        base = base_of(rng, width) if derived == "visibility over a base" else None
        f, state, vis, reach, vis0 = launch(scene, o, d, m if has["maxdist"] else None, last0, base, ids if has["ray"] else None, width, ctx,
                                            via=perm if has["via"] else None, table=table if has["via"] else None,
                                            visibility=derived != "state alone", reach=bool(has["reach"]))
        what = (derived, has)
        assert f.state is state and (f.visibility is None) == (derived == "state alone") and (f.reach is None) == (not has["reach"]), what
        # any_np over these rays: its states depend on (maxdist, last) alone, its derived planes are A.derived of them
        want = A.derived(states[has["maxdist"], has["last"]], m if has["maxdist"] else np.full(N, np.inf, F), base, ray, width)
        assert np.array_equal(_host(state), want.state), (what, np.flatnonzero(_host(state) != want.state)[:8])
        if vis is not None:
            exp = vis0.copy()                                        # ids no entry names keep the sentinel
            exp[:, want.written] = A.bits(want.visibility)[:, want.written]
            assert np.array_equal(bits(vis), exp), what
        if reach is not None:
            exp = np.full(width, SENT32)
            exp[want.written] = A.bits(want.reach)[want.written]
            assert np.array_equal(bits(reach), exp), what
            if not has["maxdist"]:
                assert np.isinf(want.reach[ray][want.state == VEILED]).all()
