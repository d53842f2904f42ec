"""-m gpu: rls_nearest_group_hits (librls_nearest_group.so) over placements the device had not seen -- each held to group_np
(tests/nearest_group_util.py) in EVERY plane over EVERY ray, bit for bit with no NaN allowance (check_exact), inside
sentinel-filled buffers:
  1. coincident instances: instance 0 again as 2 and 5, 1 again as 4.  Every hit of 0 or 1 is a tie; the smaller j wins it, and a
     second query with the winners as the skip pair returns the next copy (2 for 0, 4 for 1) at the same t bits;
  2. exact placements with mirrors over a dyadic mesh: the device also equals the ONE-MESH device query over the baked flat mesh
     in hit and t, in prim and instance through j * nt + i, and N is that query's N times the mirror's sign -- not flipped;
  3. sizes from 1e-3 to 1e3 (wide_case) for the icosphere and the quad grid;
  4. singular to_object matrices of rank 2, rank 1 and an all-zero linear part beside live instances: the object ray has zero
     components (inv is infinite), and over a mesh whose vertex normals all lie along the lost axis Ns = normalize(0);
  5. to_object that is NOT the inverse of to_world: the traversal follows A, the world box and T follow B;
  6. member scenes with degenerate triangles and slivers, the rules' mesh and the soup as two scenes of leaf sizes 1 and 4 in
     one group: a triangle with a repeated vertex has e1 x e2 = 0 exactly and N = normalize(0).
In cases 4 and 6 alone, and in the frame planes N, Ns, T alone, a NaN of the statement matches any NaN
(trace_sss_util.same_bits_or_both_nan); the number of such entries is asserted and is the statement's own NaN count.  The hit
fractions, ties, mirrored hits and NaN frames asserted below are group_np's on these streams, computed without the device."""
import numpy as np
import pytest

import rlshaders_amd as R
import nearest_group_util as G
import nearest_util as U
from nearest_group_util import group_rays
from nearest_util import F, NO_PRIM
from test_gpu_nearest import _host, untouched
from test_gpu_nearest import query as flat_query
from test_gpu_nearest_group import SCALAR, VEC, DeviceGroup, query
from test_nearest_group_statement import dyadic_mesh, dyadic_rays
from trace_sss_util import same_bits_or_both_nan

pytestmark = pytest.mark.gpu
FRAME = ("N", "Ns", "T")
SINGULAR_HITS = 300                                                  # hits of the rank 2 and the rank 1 instance: 3 NaN words of Ns each
DEGENERATE_NANS = 282                                                # 94 hits of triangles with e2 == e1: 3 NaN words of N each


@pytest.fixture(scope="module")
def ctx():
    from rlshaders_amd import nearest, nearest_group
    nearest.load(), nearest_group.load()                             # (a missing library is an error, not a build)
    c = R.Context(0)
    yield c
    c.close()


def check_exact(f, h, what, nan_frames=None):
    """every plane of the device's Found f against the statement's Hits h over every ray: the same bits, no exclusions; entries
    without a hit untouched.  nan_frames: the number of NaN words the statement holds in N, Ns, T (cases 4 and 6) -- those planes
    then go through same_bits_or_both_nan, and the device holds NaNs at exactly those words."""
    n = f.rays
    assert n == h.hit.shape[0]
    assert np.array_equal(_host(f.hit), h.hit), (what, "hit")
    hit = h.hit != 0
    nans = 0
    for name in ("t",) + VEC + SCALAR:
        t, want = getattr(f, name), getattr(h, name)
        got = np.ascontiguousarray(_host(t)[..., hit]).view(np.uint32)
        want = np.ascontiguousarray(want[..., hit])
        if nan_frames is not None and name in FRAME:
            nans += int(np.isnan(want).sum())
            same_bits_or_both_nan(got.view(F), want, (what, name))
        else:
            assert not (want.dtype == F and np.isnan(want).any() and name in FRAME), (what, name, "a NaN frame outside cases 4 and 6")
            bad = got != want.view(np.uint32)
            assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        untouched(t, ~hit, (what, name, "missed"))
    assert nans == (nan_frames or 0), (what, "NaN words in the frame planes", nans)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------
def coincident_case():
    insts = G.coincident()
    o, d, m = group_rays(insts, 960, seed=10)
    first = G.group_np(insts, o, d, m)
    skip = (np.where(first.hit != 0, first.instance, G.NO_INSTANCE).astype(np.uint32),
            np.where(first.hit != 0, first.prim, NO_PRIM).astype(np.uint32))
    return insts, (o, d, m), first, skip, G.group_np(insts, o, d, m, skip)


def test_coincident_instances_tie_to_the_smaller_index(ctx):
    insts, (o, d, m), first, skip, second = coincident_case()
    hit = first.hit != 0
    assert 0.2 < hit.mean() < 0.98
    # the statement's own account of the ties: a winner among 0, 1 has its copy at the same t bits behind it
    copied = hit & np.isin(first.instance, (0, 1))
    nxt = np.where(first.instance == 0, 2, 4)
    tie = copied & (second.hit != 0) & (second.instance == nxt) & (second.prim == first.prim) & (second.t.view(np.uint32) == first.t.view(np.uint32))
    assert tie.sum() == copied.sum() == 462 and not np.isin(first.instance[hit], (2, 4, 5)).any()
    g = DeviceGroup(ctx, insts)
    try:
        f, last, last_instance = query(ctx, g.group, o, d, m, (np.full(o.shape[1], G.NO_INSTANCE, np.uint32), np.full(o.shape[1], NO_PRIM, np.uint32)))
        check_exact(f, first, "coincident")
        assert np.array_equal(_host(last_instance).view(np.uint32), skip[0]) and np.array_equal(_host(last).view(np.uint32), skip[1])
        f2, _, _ = query(ctx, g.group, o, d, m, skip)                # the winners skipped: the next copy takes the tie
        check_exact(f2, second, "coincident, winners skipped")
        assert np.array_equal(_host(f2.instance).view(np.uint32)[tie], nxt[tie].astype(np.uint32))
        assert np.array_equal(_host(f2.t).view(np.uint32)[tie], _host(f.t).view(np.uint32)[tie])
    finally:
        g.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------
def exact_case():
    mesh = dyadic_mesh()
    insts = G.exact_instances(mesh, 6)
    o, d = dyadic_rays(np.random.default_rng(9), 1536, box=2)
    m = np.where(np.random.default_rng(10).random(1536) < 0.3, np.random.default_rng(11).integers(1, 12, 1536) / 8.0, np.inf).astype(F)
    return mesh, insts, (o, d, m), G.group_np(insts, o, d, m)


def test_exact_placements_with_mirrors_equal_the_baked_mesh_on_the_device(ctx):
    from rlshaders_amd import nearest
    mesh, insts, (o, d, m), h = exact_case()
    hit = h.hit != 0
    sigma = np.array([np.sign(np.linalg.det(i.B[:, :3].astype(np.float64))) for i in insts], F)
    mirrored = hit & (sigma[h.instance] < 0)
    assert 0.2 < hit.mean() < 0.98 and list(sigma) == [1, -1, 1, 1, -1, 1] and mirrored.sum() == 186
    flat = G.bake(insts)
    g = DeviceGroup(ctx, insts)
    scene = nearest.Scene(ctx, flat.V, flat.tri, surface=flat.surface, normals=flat.normals)
    try:
        f, _, _ = query(ctx, g.group, o, d, m)
        check_exact(f, h, "exact")
        b, _, _ = flat_query(ctx, scene, o, d, m)
        assert np.array_equal(_host(b.hit), _host(f.hit))
        for name in ("t", "P", "surface", "wo"):
            assert np.array_equal(np.ascontiguousarray(_host(getattr(b, name))[..., hit]).view(np.uint32),
                                  np.ascontiguousarray(_host(getattr(f, name))[..., hit]).view(np.uint32)), name
        assert np.array_equal(_host(f.instance)[hit].astype(np.int64) * mesh.nt + _host(f.prim)[hit], _host(b.prim)[hit])
        # no flip under a mirror: the baked triangle has the mirrored winding, the group reports A^T n
        assert np.array_equal(_host(f.N)[:, hit], _host(b.N)[:, hit] * sigma[h.instance[hit]])
        assert (np.abs(_host(f.N)[:, mirrored]).max(axis=0) > 0.5).all()
    finally:
        scene.close()
        g.close()


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed,offset,hits", [("icosphere", 2, 3.0, 945), ("quad_grid", 5, 1.0, 1028)])
def test_sizes_across_six_decades(ctx, name, seed, offset, hits):
    insts, o, d = G.wide_case(U.icosphere(2) if name == "icosphere" else U.quad_grid(17), seed, offset, K=200)
    d[:, ::4] = -d[:, ::4]                                           # every fourth ray leaves the triangle it was aimed at
    h = G.group_np(insts, o, d)
    assert (h.hit != 0).sum() == hits and 0.2 < (h.hit != 0).mean() < 0.98 and len(np.unique(h.instance[h.hit != 0])) == 6
    g = DeviceGroup(ctx, insts)
    try:
        check_exact(query(ctx, g.group, o, d)[0], h, name)
    finally:
        g.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------
def singular_case():
    """three live placements of an icosphere whose vertex normals are all (0, 1, 0), and three more under the first three's
    to_world whose to_object has lost rows of its linear part: row 1 (rank 2), rows 1 and 2 (rank 1), all three (no ray moves:
    no hit).  Where row 1 is lost A^T s = 0 for every interpolated normal s: Ns = normalize(0), three NaN words a hit."""
    ico = U.icosphere(1)
    mesh = U.Mesh(ico.V, ico.tri, surface=ico.surface, normals=np.tile(F([0, 1, 0]), (ico.V.shape[0], 1)))
    live = G.general_instances(mesh, 3, seed=12)
    out = list(live)
    for k, rows in enumerate(((1,), (1, 2), (0, 1, 2))):
        A = live[k].A.copy()
        A[list(rows), :3] = 0
        out.append(G.Inst(mesh, live[k].B, A, base=100 + 10 * k))
    o, d, m = group_rays(out, 960, seed=14)
    return out, (o, d, m), G.group_np(out, o, d, m)


def test_singular_to_object(ctx):
    insts, (o, d, m), h = singular_case()
    hit = h.hit != 0
    flat = hit & np.isin(h.instance, (3, 4))
    assert not any(i.parked for i in insts) and 0.2 < hit.mean() < 0.98
    assert flat.sum() == SINGULAR_HITS and not (hit & (h.instance == 5)).any()
    assert np.isnan(h.Ns[:, flat]).all() and not np.isnan(h.N).any() and not np.isnan(h.T).any() and not np.isnan(h.Ns[:, hit & ~flat]).any()
    g = DeviceGroup(ctx, insts)
    try:
        check_exact(query(ctx, g.group, o, d, m)[0], h, "singular", nan_frames=3 * SINGULAR_HITS)
    finally:
        g.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------
def unrelated_case():
    """to_object the inverse of ANOTHER placement than to_world: a further linear map within 0.4 of the identity and a shift of up to 0.8"""
    mesh = U.icosphere(2)
    rng = np.random.default_rng(15)
    out = []
    for j, i in enumerate(G.general_instances(mesh, 5, seed=16)):
        other = G.Inst(mesh, G.affine((np.eye(3) + rng.uniform(-0.4, 0.4, (3, 3))) @ i.B[:, :3].astype(np.float64),
                                      i.B[:, 3].astype(np.float64) + rng.uniform(-0.8, 0.8, 3)))
        out.append(G.Inst(mesh, i.B, other.A, base=10 * j))
    o, d, m = group_rays(out, 960, seed=17)
    return out, (o, d, m), G.group_np(out, o, d, m)


def test_to_object_that_is_not_the_inverse_of_to_world(ctx):
    insts, (o, d, m), h = unrelated_case()
    hit = h.hit != 0
    assert 0.2 < hit.mean() < 0.98
    # the two matrices are used independently: with to_world the inverse of to_object instead, other boxes and other tangents
    paired = G.group_np([G.Inst(i.mesh, np.linalg.inv(np.vstack([i.A.astype(np.float64), [0, 0, 0, 1]]))[:3], i.A, base=i.base) for i in insts], o, d, m)
    both = hit & (paired.hit != 0) & (paired.instance == h.instance) & (paired.prim == h.prim)
    assert both.sum() == 415 and (h.T[:, both] != paired.T[:, both]).any(axis=0).sum() == 415
    assert np.array_equal(h.N[:, both].view(np.uint32), paired.N[:, both].view(np.uint32))       # N follows A alone
    assert (hit != (paired.hit != 0)).sum() == 9                                                  # the box follows B
    g = DeviceGroup(ctx, insts)
    try:
        check_exact(query(ctx, g.group, o, d, m)[0], h, "unrelated")
    finally:
        g.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------
def degenerate_case():
    """the rules' mesh and the 1025-triangle soup, three placements each, the first of each the identity.  256 rays go through
    vertex 0 of the soup's triangles with a repeated vertex (by index or by position: e2 == e1, so e1 x e2 = 0 exactly) under the
    identity placement, from o = v0 - d / 1024 along a d of few bits: o - v0 is exact, the rounded determinant e1 . (d x e1) is
    a residue that is seldom 0, u == v is a ratio of two such residues and about half of these rays hit -- at N = normalize(0)"""
    rules, soup = U.rules_mesh(), U.soup(1025)
    a, b = G.general_instances(rules, 3, seed=18, spread=1.5), G.general_instances(soup, 3, seed=19, spread=1.5)
    a[0], b[0] = G.Inst(rules, G.IDENTITY, G.IDENTITY), G.Inst(soup, G.IDENTITY, G.IDENTITY)
    insts = [v for pair in zip(a, b) for v in pair]
    for k, i in enumerate(insts):
        i.base = 1000 * k
    o, d, m = group_rays(insts, 960, seed=20)
    rng = np.random.default_rng(21)
    K = 256
    repeated = np.array([i for i in range(0, soup.nt, 16) if (i // 16) % 3 != 1])
    v0 = soup.V[soup.tri[rng.choice(repeated, K), 0].astype(np.int64)]
    dd = (rng.integers(1, 9, (K, 3)) * rng.choice([-1, 1], (K, 3)) / 8.0).astype(F)
    o[:, :K], d[:, :K], m[:K] = (v0 - dd / F(1024)).astype(F).T, dd.T, np.inf
    return insts, (o, d, m), G.group_np(insts, o, d, m)


def test_member_scenes_with_degenerate_triangles(ctx):
    from rlshaders_amd import nearest, nearest_group
    insts, (o, d, m), h = degenerate_case()
    hit = h.hit != 0
    nan = int(sum(np.isnan(getattr(h, k)[:, hit]).sum() for k in FRAME))
    assert 0.2 < hit.mean() < 0.98 and len(np.unique(h.instance[hit])) == 6 and nan == DEGENERATE_NANS
    scenes = {}
    for i, leaf in ((insts[0], 1), (insts[1], 4)):
        scenes[id(i.mesh)] = nearest.Scene(ctx, i.mesh.V, i.mesh.tri, surface=i.mesh.surface, normals=i.mesh.normals, leaf_size=leaf)
    group = nearest_group.Group(ctx, [nearest_group.Instance(scenes[id(i.mesh)], i.B, surface_base=i.base, to_object=i.A) for i in insts])
    try:
        assert group.info()["scenes"] == 2 and sorted(s.leaf_size for s in scenes.values()) == [1, 4]
        check_exact(query(ctx, group, o, d, m)[0], h, "degenerate", nan_frames=DEGENERATE_NANS)
    finally:
        group.close()
        for s in scenes.values():
            s.close()

