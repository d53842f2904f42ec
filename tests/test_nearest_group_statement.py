"""CPU: group_np (tests/nearest_group_util.py), the float32 numpy statement of rls_nearest_group_hits that the CPU program and the
GPU tests hold the traversal to bit for bit, is itself tied to the statement of the one-mesh query and to a float64 brute force.

Part 1, identity.  A group of ONE instance with identity matrices equals nearest_util.nearest_np bit for bit, on rays whose
components are finite and non-zero.  The argument: with A = I a point maps as ((1 x + 0 y) + 0 z) + 0; 0 y and 0 z are zeros of
some sign for finite y, z, and x + (+-0) = x for x != 0 (only x = -0 would become +0, hence no zero components), so o' = o,
d' = d and inv' = inv bit for bit.  B = I maps the mesh box's corners to themselves and the pad only widens it, so W contains
every triangle's box; by the monotonicity of the slab arithmetic tnW <= a triangle's own tn from 0 and tfW >= its tf from +inf,
and an interval started at (tnW, tfW) ends at the same (tn, tf) as one started at (0, +inf) -- for finite non-zero rays no end is
a NaN.  A^T n = n and B e1 = e1 the same way (a zero component of n or e1 keeps its value, and the normalisation divides it by a
positive length: the sign of a zero can differ, which is why N, Ns, T are compared by value there -- array_equal reads -0 == +0).

Part 2, exact transforms.  Translations on the grid of 1/4, single-axis mirrors and uniform power-of-two scales are exact in
float32 in both matrices; the mesh and the rays sit on dyadic grids, so every o - v0, lo - o, every corner and every mapped
vertex is exact.  Then the object-space test of instance j against (o', d') and the world-space test of the BAKED triangle
against (o, d) run the same operations on operands that differ by exact factors (a power of two s, a sign per mirrored axis, the
mirror's determinant sigma): p_w = s^2 sigma M p, det_w = s^3 sigma det, r_w = sigma s^-3 r, s_w = s M s' and so u, v, tm are
the same floats; the slab ends are the same floats with the ends swapped together with the sign of inv.  So group_np must equal
nearest_np on the baked flat mesh, triangle j nt + i, surface based:
  hit, t, P, surface: bit for bit; prim / instance: baked prim == instance * nt + prim;
  T: the same floats; a zero component may differ in sign (B e1 sums a -0 product and +0 ones where e1_w = v1_w - v0_w is +0);
  u, v: the same floats, except that a ZERO may differ in sign under a mirror: s . p is a sum of three products, and where it
      cancels exactly (a ray through an edge or a vertex, common on a dyadic grid) it is +0 on both sides -- the negated terms
      cancel to +0 too, not to -0 -- while r_w = -r; so u = +0 on one side and -0 on the other.  Compared as floats (-0 == +0);
      no other plane reads the sign (w = (1 - u) - v and u n1 + .. are the same floats for either zero);
  Ns: the same floats (zeros as for T) -- the baked mesh carries the vertex normals mapped by A as normals, (1 / s) M n, exact, and their
      interpolation is the exact image of the object-space one;
  N: equal up to the sign sigma of the instance's mirror: the baked winding is the mirrored one, e1_w x e2_w = s^2 sigma M n,
      while the statement reports A^T n = (1 / s) M n with no flip.  Compared as N_group == sigma * N_baked.

Part 3, general transforms (a rotation times a shear times a non-uniform scale of 1e-3 .. 1e3 per axis).  group_np is held to
the float64 brute force on (hit, instance, prim) and on t.  The margins are test_nearest_statement.py's: the float64 winner at
least 1e-3 (in barycentrics) inside its triangle and from the edge of every other triangle the ray passes, at least 1e-3 (in t)
in front of the runner-up, the ray at least asin(0.25) off the surface (in object space, where the test runs).  The relative
bound on t is NOT that file's 1e-5: the matrix products add their own rounding (o' = A o cancels where the world origin is far
from the instance in ITS units).  Measured on these inputs, group_np against float64: the largest relative error in t is 1.24e-5
(icosphere) and 5.9e-6 (quad grid) -- the bound asserted is 4 x the larger, 5e-5.  At most 2 % of the rays may be left out by
the margins; the fraction is asserted (measured: 1.6 % and 0.5 %).
"""
import numpy as np
import pytest

import nearest_group_util as G
import nearest_util as U
from nearest_util import F, NO_PRIM

REL_GENERAL = 5e-5


def _planes_equal(a, b, names):
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        assert np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y), k


# ---- part 1 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere", "quad_grid", "soup"])
def test_identity_instance_is_the_one_mesh_statement(name):
    mesh = {"icosphere": lambda: U.icosphere(2), "quad_grid": lambda: U.quad_grid(9), "soup": lambda: U.soup(257)}[name]()
    rng = np.random.default_rng(21)
    o, d = U.rays_at_targets(rng, U.interior_targets(rng, mesh, 300))
    o2, d2 = U.random_rays(rng, 300)
    o, d = np.concatenate([o, o2], 1), np.concatenate([d, d2], 1)
    assert np.isfinite(o).all() and np.isfinite(d).all() and (o != 0).all() and (d != 0).all()
    m = np.where(rng.random(600) < 0.3, rng.uniform(0.5, 3.0, 600), np.inf).astype(F)
    want = U.nearest_np(mesh, o, d, m)
    skip_i = np.where(rng.random(600) < 0.5, want.prim, NO_PRIM).astype(np.uint32)
    for skip, flat_skip in ((None, None), ((np.zeros(600, np.uint32), skip_i), skip_i)):
        want = U.nearest_np(mesh, o, d, m, flat_skip)
        got = G.group_np([G.Inst(mesh, G.IDENTITY, G.IDENTITY, base=0)], o, d, m, skip)
        assert (want.hit != 0).sum() > 150
        _planes_equal(got, want, ("hit", "t", "u", "v", "P", "prim", "surface", "wo"))
        assert not got.instance.any()
        for k in ("N", "Ns", "T"):
            assert np.array_equal(getattr(got, k), getattr(want, k), equal_nan=True), k   # (a sliver of the soup has n = 0)
    # a skip pair of ANOTHER instance skips nothing
    got = G.group_np([G.Inst(mesh, G.IDENTITY, G.IDENTITY)], o, d, m, (np.ones(600, np.uint32), skip_i))
    _planes_equal(got, U.nearest_np(mesh, o, d, m), ("hit", "t", "prim"))


# ---- part 2 --------------------------------------------------------------------------------------------------------------------------
def dyadic_mesh(nt=96, seed=4):
    """triangles with vertices on the grid of 1/8 in [-1, 1]^3 and vertex normals on the grid of 1/4; some share a plane"""
    rng = np.random.default_rng(seed)
    c = rng.integers(-6, 7, (nt, 1, 3))
    V = (c + rng.integers(-2, 3, (nt, 3, 3))) / 8.0
    V[::7, :, 2] = V[::7, :1, 2]                                     # flat in z: the box is a slab
    return U.Mesh(V.reshape(-1, 3), np.arange(3 * nt).reshape(nt, 3), surface=rng.integers(0, 9, nt),
                  normals=rng.integers(-4, 5, (3 * nt, 3)) / 4.0 + np.array([0, 0, 2.0]))


def dyadic_rays(rng, K, box=5):
    o = rng.integers(-4 * box, 4 * box + 1, (3, K)) / 4.0
    d = rng.integers(-8 * box, 8 * box + 1, (3, K)) / 8.0 - o
    return o.astype(F), d.astype(F)


def test_exact_transforms_equal_the_baked_flat_mesh():
    mesh = dyadic_mesh()
    insts = G.exact_instances(mesh, 6) + [G.exact_instances(mesh, 1)[0]]         # the last coincides with the first: ties
    insts[-1].base = 7
    for i in insts:                                                  # both matrices are exact, and inverses of each other
        L, t = i.B.astype(np.float64)[:, :3], i.B.astype(np.float64)[:, 3]
        assert np.array_equal(i.A.astype(np.float64)[:, :3] @ L, np.eye(3)) and np.array_equal(i.A.astype(np.float64)[:, :3] @ t, -i.A.astype(np.float64)[:, 3])
    flat = G.bake(insts)
    nt = mesh.nt
    rng = np.random.default_rng(9)
    o, d = dyadic_rays(rng, 3000)
    m = np.where(rng.random(3000) < 0.3, rng.integers(1, 12, 3000) / 8.0, np.inf).astype(F)
    first = U.nearest_np(flat, o, d, m)
    assert (first.hit != 0).sum() > 600
    sigma = np.array([np.sign(np.linalg.det(i.B[:, :3].astype(np.float64))) for i in insts], F)
    assert (sigma < 0).any() and (sigma > 0).any()
    skip_flat = np.where(rng.random(3000) < 0.5, first.prim, NO_PRIM).astype(np.uint32)
    for flat_skip in (None, skip_flat):
        want = U.nearest_np(flat, o, d, m, flat_skip)
        skip = None if flat_skip is None else (np.where(flat_skip == NO_PRIM, G.NO_INSTANCE, flat_skip // nt).astype(np.uint32),
                                                np.where(flat_skip == NO_PRIM, NO_PRIM, flat_skip % nt).astype(np.uint32))
        got = G.group_np(insts, o, d, m, skip)
        _planes_equal(got, want, ("hit", "t", "P", "surface", "wo"))
        for k in ("u", "v", "T", "Ns"):
            assert np.array_equal(getattr(got, k), getattr(want, k), equal_nan=True), k
        hit = want.hit != 0
        assert np.array_equal(got.instance[hit].astype(np.int64) * nt + got.prim[hit], want.prim[hit])
        assert np.array_equal(got.N[:, hit], want.N[:, hit] * sigma[got.instance[hit]], equal_nan=True)
        last = got.instance[hit] == len(insts) - 1
        if flat_skip is None:                                        # a tie goes to the smaller j ..
            assert (got.instance[hit] == 0).sum() > 20 and not last.any()
        else:                                                        # .. and the coincident copy takes over where (0, i) is skipped
            assert last.sum() > 20 and np.array_equal(skip[0][hit][last], np.zeros(last.sum(), np.uint32))


# ---- part 3 --------------------------------------------------------------------------------------------------------------------------
def general_case(name, seed, offset):
    """six placements whose sizes run from 1e-3 to 1e3 in overlapping pairs (nearest_group_util.wide_instances: a rotation times a
    shear times a non-uniform scale each), 400 rays per instance aimed in ITS space at points inside its triangles from within the
    cone of cos >= 0.3 about the normal, mapped to the world.  A placement is as far from the origin as it is large: float32
    cannot resolve a millimetre-sized instance a kilometre from the origin (to_object times the world origin cancels), and
    the seeds and offsets below are ones for which the margins leave out at most 2 % of the rays."""
    return G.wide_case(U.icosphere(2) if name == "icosphere" else U.quad_grid(17), seed, offset)


@pytest.mark.parametrize("name,seed,offset", [("icosphere", 2, 3.0), ("quad_grid", 5, 1.0)])
def test_general_transforms_against_float64(name, seed, offset):
    insts, o, d = general_case(name, seed, offset)
    hit64, j64, i64, t64, margin = G.brute64(insts, o, d)
    cos = np.ones(o.shape[1])
    for j, ins in enumerate(insts):
        at = np.nonzero(hit64 & (j64 == j))[0]
        V = ins.mesh.V.astype(np.float64)[ins.mesh.tri[i64[at]].astype(np.int64)]
        n = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
        dd = (ins.A.astype(np.float64)[:, :3] @ d[:, at].astype(np.float64)).T
        cos[at] = np.abs(np.einsum("kc,kc->k", n, dd)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(dd, axis=1))
    keep = (margin >= 1e-3) & (~hit64 | (cos >= 0.25))
    left_out = 1.0 - keep.mean()
    print(f"{name}: left out {left_out:.4f}, hits kept {(keep & hit64).sum()}")
    assert left_out <= 0.02, left_out
    assert (keep & hit64).sum() >= 1000
    h = G.group_np(insts, o, d)
    assert np.array_equal(h.hit[keep] != 0, hit64[keep])
    both = keep & hit64
    assert np.array_equal(h.instance[both], j64[both].astype(np.uint32))
    assert np.array_equal(h.prim[both], i64[both].astype(np.uint32))
    rel = np.abs(h.t[both].astype(np.float64) - t64[both]) / t64[both]
    print(f"{name}: largest relative error in t {rel.max():.3e}")
    assert rel.max() <= REL_GENERAL, rel.max()
    assert len(np.unique(h.instance[both])) == len(insts)
    base = np.array([i.base for i in insts])
    sid = np.zeros(both.sum(), np.int64) if insts[0].mesh.surface is None else insts[0].mesh.surface[h.prim[both]].astype(np.int64)
    assert np.array_equal(h.surface[both], (sid + base[h.instance[both]]).astype(np.uint32))
    for v in (h.N, h.Ns, h.T):
        assert np.abs(np.linalg.norm(v[:, both].astype(np.float64), axis=0) - 1).max() < 1e-6


# ---- the world box and parking -------------------------------------------------------------------------------------------------------
def test_world_box_encloses_the_exactly_mapped_box():
    mesh = U.icosphere(1)
    for ins in G.general_instances(mesh, 40, seed=2, scales=(1e-3, 1e3)):
        lo, hi = G.mesh_box(mesh)
        c = np.array([[hi[k] if b & (1 << k) else lo[k] for k in range(3)] for b in range(8)], np.float64)
        w = c @ ins.B[:, :3].astype(np.float64).T + ins.B[:, 3].astype(np.float64)
        assert not ins.parked and (ins.wlo <= w.min(axis=0)).all() and (ins.whi >= w.max(axis=0)).all()


def test_parked_instances_never_hit():
    mesh = U.icosphere(1)
    o, d = U.random_rays(np.random.default_rng(1), 200)
    nanA, infB = G.IDENTITY.copy(), G.IDENTITY.copy()
    nanA[1, 2], infB[0, 3] = np.nan, np.inf
    huge = G.IDENTITY * F(3e38)
    huge[:, 3] = F(3e38)                                             # the corners overflow: W is not finite
    insts = [G.Inst(mesh, G.IDENTITY, nanA), G.Inst(mesh, infB, G.IDENTITY), G.Inst(U.empty_mesh()), G.Inst(mesh, huge, G.IDENTITY)]
    assert [i.parked for i in insts] == [True, True, True, True]
    assert not G.group_np(insts, o, d).hit.any()
    live = G.group_np(insts + [G.Inst(mesh, base=5)], o, d)
    assert live.hit.any() and (live.instance[live.hit != 0] == 4).all()
    # a singular to_object is no reason to park: d' = 0, no candidate
    flatA = G.IDENTITY.copy()
    flatA[:, :3] = 0
    one = G.Inst(mesh, G.IDENTITY, flatA)
    assert not one.parked and not G.group_np([one], o, d).hit.any()
