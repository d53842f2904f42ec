"""CPU: nearest_np (tests/nearest_util.py), the float32 numpy statement of rls_nearest_hits that the GPU tests hold the device to
bit for bit, is itself held to a float64 brute force and to its rules.

Against float64 Moller-Trumbore over every triangle, on the icosphere (level 2, 320 triangles) and the 33 x 33 quad grid: the
rays aim at points whose barycentrics are at least 0.05 from every edge, from a distance of 2, at an angle to the surface of at
least asin(0.25), and the float64 winner is at least 1e-3 (in t) in front of the runner-up and 1e-3 (in barycentrics) from the
edge of every other triangle the ray passes -- the stated margins: inside them float32 cannot pick another triangle, and t agrees
within the project's 1e-5 relative bound.  Then every rule on a stream made for it (nearest_util.rule_streams, on rules_mesh)."""
import numpy as np
import pytest

import nearest_util as U
from nearest_util import F, NO_PRIM

REL = 1e-5


def _margin_rays(mesh, seed, K):
    rng = np.random.default_rng(seed)
    o, d = U.rays_at_targets(rng, U.interior_targets(rng, mesh, K), spread=2.0)
    o2, d2 = U.random_rays(rng, K)
    return np.concatenate([o, o2], axis=1), np.concatenate([d, d2], axis=1)


@pytest.mark.parametrize("name", ["icosphere", "quad_grid"])
def test_statement_against_float64(name):
    mesh = U.icosphere(2) if name == "icosphere" else U.quad_grid(33)
    assert mesh.nt == (320 if name == "icosphere" else 2 * 33 * 33)
    o, d = _margin_rays(mesh, 3, 1500)
    hit64, prim64, t64, margin = U.brute64(mesh, o, d)
    V = mesh.V.astype(np.float64)[mesh.tri[prim64].astype(np.int64)]
    n = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
    d64 = d.astype(np.float64).T
    cos = np.abs(np.einsum("kc,kc->k", n, d64)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(d64, axis=1))
    keep = (margin >= 1e-3) & (~hit64 | (cos >= 0.25))
    assert keep.sum() >= 1500 and (keep & hit64).sum() >= 1000 and (keep & ~hit64).sum() >= 50, (keep.sum(), (keep & hit64).sum())
    h = U.nearest_np(mesh, o, d)
    assert np.array_equal(h.hit[keep] != 0, hit64[keep])
    both = keep & hit64
    assert np.array_equal(h.prim[both], prim64[both].astype(np.uint32))
    rel = np.abs(h.t[both].astype(np.float64) - t64[both]) / t64[both]
    assert rel.max() <= REL, rel.max()
    # the frame: unit vectors, N perpendicular to T, P on the ray, wo = -d, barycentrics inside
    for v in (h.N, h.Ns, h.T):
        assert np.abs(np.linalg.norm(v[:, both].astype(np.float64), axis=0) - 1).max() < 1e-6
    assert np.abs(np.einsum("ck,ck->k", h.N[:, both], h.T[:, both])).max() < 1e-6
    assert np.array_equal(h.P[:, both], (o[:, both] + h.t[both] * d[:, both]).astype(F))
    assert np.array_equal(h.wo[:, both], -d[:, both])
    assert (h.u[both] >= 0).all() and (h.v[both] >= 0).all() and (h.u[both] + h.v[both] <= 1).all()
    if mesh.normals is not None:                                     # the sphere's shading normal points along the hit's position
        assert np.abs(h.Ns[:, both] - h.P[:, both] / np.linalg.norm(h.P[:, both], axis=0)).max() < 2e-2
    assert np.array_equal(h.surface[both], mesh.surface[h.prim[both]])
    # a reach: exactly t still hits, one ulp less does not
    t = h.t
    for m, want in ((t, True), (np.nextafter(t, F(0)), False)):
        g = U.nearest_np(mesh, o[:, both], d[:, both], m[both])
        if want:
            assert (g.hit != 0).all() and np.array_equal(g.t, t[both]) and np.array_equal(g.prim, h.prim[both])
        else:
            assert not np.any((g.hit != 0) & (g.prim == h.prim[both]))


@pytest.fixture(scope="module")
def rules():
    mesh = U.rules_mesh()
    return {name: (r, U.nearest_np(mesh, *r)) for name, r in U.rule_streams().items()}


def _prims(h):
    return [int(p) if k else None for k, p in zip(h.hit, h.prim)]


def test_ties_go_to_the_smaller_index(rules):
    _, h = rules["ties"]
    assert _prims(h) == [0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1]
    assert np.array_equal(h.t, np.full(12, 0.5, F))


def test_skip(rules):
    _, h = rules["skip"]
    assert _prims(h) == [0, 2, 0, 0, 0, 0, 0, 0, 1, 3, 1, 4, 0]
    assert np.array_equal(h.t, np.array([0.5] * 11 + [1.0, 2.0], F))


def test_maxdist(rules):
    (o, d, m, skip), h = rules["maxdist"]
    #        0  -0  -1  NaN inf -inf below  at  above 1e-45 3e38
    assert list(h.hit) == [0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1]
    assert np.array_equal(h.t[h.hit != 0], np.full(4, 0.5, F))


def test_flat_triangles_report_the_slab_plane(rules):
    (o, d, m, skip), h = rules["flat"]
    assert _prims(h) == [0, 0, 6, 6, 0, 0]
    axis, plane = [2, 2, 0, 0, 2, 2], F([0, 0, 2, 2, 0, 0])
    k = np.arange(6)
    want = ((plane - o[axis, k]) * (F(1) / d[axis, k])).astype(F)   # tn == tf of the flat axis: the confinement leaves no other t
    assert np.array_equal(h.t, want)


def test_degenerate_triangles_never_hit(rules):
    _, h = rules["degenerate"]
    assert _prims(h) == [None, None, None, 6]
    mesh = U.rules_mesh()
    rng = np.random.default_rng(2)
    o, d = U.rays_at_targets(rng, np.tile(np.array([[0.5, 0.25, 0.5]]), (64, 1)) + rng.normal(scale=0.02, size=(64, 3)))
    g = U.nearest_np(mesh, o, d)
    assert not np.any((g.hit != 0) & ((g.prim == 7) | (g.prim == 8)))


def test_zero_direction_components(rules):
    _, h = rules["zero_dir"]
    assert _prims(h) == [0] * 16 + [None] * 8 + [6] * 4
    assert np.array_equal(h.t[:16], np.full(16, 0.5, F)) and np.array_equal(h.t[24:], np.full(4, 3.0, F))


def test_origins_on_a_box_plane(rules):
    _, h = rules["on_box"]
    assert _prims(h) == [1, 0, 0, None, 4, 0, 6, None, None, 1, 0]
    assert np.array_equal(h.t[h.hit != 0], F([0.5, 0.5, 0.5, 1.0, 1.0, 1.25, 0.5, 0.5]))


def test_nonfinite_rays_have_no_candidate(rules):
    (o, d, m, skip), h = rules["nonfinite"]
    bad = ~(np.isfinite(o).all(axis=0) & np.isfinite(d).all(axis=0)) | (d == 0).all(axis=0)
    assert bad.sum() == 31 and not h.hit[bad].any()
    for mesh in (U.icosphere(1), U.soup(65)):
        ho, hd, hm, hs = U.hostile_rays(mesh)
        g = U.nearest_np(mesh, ho, hd, hm, hs)
        bad = ~(np.isfinite(ho).all(axis=0) & np.isfinite(hd).all(axis=0))
        assert bad.sum() == 24 and not g.hit[bad].any()
        with np.errstate(invalid="ignore"):
            assert not g.hit[~(hm > 0)].any()
        assert not np.any((g.hit != 0) & (g.prim == hs))


def test_missed_entries_hold_zero_and_an_empty_mesh_misses():
    mesh = U.single_triangle()
    o, d = F([[0.2, 5.0], [0.2, 5.0], [1.0, 1.0]]), F([[0, 0], [0, 0], [-1, -1]])
    h = U.nearest_np(mesh, o, d)
    assert list(h.hit) == [1, 0] and h.surface[0] == 3 and h.t[1] == 0 and not h.P[:, 1].any()
    assert np.array_equal(h.N[:, 0], F([0, 0, 1])) and np.array_equal(h.Ns[:, 0], h.N[:, 0]) and np.array_equal(h.T[:, 0], F([1, 0, 0]))
    e = U.nearest_np(U.empty_mesh(), o, d)
    assert not e.hit.any()


def test_np_tracer_carries_last_by_queue_ray():
    """a ray leaving a triangle it stands on does not hit it again, by `last`, not by an epsilon"""
    mesh = U.icosphere(2)
    rng = np.random.default_rng(4)
    o, d = U.rays_at_targets(rng, U.interior_targets(rng, mesh, 32), spread=2.0)
    tr = U.np_tracer(mesh, 40)
    ray = np.arange(32, dtype=np.uint32) + 8
    a = tr(ray, o, d, np.full(32, np.inf, F))
    assert (a.hit != 0).all() and np.array_equal(tr.last[8:], a.prim) and (tr.last[:8] == NO_PRIM).all()
    b = tr(ray, a.P, d, np.full(32, np.inf, F))
    assert (b.hit != 0).all() and not np.any(b.prim == a.prim)       # through the sphere: the far side
    c = tr(ray, b.P, d, np.full(32, np.inf, F))
    assert not c.hit.any() and np.array_equal(tr.last[8:], b.prim)   # a miss leaves `last`
