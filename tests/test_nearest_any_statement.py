"""CPU: any_np (tests/nearest_any_util.py), the float32 numpy statement of rls_nearest_any_hits that the GPU tests hold the device
to bit for bit, is held to the nearest-hit statement, to a float64 brute force and to its own rules; and the header carries the
statement.

state != 0 exactly where nearest_np hits (both are "the candidate set is not empty"); with every triangle opaque state == hit;
the flag of a surface at or past the table's end is the table's last; reach and visibility are held bit for bit with base
absent, given, -0, inf and NaN; on rays kept clear of edges (the margins of test_nearest_statement.py) the state agrees with
float64 Moller-Trumbore over every triangle."""
import numpy as np
import pytest

import nearest_any_util as A
import nearest_util as U
from nearest_any_util import BLOCKED, CLEAR, VEILED, any_np, bits
from nearest_util import F, NO_PRIM
from trace_abi_util import ROOT

HEADER = ROOT / "include" / "rlshaders_amd_nearest_any.h"


def _streams(mesh, seed, K=400):
    rng = np.random.default_rng(seed)
    o, d = U.rays_at_targets(rng, U.interior_targets(rng, mesh, K), spread=2.0) if mesh.nt else U.random_rays(rng, K)
    o2, d2 = U.random_rays(rng, K)
    ho, hd, hm, hs = U.hostile_rays(mesh)
    o, d = np.concatenate([o, o2, ho], 1), np.concatenate([d, d2, hd], 1)
    m = np.concatenate([rng.uniform(0.5, 4.0, 2 * K).astype(F), hm])
    m[rng.random(m.size) < 0.3] = np.inf
    skip = np.concatenate([np.full(2 * K, NO_PRIM, np.uint32), hs])
    return o, d, m, skip


MESHES = {"icosphere": lambda: U.icosphere(2), "quad_grid": lambda: U.quad_grid(9), "soup": lambda: U.soup(257), "rules": U.rules_mesh,
          "empty": U.empty_mesh, "single": U.single_triangle}


def test_the_header_states_the_result():
    text = HEADER.read_text()
    for must in ("THE STATEMENT", "blocked", "veiled", "clear", "NO BLOCKING PRIMITIVE", "NEVER WRITTEN", "NO BIT-FOR-BIT CLAIM", "BORROWED",
                 "min(surface_i, opaque_count - 1)", "b_c * 0.0f", "rls_shadow_walk_found.index"):
        assert must in text, must
    assert "the test hits, t_i > 0 and t_i <= m" in text


@pytest.mark.parametrize("name", list(MESHES))
def test_state_is_the_nearest_statements_hit(name):
    mesh = MESHES[name]()
    o, d, m, skip = _streams(mesh, 7)
    h = U.nearest_np(mesh, o, d, m, skip)
    rng = np.random.default_rng(1)
    for flags in (None, np.ones(4, np.uint8), np.array([1, 0, 0, 1], np.uint8), np.zeros(3, np.uint8), rng.integers(0, 2, 301).astype(np.uint8)):
        a = any_np(mesh, o, d, m, skip, flags=flags)
        assert np.array_equal(a.state != CLEAR, h.hit != 0)
        if flags is None or flags.all():
            assert np.array_equal(a.state, h.hit)                    # every triangle opaque: blocked exactly where there is a hit
        if flags is not None and not flags.any():
            assert not (a.state == BLOCKED).any()
        assert np.array_equal(a.reach > 0, a.state == VEILED)        # (a candidate has 0 < t <= m: m > 0)
        assert np.array_equal(bits(a.reach[a.state == VEILED]), bits(m[a.state == VEILED])) and not bits(a.reach[a.state != VEILED]).any()
    if name in ("icosphere", "soup"):
        assert (h.hit != 0).sum() > 100


def test_a_skip_removes_one_candidate():
    mesh = U.rules_mesh()
    o, d, m, skip = U.rule_streams()["skip"]
    # 0 and 2 coincide under the first rays: with 0 alone opaque, skipping it leaves the translucent copy
    flags = np.array([1, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.uint8)
    a = any_np(mesh, o, d, m, skip, flags=flags)
    assert list(a.state[:4]) == [BLOCKED, VEILED, BLOCKED, BLOCKED]
    assert np.array_equal(a.state != 0, U.nearest_np(mesh, o, d, m, skip).hit != 0)


def test_the_flag_clamp_past_the_table():
    """surfaces 0 .. 9 on rules_mesh, 0 .. 299 on the soup: a table of 4 gives every surface >= 3 the flag of entry 3"""
    mesh = U.rules_mesh()
    assert list(A.opaque_of(mesh, np.array([0, 0, 0, 1], np.uint8))) == [False] * 3 + [True] * 7
    assert list(A.opaque_of(mesh, np.array([1, 1, 1, 0], np.uint8))) == [True] * 3 + [False] * 7
    assert A.opaque_of(mesh, np.array([0], np.uint8)).sum() == 0 and A.opaque_of(mesh, None).all()
    assert A.opaque_of(U.Mesh(mesh.V, mesh.tri), np.array([1, 0], np.uint8)).all()          # no surfaces: surface 0
    o, d, m, skip = U.rule_streams()["skip"]
    # the ray from z = 2 through triangle 4 (surface 4) and the square below (surfaces 0 .. 3)
    k = [11]
    for flags, want in (([0, 0, 0, 1], BLOCKED), ([1, 1, 1, 0], BLOCKED), ([0, 0, 0, 0], VEILED), ([0, 0, 0, 0, 0, 1], BLOCKED), ([0] * 10 + [1], VEILED),
                        ([0, 0, 0, 0, 1], BLOCKED)):
        a = any_np(mesh, o[:, k], d[:, k], m[k], skip[k], flags=np.array(flags, np.uint8))
        assert a.state[0] == want, (flags, a.state)
    soup = U.soup(257)
    so, sd, sm, ss = _streams(soup, 3)
    table = np.array([0, 0, 0, 1], np.uint8)
    wide = np.concatenate([table[:3], np.ones(297, np.uint8)])
    assert np.array_equal(any_np(soup, so, sd, sm, ss, flags=table).state, any_np(soup, so, sd, sm, ss, flags=wide).state)


def test_opaque_flags_of_an_opacity_table():
    one = F(1)
    t = np.array([[1, 1, 1, np.nan, 1, np.nextafter(one, F(2)), np.inf, 0, -1], [1, 1, np.nextafter(one, F(0)), 1, 1, 1, 1, 0, -1],
                  [1, 0.5, 1, 1, np.nan, 1, 1, 0, -1]], F)
    assert list(A.flags_np(t)) == [1, 0, 0, 0, 0, 0, 0, 0, 0]


def test_derived_planes_bit_for_bit():
    mesh = U.icosphere(1)
    o, d, m, skip = _streams(mesh, 5, 200)
    M = o.shape[1]
    flags = np.array([0], np.uint8)
    rng = np.random.default_rng(9)
    special = np.array([1.0, -0.0, 0.0, np.inf, -np.inf, np.nan, 0.25, -3.0, 1e-45], F)
    base = special[rng.integers(0, special.size, (3, M))]
    for fl in (None, flags):
        for b in (None, base):
            a = any_np(mesh, o, d, m, skip, flags=fl, base=b)
            bb = np.ones((3, M), F) if b is None else b
            blocked = a.state == BLOCKED
            assert blocked.sum() > 50 or fl is not None
            with np.errstate(all="ignore"):
                zero = (bb * F(0)).astype(F)
            assert np.array_equal(bits(a.visibility[:, blocked]), bits(zero[:, blocked]))
            assert np.array_equal(bits(a.visibility[:, ~blocked]), bits(bb[:, ~blocked]))
            if b is not None and blocked.any():                      # -0 and negatives give -0, inf and NaN give NaN: the walk's T * (1 - 1)
                v, k = a.visibility[:, blocked], bb[:, blocked]
                assert np.array_equal(np.isnan(v), ~np.isfinite(k)) and np.array_equal(np.signbit(v[np.isfinite(k)]), np.signbit(k[np.isfinite(k)]))
                with np.errstate(all="ignore"):
                    assert np.array_equal(bits(v), bits((k * (F(1) - F(1))).astype(F)))
            veiled = a.state == VEILED
            assert np.array_equal(bits(a.reach), bits(np.where(veiled, m, F(0)).astype(F)))
            assert a.written.all()
    # a permuted ray plane and planes wider than the rays: ids without an entry keep base and 0
    ray = rng.permutation(M + 40)[:M]
    wide = special[rng.integers(0, special.size, (3, M + 40))]
    a = any_np(mesh, o, d, m, skip, flags=flags, base=wide, ray=ray, ids=M + 40)
    s = any_np(mesh, o, d, m, skip, flags=flags)
    assert np.array_equal(a.state, s.state) and a.written.sum() == M
    assert np.array_equal(bits(a.visibility[:, ~a.written]), bits(wide[:, ~a.written])) and not bits(a.reach[~a.written]).any()
    assert np.array_equal(bits(a.reach[ray]), bits(s.reach))


@pytest.mark.parametrize("name", ["icosphere", "quad_grid"])
def test_statement_against_float64(name):
    mesh = U.icosphere(2) if name == "icosphere" else U.quad_grid(33)
    rng = np.random.default_rng(3)
    o, d = U.rays_at_targets(rng, U.interior_targets(rng, mesh, 1500), spread=2.0)
    o2, d2 = U.random_rays(rng, 1500)
    o, d = np.concatenate([o, o2], axis=1), np.concatenate([d, d2], axis=1)
    hit64, prim64, t64, margin = U.brute64(mesh, o, d)
    V = mesh.V.astype(np.float64)[mesh.tri[prim64].astype(np.int64)]
    n = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
    d64 = d.astype(np.float64).T
    cos = np.abs(np.einsum("kc,kc->k", n, d64)) / (np.linalg.norm(n, axis=1) * np.linalg.norm(d64, axis=1))
    keep = (margin >= 1e-3) & (~hit64 | (cos >= 0.25))
    assert keep.sum() >= 1500 and (keep & hit64).sum() >= 1000 and (keep & ~hit64).sum() >= 50
    a = any_np(mesh, o, d)
    assert np.array_equal(a.state[keep] != CLEAR, hit64[keep]) and not (a.state == VEILED).any()
    # a reach 1e-3 (relative) in front of the float64 nearest hit clears the ray, one behind it does not (the margin is in t)
    both = keep & hit64
    for scale, want in ((1 - 2e-3, False), (1 + 1e-4, True)):
        g = any_np(mesh, o[:, both], d[:, both], (t64[both] * scale).astype(F))
        assert ((g.state != CLEAR) == want).all()
