"""CPU: the any-hit traversal of librls_nearest_any.so -- rlshaders_amd/csrc_nearest/rls_nearest_any.hpp compiled for the host with
-ffp-contract=off by tests/native/nearest_any_host_check.cpp, over the product's builder.  For every ray any_traverse equals
any_brute (every triangle, no tree, no early end) in state -- the program refuses otherwise (differ == 0) -- at leaf sizes 1, 4
and 8, without a table, with every flag set, with none set and with mixed flags, with skipped triangles; and on the small meshes
this file holds that brute force to any_np (tests/nearest_any_util.py): the C++ restatement and the numpy one are one function.
The meshes: the icosphere, the soup with its degenerate triangles, the rules' mesh with its rule streams, the deep grid (2^21 + 20
triangles, 23 levels at leaf 1) with its stack-filling stream, and the two sheets at the triangle limit; the hostile rays (NaN /
inf / zero directions, NaN reach) are in every stream.  The nodes and triangles any_traverse and nearest_traverse visit on the
same rays are printed for the record.  The same program runs once more under the address and undefined-behaviour sanitizers, on
the small meshes; nothing is loaded into Python."""
import numpy as np
import pytest

import nearest_any_host_util as H
import nearest_util as U
from nearest_any_util import BLOCKED, CLEAR, VEILED, any_np
from nearest_util import F, NO_PRIM


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("any_host")
    return d, H.build(d), H.build(d, sanitize=True)


def stream(mesh, K, seed):
    """random rays, half of them aimed at the mesh, finite reaches for most, and the hostile rays"""
    rng = np.random.default_rng(seed)
    o, d = U.random_rays(rng, K)
    o[:, :K // 2], d[:, :K // 2] = U.rays_at_targets(rng, U.interior_targets(rng, mesh, K // 2, margin=0.0), spread=2.0)
    m = rng.uniform(0.3, 3.0, K).astype(F)
    m[rng.random(K) < 0.3] = np.inf
    ho, hd, hm, hs = U.hostile_rays(mesh, seed=seed)
    return np.concatenate([o, ho], 1), np.concatenate([d, hd], 1), np.concatenate([m, hm]), np.concatenate([np.full(K, NO_PRIM, np.uint32), hs])


def tables(rng):
    return {"none": None, "all": np.ones(4, np.uint8), "mixed": np.array([1, 0, 0, 1], np.uint8), "clear": np.zeros(5, np.uint8),
            "wide": rng.integers(0, 2, 320).astype(np.uint8)}


def record(name, r):
    print(f"visits {name}: leaf {r.leaf} rays {r.rays} blocked {r.blocked} veiled {r.veiled} per ray: any nodes {r.any_nodes / max(r.rays, 1):.1f} "
          f"tris {r.any_tris / max(r.rays, 1):.1f}, nearest nodes {r.nearest_nodes / max(r.rays, 1):.1f} tris {r.nearest_tris / max(r.rays, 1):.1f}")


SMALL = {"icosphere": lambda: U.icosphere(2), "soup": lambda: U.soup(1025), "rules": U.rules_mesh}


@pytest.mark.parametrize("name", list(SMALL))
def test_any_traverse_equals_the_brute_force_and_numpy(programs, name):
    d, plain, san = programs
    mesh = SMALL[name]()
    o, dd, m, skip = stream(mesh, 1200, seed=len(name))
    if name == "rules":
        extra = list(U.rule_streams().values())
        o, dd = np.concatenate([o] + [e[0] for e in extra], 1), np.concatenate([dd] + [e[1] for e in extra], 1)
        m, skip = np.concatenate([m] + [e[2] for e in extra]), np.concatenate([skip] + [e[3] for e in extra])
    first = U.nearest_np(mesh, o, dd, m, skip)
    rng = np.random.default_rng(2)
    skip2 = np.where((first.hit != 0) & (rng.random(o.shape[1]) < 0.5), first.prim, skip).astype(np.uint32)
    for tname, flags in tables(rng).items():
        path = H.write_mesh(d / f"{name}_{tname}.bin", mesh, flags)
        for sk in (skip, skip2):
            want = any_np(mesh, o, dd, m, sk, flags=flags).state
            for leaf in (1, 4, 8):
                r = H.run(plain, path, o, dd, m, sk, leaf=leaf)
                assert np.array_equal(r.state, want), (tname, leaf)
                assert (r.ray_any_nodes <= max(r.nodes, 1)).all() and r.max_stack <= max(r.depth - 1, 0)
                if flags is None or flags.all():                     # nothing to go on for: never more work than the nearest hit
                    assert (r.ray_any_nodes <= r.ray_nearest_nodes).all() and (r.ray_any_tris <= r.ray_nearest_tris).all()
            if sk is skip:
                record(f"{name} {tname}", r)
        if name != "rules":
            assert (want == CLEAR).sum() > 100 and ((want != CLEAR).sum() > 100)
        if tname == "mixed" and name != "icosphere":                 # (the icosphere is one surface)
            assert (want == BLOCKED).any() and (want == VEILED).any()
        # the sanitized program: fewer rays, the hostile ones among them
        keep = np.r_[0:200, o.shape[1] - 100:o.shape[1]]
        r = H.run(san, path, o[:, keep], dd[:, keep], m[keep], skip2[keep], leaf=4)
        assert np.array_equal(r.state, any_np(mesh, o[:, keep], dd[:, keep], m[keep], skip2[keep], flags=flags).state)
    # a mesh without surfaces: every triangle is surface 0
    bare = U.Mesh(mesh.V, mesh.tri)
    path = H.write_mesh(d / f"{name}_bare.bin", bare, np.array([0, 1], np.uint8))
    r = H.run(plain, path, o, dd, m, skip, leaf=4)
    assert not (r.state == BLOCKED).any() and np.array_equal(r.state != CLEAR, first.hit != 0)


def test_the_empty_mesh(programs):
    d, plain, san = programs
    mesh = U.empty_mesh()
    o, dd, m, skip = stream(U.icosphere(0), 100, 3)
    for exe in (plain, san):
        r = H.run(exe, H.write_mesh(d / "empty.bin", mesh, np.array([1], np.uint8)), o, dd, m, skip, leaf=1)
        assert r.nodes == 0 and not r.state.any()


def test_the_deep_grid_and_its_stack_filling_stream(programs):
    d, plain, _ = programs
    mesh = U.deep_grid()
    o, dd, m, skip, info = U.deep_stream(mesh)
    # surfaces 0 .. 4 on the grid, 1000 .. 1019 on the extra triangles above it: the table's last entry is theirs
    for tname, flags in (("none", None), ("veil_above", np.array([1, 1, 0, 1, 1, 0], np.uint8)), ("veil_grid", np.array([0, 0, 0, 0, 0, 1], np.uint8))):
        path = H.write_mesh(d / f"deep_{tname}.bin", mesh, flags)
        by_leaf = {}
        for leaf in (1, 8) if tname == "none" else (1,):
            r = by_leaf[leaf] = H.run(plain, path, o, dd, m, skip, leaf=leaf)
            assert r.depth == (23 if leaf == 1 else 20)
            record(f"deep_grid {tname}", r)
        assert all(np.array_equal(by_leaf[1].state, b.state) for b in by_leaf.values())
        r = by_leaf[1]
        # a corner ray holds the sibling of every level on its way down, as it does for the nearest hit
        assert r.ray_max_stack[info["corner"][0]] == r.depth - 1 == 22 and r.max_stack == 22
        above = info["above"]
        if tname == "none":
            assert (r.state[above] == BLOCKED).all() and not (r.state == VEILED).any()
            assert (r.state[info["vertical"]] == BLOCKED).all()
        elif tname == "veil_above":                                  # through an extra triangle (translucent), then the grid below
            grid_flag = flags[np.minimum(mesh.surface[:1 << 21], 5)]
            assert (r.state[above] != CLEAR).all() and (r.state[above] == VEILED).any() and (r.state[above] == BLOCKED).any()
            want = np.where(grid_flag[info["vertical_prim"]] != 0, BLOCKED, VEILED)
            assert np.array_equal(r.state[info["vertical"]], want)
        else:
            assert (r.state[above] == BLOCKED).all() and (r.state[info["vertical"]] == VEILED).all()


def test_two_sheets_at_the_triangle_limit(programs):
    d, plain, _ = programs
    mesh = U.two_sheets()
    o, dd, m, skip, info = U.deep_stream(U.deep_grid())
    keep = np.r_[0:1, 64:96, 128:144, 256:288, 320:384, 384:416]
    o, dd, m, skip = o[:, keep], dd[:, keep], m[keep], skip[keep]
    # the lower sheet's surfaces 0 .. 4 translucent, the upper one's 5 .. 9 opaque
    path = H.write_mesh(d / "two_sheets.bin", mesh, np.array([0, 0, 0, 0, 0, 1], np.uint8))
    r = H.run(plain, path, o, dd, m, skip, leaf=1)
    assert r.nt == U.MAX_TRIANGLES and r.depth == 23
    record("two_sheets", r)
    vertical = slice(49, 81)                                         # from z = 0.5 down: the upper sheet is at or behind the origin
    assert (r.state[vertical] != CLEAR).all()
    assert (r.state == BLOCKED).any() and (r.state == VEILED).any() and (r.state == CLEAR).any()
