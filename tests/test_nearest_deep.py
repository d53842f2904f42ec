"""CPU: the tree and the traversal of librls_nearest.so at the depth their stack is sized for.  No mesh of the other nearest tests
has more than 2 178 triangles, a tree of 12 levels; here the stand-alone host program tests/native/nearest_host_check.cpp (its
file mode: a brute force over every triangle on a pool of threads, the library's builder and traversal beside it) runs

  - the 1025-triangle soup and the rules' mesh on the existing streams: its brute force = nearest_np bit for bit in (prim, t),
    rays without a hit included, and nearest_util.hits_at -- the candidate rule at one given triangle per ray -- reproduces every
    plane of nearest_np: the two restatements are tied to each other before either is the reference at scale;
  - mid_soup (2^17 + 1 triangles, 19 levels at leaf_size 1) at leaf_size 1, 2, 4, 8 on 4096 rays: traversal = brute force, the
    tree's invariants hold; once more under the address and undefined-behaviour sanitizers on 512 rays;
  - deep_grid (2^21 + 20 triangles) at leaf_size 1 and 8: 23 and 20 levels; on the 577 rays of nearest_util.deep_stream the
    traversal = the brute force; at least 30 % of the rays hit and at least 65 hold depth - 1 entries -- 22 at leaf_size 1, the
    largest the traversal has been seen to hold, stack words 0 .. 21 written (the documented worst case; RLS_NEAREST_STACK is
    24) --, asserted BEFORE anything is compared; the reversed corner rays hold at most 2; the vertical rays hit the triangle
    the cell index names;
  - two_sheets, the documented limit of 2^22 triangles itself, built once: invariants, 23 levels, depth - 1 <= 24, traversal =
    brute force on 64 rays with corner rays among them;
  - copies (4097 coincident triangles) at leaf_size 1, 4, 8: a ray through the interior opens EVERY node, nodes == node_count
    (8193, 2049, 1025) and tris == K -- the loop bound `visits < node_count` met with equality, where an off-by-one drops the last
    leaf --, and the tie goes to triangle 0, to 1 with 0 skipped, to 0 with K - 1 skipped;
  - huge_soup (coordinates up to 3e38, subnormal triangles: non-finite centroid keys in the builder) at every leaf size:
    traversal = brute force = nearest_np.
A wrong traversal cannot hang any of this: its loop is bounded by node_count."""
import numpy as np
import pytest

import nearest_util as U
from nearest_util import F, NO_PRIM
from nearest_host_check_util import build, mixed_stream, run_file, write_mesh

LEAVES = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("nearest_deep")


@pytest.fixture(scope="module")
def exe(work):
    return build(work)


_meshes = {}


def mesh_file(work, name):
    if name not in _meshes:
        mesh = U.DEEP_MESHES[name]() if name in U.DEEP_MESHES else dict(soup=U.soup, rules=U.rules_mesh)[name]()
        _meshes[name] = (mesh, write_mesh(work / f"{name}.bin", mesh))
    return _meshes[name]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_prim_t(r, prim, t, what):
    """two (prim, t) answers, NO_PRIM where there is no hit: the same triangles and, on the hits, the same bits of t"""
    assert np.array_equal(r[0], prim), (what, "prim", np.flatnonzero(r[0] != prim)[:8])
    hit = prim != NO_PRIM
    assert np.array_equal(bits(r[1])[hit], bits(t)[hit]), (what, "t", np.flatnonzero(hit & (bits(r[1]) != bits(t)))[:8])


def traversal_is_brute(r, what):
    same_prim_t((r.tree_prim, r.tree_t), r.prim, r.t, what)
    assert r.differ == 0, what
    assert (r.nodes >= 1).all() and (r.nodes <= r.tree_nodes).all() and (r.tris <= r.nt).all() and (r.max_stack <= r.depth - 1).all()


def same_planes(g, h, what):
    for name in ("hit", "prim", "surface", "t", "u", "v", "P", "N", "Ns", "T", "wo"):
        a, b = getattr(g, name), getattr(h, name)
        if a.dtype.kind == "f":
            ok = (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
        else:
            ok = a == b
        assert ok.all(), (what, name, np.argwhere(~ok)[:4].tolist())


def brute_is_nearest_np(mesh, r, o, d, m, skip, what):
    """the program's brute force = the numpy statement, and hits_at on the brute force's prim = every plane of it"""
    h = U.nearest_np(mesh, o, d, m, skip)
    same_prim_t((r.prim, r.t), np.where(h.hit != 0, h.prim, NO_PRIM).astype(np.uint32), h.t, what)
    same_planes(U.hits_at(mesh, o, d, r.prim, m, skip), h, what)
    return h


def test_file_mode_is_the_numpy_statement_on_the_existing_streams(exe, work):
    mesh, path = mesh_file(work, "soup")
    o, d, m, skip = mixed_stream(exe, path, mesh, 600, 13)
    h = brute_is_nearest_np(mesh, run_file(exe, path, o, d, m, skip), o, d, m, skip, "soup")
    assert 0.2 < h.hit.mean() < 0.95 and (skip != NO_PRIM).sum() > 50
    h = brute_is_nearest_np(mesh, run_file(exe, path, o, d), o, d, None, None, "soup, no reach, no skip")
    mesh, path = mesh_file(work, "rules")
    for name, (o, d, m, skip) in sorted(U.rule_streams().items()):
        r = run_file(exe, path, o, d, m, skip, leaf=1)
        brute_is_nearest_np(mesh, r, o, d, m, skip, name)
        traversal_is_brute(r, name)
    # hits_at at a triangle that is NOT a candidate reports no hit: every ray of the ties stream at the degenerate triangle 7
    o, d, m, skip = U.rule_streams()["ties"]
    assert not U.hits_at(mesh, o, d, np.full(d.shape[1], 7)).hit.any()


@pytest.fixture(scope="module")
def mid_stream(exe, work):
    mesh, path = mesh_file(work, "mid_soup")
    return mixed_stream(exe, path, mesh, 4096, 17)


@pytest.mark.parametrize("leaf", LEAVES)
def test_mid_soup_traversal_is_the_brute_force(exe, work, mid_stream, leaf):
    mesh, path = mesh_file(work, "mid_soup")
    o, d, m, skip = mid_stream
    r = run_file(exe, path, o, d, m, skip, leaf=leaf)
    assert r.nt == (1 << 17) + 1 and r.depth <= int(np.ceil(np.log2(r.nt / leaf))) + 1 and r.depth - 1 <= U.STACK
    assert leaf != 1 or r.depth == 19
    assert 0.3 < r.hit.mean() < 0.98 and (skip != NO_PRIM).sum() > 300
    traversal_is_brute(r, ("mid_soup", leaf))
    g = U.hits_at(mesh, o, d, r.prim, m, skip)
    assert np.array_equal(g.hit != 0, r.hit) and np.array_equal(bits(g.t)[r.hit], bits(r.t)[r.hit])
    print("mid_soup leaf", leaf, dict(depth=r.depth, nodes=r.tree_nodes, max_stack=int(r.max_stack.max())))


def test_mid_soup_under_sanitizers(work, mid_stream):
    san = build(work, sanitize=True)
    mesh, path = mesh_file(work, "mid_soup")
    o, d, m, skip = (x[..., -512:] for x in mid_stream)              # the hostile rays are the last 64
    r = run_file(san, path, o, d, m, skip, leaf=1)
    assert r.depth == 19 and r.hit.sum() > 100
    traversal_is_brute(r, "mid_soup under sanitizers")


@pytest.fixture(scope="module")
def deep(work):
    mesh, path = mesh_file(work, "deep_grid")
    return mesh, path, U.deep_stream(mesh)


@pytest.mark.parametrize("leaf, depth", [(1, 23), (8, 20)])
def test_deep_grid_fills_the_stack(exe, deep, leaf, depth):
    mesh, path, (o, d, m, skip, info) = deep
    assert d.shape[1] == 577 == 2 * 256 + 64 + 1
    r = run_file(exe, path, o, d, m, skip, leaf=leaf)
    # the caps first: a stream that stopped exercising the stack fails here, whatever it would compare to
    assert r.depth == depth and depth - 1 <= U.STACK
    assert r.hit.mean() >= 0.30, r.hit.mean()
    full = r.max_stack == depth - 1
    assert full.sum() >= 65 and r.max_stack.max() == depth - 1, (int(full.sum()), int(r.max_stack.max()))
    assert full[info["corner"]].all() and full[info["corner_wave"]].all() and full[info["corner_even"]].all()
    assert (r.max_stack[info["reversed"]] <= 2).all() and r.hit[info["reversed"]].all()
    print("deep_grid leaf", leaf, dict(depth=r.depth, nodes=r.tree_nodes, max_stack=int(r.max_stack.max()), full=int(full.sum()),
                                       hits=int(r.hit.sum())))
    traversal_is_brute(r, ("deep_grid", leaf))
    # the corner rays hit the corner triangle, the neighbours' rays their triangle out of a sibling pushed at a high index
    for k in ("corner", "corner_wave", "corner_even", "reversed"):
        assert (r.prim[info[k]] == 0).all(), k
    assert np.array_equal(r.prim[info["near_corner"]], np.arange(1, 25)) and (r.max_stack[info["near_corner"]] >= depth - 7).all()
    # anchors that depend on neither restatement: the triangle a cell index names, the extra triangle a ray was aimed through
    assert np.array_equal(r.prim[info["vertical"]], info["vertical_prim"])
    assert np.array_equal(r.prim[info["above"]], info["above_prim"])
    assert np.array_equal(mesh.surface[r.prim[info["above"]]], 1000 + np.arange(40) // 2)
    g = U.hits_at(mesh, o, d, r.prim, m, skip)
    assert np.array_equal(g.hit != 0, r.hit) and np.array_equal(bits(g.t)[r.hit], bits(r.t)[r.hit])
    if leaf == 1:                                                    # with `last` carried the rays from above go on to the grid
        below = run_file(exe, path, o, d, m, np.where(r.hit, r.prim, skip), leaf=leaf)
        traversal_is_brute(below, "deep_grid, second query")
        assert below.hit[info["above"]].all() and (below.prim[info["above"]] < (1 << 21)).all()
        assert not below.hit[info["vertical"]].any()


def test_the_triangle_limit_is_built_once(exe, work):
    """RLS_NEAREST_MAX_TRIANGLES = 2^22 triangles at leaf_size 1: the only place the documented limit itself is built.  About 5 s
    on the 8-core development machine: the mesh and its 75 MB file, one build, the invariants, 64 rays against 2^22 triangles."""
    mesh, path = mesh_file(work, "two_sheets")
    rng = np.random.default_rng(3)
    o, d = U.random_rays(rng, 64)
    third = np.full((1, 3), 1.0 / 3.0)
    o[:, 0:1], d[:, 0:1] = U.corner_rays(mesh, third)
    o[:, 1:2], d[:, 1:2] = U.corner_rays(mesh, third, reverse=True)
    o[:, 2:10], d[:, 2:10] = U.corner_rays(mesh, rng.dirichlet((1, 1, 1), 8) * 0.7 + 0.1, np.array(U.CORNER_D) + 0.01 * np.arange(8)[:, None])
    o[:, 10:12], d[:, 10:12] = U.corner_rays(mesh, np.tile(third, (2, 1)), tri=(1 << 21))      # the upper sheet's corner
    d[:, 11] = -d[:, 11]
    o[:, 11] = o[:, 10] - 2 * d[:, 11]                               # ... and the same point from above
    r = run_file(exe, path, o, d, leaf=1)
    assert r.nt == U.MAX_TRIANGLES == 1 << 22 and r.depth == 23 and r.depth - 1 <= U.STACK and r.tree_nodes == 2 * r.nt - 1
    assert r.hit.mean() >= 0.30 and (r.max_stack[[0, 2, 3, 4, 5, 6, 7, 8, 9]] == 22).all() and r.max_stack.max() == 22
    traversal_is_brute(r, "two sheets")
    assert (r.prim[[0, 2, 3, 4, 5, 6, 7, 8, 9]] == 0).all() and (r.prim[10:12] == (1 << 21)).all()
    assert r.prim[1] >= (1 << 21)                                    # the reversed ray comes from above: the upper sheet
    print("two sheets", dict(depth=r.depth, nodes=r.tree_nodes, max_stack=int(r.max_stack.max()), hits=int(r.hit.sum())))


@pytest.mark.parametrize("leaf, nodes", [(1, 8193), (4, 2049), (8, 1025)])
def test_copies_open_every_node(exe, work, leaf, nodes):
    mesh, path = mesh_file(work, "copies")
    K = mesh.nt
    o, d, m, skip = U.copies_rays(K)
    r = run_file(exe, path, o, d, m, skip, leaf=leaf)
    assert K == 4097 and r.tree_nodes == nodes
    # rays 0 .. 6 tie at every triangle: no node is culled (tn <= t), the loop runs node_count times and tests every copy
    assert (r.nodes[:7] == nodes).all() and (r.tris[:7] == K).all(), (r.nodes, r.tris)
    assert r.prim[:7].tolist() == [0, 1, 0, 0, 0, 0, 0] and r.tree_prim[:7].tolist() == [0, 1, 0, 0, 0, 0, 0]
    assert r.nodes[7] == nodes and r.tris[7] == K and not r.hit[7]   # the edge ray: every box open, no candidate
    assert not r.hit[8]
    traversal_is_brute(r, ("copies", leaf))
    brute_is_nearest_np(mesh, r, o, d, m, skip, ("copies", leaf))


@pytest.mark.parametrize("leaf", LEAVES)
def test_huge_and_subnormal_coordinates(exe, work, leaf):
    mesh, path = mesh_file(work, "huge_soup")
    o, d, m, skip = U.huge_rays(mesh)
    r = run_file(exe, path, o, d, m, skip, leaf=leaf)               # the build ends and its invariants hold
    assert r.depth <= int(np.ceil(np.log2(1025 / leaf))) + 1
    traversal_is_brute(r, ("huge_soup", leaf))
    h = brute_is_nearest_np(mesh, r, o, d, m, skip, ("huge_soup", leaf))
    assert h.hit.sum() > 60
