"""CPU: nearest.host_stats (rlshaders_amd/csrc_nearest/nearest_stats.cpp, the kernel's traversal source compiled for the host
over the library's own tree) -- what tools/trace_bench.py --closure nearest and tests/test_gpu_nearest_edges.py count nodes and
triangles with.  Its hits are the numpy statement's, for every leaf size; its counts are within what the tree allows: a ray that
misses the root box opens one node, no triangle and holds no stack entry, no ray opens more nodes than the tree has or more
triangles than the mesh or holds more than depth - 1 entries, a ray that opens an inner node holds at least one, and smaller
leaves mean more nodes and fewer triangles in all.  (Trees deep enough to fill the stack: test_nearest_deep.py.)"""
import numpy as np

import nearest_util as U
from nearest_util import F


def test_host_stats_hits_are_the_statements_and_counts_are_bounded():
    from rlshaders_amd import nearest
    mesh = U.soup(257)
    rng = np.random.default_rng(6)
    o, d = U.random_rays(rng, 400)
    o[:, :8], d[:, :8] = F([[9.0], [9.0], [9.0]]), F([[1.0], [1.0], [1.0]])      # away from everything
    first = U.nearest_np(mesh, o, d)
    skip = np.where((first.hit != 0) & (np.arange(400) % 3 == 0), first.prim, U.NO_PRIM).astype(np.uint32)
    m = rng.uniform(0.5, 3.0, 400).astype(F)
    h = U.nearest_np(mesh, o, d, m, skip)
    totals = {}
    for leaf in (1, 4, 8):
        r = nearest.host_stats(mesh.V, mesh.tri, o, d, maxdist=m, skip=skip, leaf_size=leaf, per_ray=True)
        st = np.array(r["per_ray"])
        assert r["rays"] == 400 and r["hits"] == int(h.hit.sum()) > 100
        assert np.array_equal(st[:, 0], h.hit) and np.array_equal(st[h.hit != 0, 1], h.prim[h.hit != 0])
        assert st.shape == (400, 5)                                  # hit, prim, nodes, triangles, max_stack
        assert (st[:8, 2] == 1).all() and (st[:8, 3] == 0).all() and (st[:8, 4] == 0).all()
        assert (st[:, 4] >= 0).all() and (st[:, 4] <= r["depth"] - 1).all() and r["depth"] - 1 <= U.STACK
        assert ((st[:, 4] >= 1) == (st[:, 2] > 1)).all()             # past the root: the root was inner and pushed a sibling
        assert r["max_stack"] == int(st[:, 4].max()) >= 3
        assert (st[:, 2] >= 1).all() and (st[:, 2] <= r["tree_nodes"]).all() and (st[:, 3] <= mesh.nt).all()
        assert r["nodes"] == int(st[:, 2].sum()) and r["triangles"] == int(st[:, 3].sum())
        assert r["depth"] <= int(np.ceil(np.log2(mesh.nt / leaf))) + 1
        totals[leaf] = (r["nodes"], r["triangles"])
    assert totals[1][0] > totals[4][0] > totals[8][0] and totals[1][1] < totals[4][1] < totals[8][1], totals
    empty = nearest.host_stats(np.zeros((3, 3), F), np.zeros((0, 3), np.uint32), o[:, :4], d[:, :4])
    assert (empty["rays"], empty["hits"], empty["nodes"], empty["triangles"], empty["tree_nodes"], empty["max_stack"]) == (4, 0, 0, 0, 0, 0)
