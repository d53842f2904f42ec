"""helpers of the refit library's tests (test_nearest_refit_*.py, test_gpu_nearest_refit*.py): what
include/rlshaders_amd_nearest_refit.h declares and librls_nearest_refit.so exports, valid arguments over dummy memory for the
refusal table, the build and the pair files of tests/native/nearest_refit_host_check.cpp, the moved meshes, and the numpy
bottom-up union a read tree is held to (node by node, and a frontier a level for trees of millions of nodes).  pytest does not
collect this module."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import nearest_util as U
from nearest_abi_util import SCENE_HEADER, MovingWorld, exported_symbols, header_abi, scene_layout_tag  # noqa: F401
from nearest_util import F
from trace_abi_util import ROOT

HEADER = ROOT / "include" / "rlshaders_amd_nearest_refit.h"
SOURCE = ROOT / "tests" / "native" / "nearest_refit_host_check.cpp"
FLAGS = ["-std=c++14", "-Wall", "-Werror", "-ffp-contract=off", "-pthread"]
COUNT_MASK = 0xFF


@pytest.fixture(scope="module")
def refit_lib():
    from rlshaders_amd import build
    return build.build_nearest_refit_library()


# ---- the header, the dummy-memory world (nearest_abi_util.py) ----------------------------------------------------------------------
declared_symbols, declarations, structs, struct_members = header_abi(HEADER, "rls_nearest_refit_")


class RefitWorld(MovingWorld):
    NOUN = "refit"


# ---- the host check ------------------------------------------------------------------------------------------------------------------
def build(directory, sanitize=False):
    exe = Path(directory) / ("nearest_refit_host_check_san" if sanitize else "nearest_refit_host_check")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    p = subprocess.run(["g++", *FLAGS, *extra, str(SOURCE), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return exe


def write_pair(path, A, B, tri):
    """int64 nv, nt; float32 A[nv * 3]; float32 B[nv * 3]; uint32 T[nt * 3]"""
    A, B, tri = np.ascontiguousarray(A, "<f4"), np.ascontiguousarray(B, "<f4"), np.ascontiguousarray(tri, "<u4")
    assert A.shape == B.shape
    with open(path, "wb") as f:
        f.write(np.array([A.shape[0], tri.shape[0]], "<i8").tobytes())
        f.write(A.tobytes() + B.tobytes() + tri.tobytes())
    return Path(path)


PAIR_LINE = re.compile(r"ok pair: nt (\d+) leaf (\d+) depth (\d+) nodes (\d+) parked (\d+) rays (\d+) hits (\d+) differ (\d+) "
                       r"refit ([\d.]+) nodes ([\d.]+) triangles a ray rebuilt ([\d.]+) nodes ([\d.]+) triangles a ray")


def run_pair(exe, path, rays, leaf):
    p = subprocess.run([str(exe), str(path), str(rays), str(leaf)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    m = PAIR_LINE.fullmatch(p.stdout.strip().splitlines()[-1])
    assert m, p.stdout
    keys = ("nt", "leaf", "depth", "nodes", "parked", "rays", "hits", "differ")
    out = {k: int(v) for k, v in zip(keys, m.groups())}
    out.update(refit_nodes=float(m.group(9)), refit_tris=float(m.group(10)), rebuilt_nodes=float(m.group(11)), rebuilt_tris=float(m.group(12)))
    return out


def run_tree(exe, path, leaf):
    """the program's tree mode over a pair file: the tree the product's builder makes on A, which is the tree a scene on A
    holds -> (boxes float32 [nodes, 6], links uint32 [nodes, 2], prims uint32 [nt]), what Refit.read_tree returns"""
    path = Path(path)
    out = path.with_name(f"{path.stem}.tree{leaf}.bin")
    p = subprocess.run([str(exe), "tree", str(path), str(leaf), str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    raw = out.read_bytes()
    out.unlink()
    nodes, nt = (int(x) for x in np.frombuffer(raw, "<i8", 2))
    links = np.frombuffer(raw, "<u4", 2 * nodes, 16).reshape(nodes, 2).copy()
    prims = np.frombuffer(raw, "<u4", nt, 16 + 8 * nodes).copy()
    boxes = np.frombuffer(raw, "<f4", 6 * nodes, 16 + 8 * nodes + 4 * nt).reshape(nodes, 6).copy()
    assert len(raw) == 16 + 32 * nodes + 4 * nt
    return boxes, links, prims


# ---- moved meshes --------------------------------------------------------------------------------------------------------------------
def jittered(mesh, seed, amount=0.15):
    rng = np.random.default_rng(seed)
    return (mesh.V + rng.uniform(-amount, amount, mesh.V.shape)).astype(F)


def squashed(mesh, seed):
    """scaled per axis, sheared and moved: every triangle moves, most rays change their hit"""
    rng = np.random.default_rng(seed)
    V = mesh.V.astype(np.float64) * np.array([1.3, 0.55, 0.9])
    V[:, 0] += 0.35 * V[:, 1]
    return (V + np.array([0.21, -0.17, 0.12]) + rng.uniform(-0.02, 0.02, V.shape)).astype(F)


def twisted(V, radians):
    """about y, by `radians` end to end over the mesh's height"""
    V = np.asarray(V, np.float64)
    y = V[:, 1]
    a = radians * (y - y.min()) / max(float(np.ptp(y)), 1e-30)
    c, s = np.cos(a), np.sin(a)
    return np.stack([c * V[:, 0] + s * V[:, 2], y, -s * V[:, 0] + c * V[:, 2]], 1).astype(F)


def stacked():
    """-> (A, B, tri): the 4097-triangle soup, and every triangle of it stacked onto the three points of U.copies: every box is
    the same box and every hit ties, on a tree whose leaf order was made for another mesh"""
    a = U.soup(4097, seed=21)
    return a.V, np.tile(U.copies(1).V, (a.nt, 1)), a.tri             # (a soup triangle's vertices are its own: 3 i, 3 i + 1, 3 i + 2)


_POWERS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]
# The trees both launch plans of the update are held to (U.soup(nt) at leaf 1): nt -> the sizes of its levels, the root's first.
# The top of the tree -- the run of levels of at most 256 nodes that ends at the root -- is one launch of one workgroup unless
# RLS_NEAREST_REFIT_FOLD=0; every other level is a launch of its own.  1: one level, no fold either way; 2: the smallest fold;
# 256: a full 256-lane level in the top kernel; 257: all folded, and without the fold the level kernel's only level of exactly
# 256 nodes above a level of 2; 513, 1025: a deepest level of 2 nodes under a wide one; 640, 641: a deepest level of one full
# tile, and of one tile and two lanes, launched wide under both plans.
PLAN_TREES = {1: [1], 2: [1, 2], 256: _POWERS[:9], 257: _POWERS[:9] + [2], 513: _POWERS[:10] + [2], 640: _POWERS[:10] + [256],
              641: _POWERS[:10] + [258], 1025: _POWERS + [2]}
PLAN_GRIDS = {4: _POWERS[:10] + [260], 8: _POWERS[:9] + [260]}       # U.quad_grid(33) at leaf 4 and 8


def profile_np(links):
    """the sizes of a tree's levels, the root's first"""
    return np.bincount(levels_np(links))[1:].tolist()


def moved(mesh, V):
    return U.Mesh(V, mesh.tri, surface=mesh.surface, normals=mesh.normals)


def without(mesh, V, gone):
    """the mesh on V with the triangles `gone` (a bool mask) made degenerate at the origin: they never hit, ids stay"""
    V = np.concatenate([np.asarray(V, F), np.zeros((1, 3), F)])
    tri = mesh.tri.copy()
    tri[gone] = V.shape[0] - 1
    V = np.where(np.isfinite(V), V, F(0))
    normals = None if mesh.normals is None else np.concatenate([mesh.normals, np.zeros((1, 3), F)])
    return U.Mesh(V, tri, surface=mesh.surface, normals=normals)


def levels_np(links):
    """the level of every node (the root: 1) from the links; a child's index is past its parent's"""
    level = np.zeros(links.shape[0], np.int64)
    if links.shape[0]:
        level[0] = 1
    inner = np.flatnonzero((links[:, 1] & COUNT_MASK) == 0)
    for n in inner:
        level[links[n, 0]] = level[links[n, 0] + 1] = level[n] + 1
    return level


def levels_fast(links):
    """levels_np by a frontier expanded once per level: as many numpy steps as the tree has levels"""
    level = np.zeros(links.shape[0], np.int64)
    frontier = np.zeros(min(links.shape[0], 1), np.int64)
    l = 0
    while frontier.size:
        l += 1
        assert l <= 64 and (level[frontier] == 0).all()
        level[frontier] = l
        first = links[frontier[(links[frontier, 1] & COUNT_MASK) == 0], 0].astype(np.int64)
        frontier = np.concatenate([first, first + 1])
    return level


def union_np(boxes, links, prims, V, tri, levels=levels_np):
    """the bottom-up union over a read tree: a leaf from its triangles' vertices (a triangle with a non-finite coordinate: the
    origin), an inner node from its children, level by level -> boxes [nodes, 6]"""
    V, tri = np.asarray(V, F), np.asarray(tri).astype(np.int64)
    nodes = links.shape[0]
    want = np.zeros((nodes, 6), F)
    if nodes == 0:
        return want
    P = V[tri[prims.astype(np.int64)]]                               # [nt, 3, 3] in leaf order
    P = np.where(np.isfinite(P).all(axis=(1, 2))[:, None, None], P, F(0))
    lo, hi = P.min(axis=1), P.max(axis=1)
    count = (links[:, 1] & COUNT_MASK).astype(np.int64)
    leaves = np.flatnonzero(count)
    leaves = leaves[np.argsort(links[leaves, 0], kind="stable")]
    first = links[leaves, 0].astype(np.int64)
    assert first[0] == 0 and np.array_equal(first[1:], (first + count[leaves])[:-1]) and first[-1] + count[leaves[-1]] == len(prims)
    want[leaves, :3], want[leaves, 3:] = np.minimum.reduceat(lo, first), np.maximum.reduceat(hi, first)
    level = levels(links)
    assert (level > 0).all()
    for l in range(int(level.max()), 0, -1):
        n = np.flatnonzero((level == l) & (count == 0))
        a, b = links[n, 0].astype(np.int64), links[n, 0].astype(np.int64) + 1
        want[n, :3], want[n, 3:] = np.minimum(want[a, :3], want[b, :3]), np.maximum(want[a, 3:], want[b, 3:])
    return want


def union_fast(boxes, links, prims, V, tri):
    """union_np over levels_fast: for trees of millions of nodes"""
    return union_np(boxes, links, prims, V, tri, levels=levels_fast)
