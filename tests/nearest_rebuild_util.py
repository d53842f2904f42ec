"""helpers of the rebuild library's tests (test_nearest_rebuild_*.py, test_cmake_nearest_rebuild.py, test_gpu_nearest_rebuild*.py):
what include/rlshaders_amd_nearest_rebuild.h declares and librls_nearest_rebuild.so exports, valid arguments over dummy memory for
the refusal table, the build and the runs of tests/native/nearest_rebuild_host_check.cpp, and the meshes of exactly nt triangles
both the CPU and the GPU tests rebuild.  pytest does not collect this module."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import nearest_util as U
from nearest_abi_util import MovingWorld, exported_symbols, header_abi, scene_layout_tag  # noqa: F401
from nearest_util import F
from nearest_refit_util import run_tree, write_pair  # noqa: F401
from trace_abi_util import ROOT

HEADER = ROOT / "include" / "rlshaders_amd_nearest_rebuild.h"
SOURCE = ROOT / "tests" / "native" / "nearest_rebuild_host_check.cpp"
FLAGS = ["-std=c++14", "-Wall", "-Werror", "-ffp-contract=off"]
TILE = 256                                                          # kRebuildTile: the sort's and the scan's tile
SIZES = (0, 1, "leaf", "leaf+1", "2leaf+1", 11, 1000, 4099)         # the triangle counts of the CPU check, a leaf size at a time
LEAVES = (1, 3, 4, 8)


def sizes(leaf):
    return sorted({dict(leaf=leaf, **{"leaf+1": leaf + 1, "2leaf+1": 2 * leaf + 1}).get(s, s) for s in SIZES})


@pytest.fixture(scope="module")
def rebuild_lib():
    from rlshaders_amd import build
    build.build_nearest_library()                                   # the module loads it first: its scenes are what this library reads
    return build.build_nearest_rebuild_library()


# ---- the header, the dummy-memory world (nearest_abi_util.py) ----------------------------------------------------------------------
declared_symbols, declarations, structs, struct_members = header_abi(HEADER, "rls_nearest_rebuild_")


class RebuildWorld(MovingWorld):
    NOUN = "rebuild"


# ---- the host check ------------------------------------------------------------------------------------------------------------------
def build(directory, sanitize=False):
    exe = Path(directory) / ("nearest_rebuild_host_check_san" if sanitize else "nearest_rebuild_host_check")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    p = subprocess.run(["g++", *FLAGS, *extra, str(SOURCE), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return exe


LINE = re.compile(r"ok rebuild: nt (\d+) leaf (\d+) depth (\d+) nodes (\d+) parked (\d+) axes (\d+) (\d+) (\d+)")


def run_check(exe, path, leaf, out=None):
    """-> the program's figures; with `out` the rebuilt tree too, as nearest_refit_util.run_tree returns one"""
    p = subprocess.run([str(exe), str(path), str(leaf)] + ([str(out)] if out else []), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    m = LINE.fullmatch(p.stdout.strip().splitlines()[-1])
    assert m, p.stdout
    v = [int(x) for x in m.groups()]
    return dict(nt=v[0], leaf=v[1], depth=v[2], nodes=v[3], parked=v[4], axes=v[5:])


def read_tree_file(path):
    raw = Path(path).read_bytes()
    nodes, nt = (int(x) for x in np.frombuffer(raw, "<i8", 2))
    links = np.frombuffer(raw, "<u4", 2 * nodes, 16).reshape(nodes, 2).copy()
    prims = np.frombuffer(raw, "<u4", nt, 16 + 8 * nodes).copy()
    boxes = np.frombuffer(raw, "<f4", 6 * nodes, 16 + 8 * nodes + 4 * nt).reshape(nodes, 6).copy()
    assert len(raw) == 16 + 32 * nodes + 4 * nt
    return boxes, links, prims


# ---- meshes of exactly nt triangles: (A, B, tri), the scene is made on A and rebuilt to B ------------------------------------------
def _soup(nt, seed):
    return U.soup(nt, seed=seed) if nt else U.Mesh(np.zeros((3, 3), F), np.zeros((0, 3), np.uint32))


def random_pair(nt):
    a, b = _soup(nt, 5), _soup(nt, 6)                               # (a soup's indices depend on nt alone)
    assert np.array_equal(a.tri, b.tri)
    return a.V, b.V, a.tri


def identical_pair(nt):
    """every triangle over the same three vertices, in A and (elsewhere) in B: every key ties and the order is the ids'"""
    b = U.copies(max(nt, 1))
    return (b.V[:, [2, 0, 1]] + F(0.5)).astype(F), b.V, b.tri[:nt]


def flat_grid(nt):
    """the first nt triangles of a flat grid in the plane z = 0 over [-1, 1]^2: negative coordinates, whole rows of equal keys,
    and zeros of both signs (z is +-0 by the sign of the height field's sine; x and y pass through 0)"""
    n = max(int(np.ceil(np.sqrt(max(nt, 1) / 2.0))), 2)
    n += n % 2                                                      # an even side: the grid's middle line stands at 0
    g = U.quad_grid(n, flat=True)
    assert g.nt >= nt
    return U.Mesh(g.V, g.tri[:nt], surface=g.surface[:nt])


def flat_pair(nt):
    g = flat_grid(nt)
    V = g.V.copy()
    assert nt < 8 or ((V == 0) & np.signbit(V)).any() and ((V == 0) & ~np.signbit(V)).any() and (V < 0).any()
    A = (V[:, [1, 2, 0]] * F(0.5) + F(0.25)).astype(F)              # another pose: the axes dealt round
    return A, V, g.tri


def huge_pair(nt):
    """B: a soup scaled so that coordinates reach +-3e38: a centroid sum lo + hi is +-inf for a fifth of the triangles at
    either end of every axis, and the extent of a node that holds such triangles alone is inf - inf = NaN"""
    a = _soup(nt, 5)
    rng = np.random.default_rng(31)
    B = np.clip(a.V.astype(np.float64) * 2.8e38, -3.3e38, 3.3e38).astype(F)
    small = rng.random(B.shape[0]) < 0.125                          # an eighth of the vertices stay small
    B[small] = a.V[small]
    assert np.isfinite(B).all()
    if nt >= 1000:
        P = B[a.tri.astype(np.int64)]
        with np.errstate(over="ignore"):
            ctr = P.min(axis=1) + P.max(axis=1)
        assert (ctr == np.inf).sum() > nt // 16 and (ctr == -np.inf).sum() > nt // 16
    return a.V, B, a.tri


def hostile_pair(nt, seed=9):
    """B: a soup with NaN, +inf or -inf in one coordinate of a quarter of the vertices"""
    a, b = _soup(nt, 5), _soup(nt, 7)
    rng = np.random.default_rng(seed)
    B = b.V.copy()
    bad = rng.permutation(B.shape[0])[:B.shape[0] // 4]
    B[bad, rng.integers(0, 3, bad.size)] = np.array([np.nan, np.inf, -np.inf], F)[rng.integers(0, 3, bad.size)]
    return a.V, B, a.tri


def subnormal_pair(nt):
    """B: a soup scaled by 2^-128: every non-zero coordinate is denormal, and so is every centroid sum lo + hi and every extent
    kmax - kmin.  An add or a subtract that flushed denormals would make every key tie and every extent zero: axis 0 everywhere,
    the order the ids' -- the tree of the identical mesh, not the builder's"""
    a, b = _soup(nt, 5), _soup(nt, 6)
    assert np.array_equal(a.tri, b.tri)
    B = (b.V.astype(np.float64) * 2.0 ** -128).astype(F)
    if nt >= 1000:
        assert (np.abs(B[B != 0]) < 1.1754944e-38).all() and (B != 0).mean() > 0.99
        P = B[a.tri.astype(np.int64)]
        ctr = P.min(axis=1) + P.max(axis=1)
        assert (np.abs(ctr) < 1.2e-38).all()
        for c in range(3):
            assert np.unique(ctr[:, c]).size > nt - 4, (c, np.unique(ctr[:, c]).size)
    return a.V, B, a.tri


PAIRS = dict(random=random_pair, identical=identical_pair, flat=flat_pair, huge=huge_pair, subnormal=subnormal_pair)


def parked_of(B, tri):
    return ~np.isfinite(np.asarray(B, F)[np.asarray(tri).astype(np.int64)]).all(axis=(1, 2)) if len(tri) else np.zeros(0, bool)


def same_tree(got, want):
    """links and prims exactly, boxes by value (a zero bound may differ in sign) -> None, or what differs"""
    (gb, gl, gp), (wb, wl, wp) = got, want
    if gl.shape != wl.shape or gp.shape != wp.shape:
        return f"sizes {gl.shape} {gp.shape} against {wl.shape} {wp.shape}"
    if not np.array_equal(gl, wl):
        n = int(np.flatnonzero((gl != wl).any(axis=1))[0])
        return f"{int((gl != wl).any(axis=1).sum())} nodes' links differ, the first at {n}: {gl[n]} against {wl[n]}"
    if not np.array_equal(gp, wp):
        k = int(np.flatnonzero(gp != wp)[0])
        return f"{int((gp != wp).sum())} records differ, the first at {k}: {gp[k]} against {wp[k]}"
    if not (gb == wb).all():
        n = int(np.flatnonzero((gb != wb).any(axis=1))[0])
        return f"{int((gb != wb).any(axis=1).sum())} boxes differ, the first at {n}: {gb[n]} against {wb[n]}"
    return None
