"""builds and drives tests/native/nearest_group_host_check.cpp for test_nearest_group_host.py, test_gpu_nearest_group_edges.py and
test_gpu_nearest_group_update_edges.py: a stand-alone host program (g++, -ffp-contract=off, no HIP), plain or under the address and
undefined-behaviour sanitizers.  A group (nearest_group_util.Inst's over shared meshes) and a ray stream go in as raw
little-endian files; the program's brute force and the library's two-level traversal come back as arrays.  pytest does not
collect this module."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "native" / "nearest_group_host_check.cpp"
FLAGS = ["-std=c++14", "-Wall", "-Werror", "-ffp-contract=off", "-pthread"]
NO_PRIM = NO_INSTANCE = 0xFFFFFFFF


def build(directory, sanitize=False):
    exe = Path(directory) / ("nearest_group_host_check_san" if sanitize else "nearest_group_host_check")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    p = subprocess.run(["g++", *FLAGS, *extra, str(SOURCE), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return exe


def write_group(path, insts):
    """the distinct meshes (by identity) once each, then the instances"""
    meshes, index = [], {}
    for i in insts:
        if id(i.mesh) not in index:
            index[id(i.mesh)] = len(meshes)
            meshes.append(i.mesh)
    with open(path, "wb") as f:
        f.write(np.array([len(meshes), len(insts)], "<i8").tobytes())
        for m in meshes:
            f.write(np.array([m.V.shape[0], m.nt], "<i8").tobytes())
            f.write(np.ascontiguousarray(m.V, "<f4").tobytes())
            f.write(np.ascontiguousarray(m.tri, "<u4").tobytes())
        for i in insts:
            f.write(np.array([index[id(i.mesh)]], "<u4").tobytes())
            f.write(np.ascontiguousarray(i.A, "<f4").tobytes() + np.ascontiguousarray(i.B, "<f4").tobytes())
    return Path(path)


_runs = [0]
LINE = re.compile(r"ok group: instances (\d+) parked (\d+) top_leaf (\d+) scene_leaf (\d+) depth (\d+) top_nodes (\d+) rays (\d+) hits (\d+) "
                  r"differ (\d+) max_top (\d+) max_stack (\d+)")


def run(exe, group_path, o, d, m=None, skip=None, top_leaf=2, scene_leaf=4):
    """-> instance, prim uint32 [M] (NO_INSTANCE / NO_PRIM: no hit), t float32 [M]: the program's brute force; tree_instance,
    tree_prim, tree_t: the traversal; ray_top_nodes, entered, ray_max_top, ray_max_stack [M]; levels: the top tree's node counts,
    the root's level first; and the fields of its last line"""
    group_path = Path(group_path)
    _runs[0] += 1
    rays, out = group_path.with_name(f"grays{_runs[0]}.bin"), group_path.with_name(f"gout{_runs[0]}.bin")
    M = d.shape[1]
    rec = np.empty((M, 9), "<u4")
    rec[:, 0:3], rec[:, 3:6] = np.asarray(o, "<f4").T.copy().view("<u4"), np.asarray(d, "<f4").T.copy().view("<u4")
    rec[:, 6] = (np.full(M, np.inf, "<f4") if m is None else np.ascontiguousarray(m, "<f4")).view("<u4")
    rec[:, 7] = NO_INSTANCE if skip is None else np.asarray(skip[0]).astype(np.int64) & 0xFFFFFFFF
    rec[:, 8] = NO_PRIM if skip is None else np.asarray(skip[1]).astype(np.int64) & 0xFFFFFFFF
    with open(rays, "wb") as f:
        f.write(np.array([M], "<i8").tobytes())
        f.write(rec.tobytes())
    p = subprocess.run([str(exe), str(group_path), str(rays), str(out), str(top_leaf), str(scene_leaf)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    w = np.fromfile(out, "<u4").reshape(M, 10)
    rays.unlink()
    out.unlink()
    head = LINE.fullmatch(p.stdout.splitlines()[-1])
    assert head, p.stdout
    names = ("instances", "parked", "top_leaf", "scene_leaf", "depth", "top_nodes", "rays", "hits", "differ", "max_top", "max_stack")
    r = SimpleNamespace(**{k: int(v) for k, v in zip(names, head.groups())})
    levels = p.stdout.splitlines()[-2].split()
    assert levels[0] == "levels:", p.stdout
    r.levels = [int(v) for v in levels[1:]]                          # the top tree's nodes level by level, the root's first
    r.instance, r.prim, r.t = w[:, 0].copy(), w[:, 1].copy(), w[:, 2].copy().view("<f4")
    r.tree_instance, r.tree_prim, r.tree_t = w[:, 3].copy(), w[:, 4].copy(), w[:, 5].copy().view("<f4")
    r.ray_top_nodes, r.entered, r.ray_max_top, r.ray_max_stack = (w[:, k].astype(np.int64) for k in (6, 7, 8, 9))
    r.hit = r.instance != NO_INSTANCE
    assert r.rays == M and r.hits == int(r.hit.sum()) and r.top_leaf == top_leaf and r.scene_leaf == scene_leaf
    return r
