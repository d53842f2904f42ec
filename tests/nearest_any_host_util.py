"""builds and drives tests/native/nearest_any_host_check.cpp for test_nearest_any_host.py and test_gpu_nearest_any.py: a stand-alone
host program (g++, -ffp-contract=off, no HIP), plain or under the address and undefined-behaviour sanitizers.  A mesh with its
surfaces and a flag table, and a ray stream, go in as raw little-endian files; the program's brute force over the statement, the
library's traversal and the work both traversals did come back as arrays.  pytest does not collect this module."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np

from nearest_host_check_util import write_rays

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "native" / "nearest_any_host_check.cpp"
FLAGS = ["-std=c++14", "-Wall", "-Werror", "-ffp-contract=off", "-pthread"]


def build(directory, sanitize=False):
    exe = Path(directory) / ("nearest_any_host_check_san" if sanitize else "nearest_any_host_check")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    p = subprocess.run(["g++", *FLAGS, *extra, str(SOURCE), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return exe


def write_mesh(path, mesh, flags=None):
    """int64 nv, nt, surfaces, flags; float32 V; uint32 T; uint32 surface [nt] where the mesh has one; uint8 flags"""
    flags = np.zeros(0, np.uint8) if flags is None else np.ascontiguousarray(flags, np.uint8)
    with open(path, "wb") as f:
        f.write(np.array([mesh.V.shape[0], mesh.nt, 0 if mesh.surface is None else 1, flags.size], "<i8").tobytes())
        f.write(np.ascontiguousarray(mesh.V, "<f4").tobytes())
        f.write(np.ascontiguousarray(mesh.tri, "<u4").tobytes())
        if mesh.surface is not None:
            f.write(np.ascontiguousarray(mesh.surface, "<u4").tobytes())
        f.write(flags.tobytes())
    return Path(path)


_runs = [0]
NAMES = ("nt", "leaf", "depth", "nodes", "rays", "clear", "blocked", "veiled", "differ", "any_nodes", "any_tris", "nearest_nodes",
         "nearest_tris", "max_stack")
LINE = re.compile("ok any: " + " ".join(rf"{k} (\d+)" for k in NAMES))


def run(exe, mesh_path, o, d, m=None, skip=None, leaf=4):
    """-> state uint8 [M]: the program's brute force; tree_state: the traversal; ray_any_nodes, ray_any_tris, ray_nearest_nodes,
    ray_nearest_tris, ray_max_stack [M]; and the fields of its last line"""
    mesh_path = Path(mesh_path)
    _runs[0] += 1
    rays, out = mesh_path.with_name(f"arays{_runs[0]}.bin"), mesh_path.with_name(f"aout{_runs[0]}.bin")
    write_rays(rays, o, d, m, skip)
    p = subprocess.run([str(exe), str(mesh_path), str(rays), str(out), str(leaf)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    M = d.shape[1]
    w = np.fromfile(out, "<u4").reshape(M, 7)
    rays.unlink()
    out.unlink()
    head = LINE.fullmatch(p.stdout.splitlines()[-1])
    assert head, p.stdout
    r = SimpleNamespace(**{k: int(v) for k, v in zip(NAMES, head.groups())})
    r.state, r.tree_state = w[:, 0].astype(np.uint8), w[:, 1].astype(np.uint8)
    r.ray_any_nodes, r.ray_any_tris, r.ray_nearest_nodes, r.ray_nearest_tris, r.ray_max_stack = (w[:, k].astype(np.int64) for k in range(2, 7))
    assert r.rays == M and r.leaf == leaf and r.differ == 0 and np.array_equal(r.state, r.tree_state)
    assert (r.clear, r.blocked, r.veiled) == tuple(int((r.state == s).sum()) for s in (0, 1, 2))
    return r
