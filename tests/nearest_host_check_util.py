"""builds tests/native/nearest_host_check.cpp for test_nearest_bvh.py, test_nearest_host_traversal.py and the deep tests
(test_nearest_deep.py, test_gpu_nearest_deep.py): a stand-alone host program (g++, -ffp-contract=off, no HIP), plain or under the
address and undefined-behaviour sanitizers; and drives its file mode: a mesh and a ray stream written as raw little-endian files,
the program's brute force -- and, with a leaf size, the library's builder and traversal -- read back as arrays.  pytest does not
collect this module."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "native" / "nearest_host_check.cpp"
FLAGS = ["-std=c++14", "-Wall", "-Werror", "-ffp-contract=off", "-pthread"]
NO_PRIM = 0xFFFFFFFF


def build(directory, sanitize=False):
    exe = Path(directory) / ("nearest_host_check_san" if sanitize else "nearest_host_check")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    p = subprocess.run(["g++", *FLAGS, *extra, str(SOURCE), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return exe


def run(exe, *args):
    p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    return p.stdout.splitlines()


def write_mesh(path, mesh):
    """int64 nv, nt; float32 V[nv * 3]; uint32 T[nt * 3]"""
    with open(path, "wb") as f:
        f.write(np.array([mesh.V.shape[0], mesh.nt], "<i8").tobytes())
        f.write(np.ascontiguousarray(mesh.V, "<f4").tobytes())
        f.write(np.ascontiguousarray(mesh.tri, "<u4").tobytes())
    return Path(path)


def write_rays(path, o, d, m=None, skip=None):
    """int64 rays; 8 words a ray: o.xyz, d.xyz, maxdist (float32; None: +inf), skip (uint32; None: nothing)"""
    M = d.shape[1]
    rec = np.empty((M, 8), "<u4")
    rec[:, 0:3], rec[:, 3:6] = np.asarray(o, "<f4").T.copy().view("<u4"), np.asarray(d, "<f4").T.copy().view("<u4")
    rec[:, 6] = (np.full(M, np.inf, "<f4") if m is None else np.ascontiguousarray(m, "<f4")).view("<u4")
    rec[:, 7] = NO_PRIM if skip is None else np.asarray(skip).astype(np.int64) & 0xFFFFFFFF
    with open(path, "wb") as f:
        f.write(np.array([M], "<i8").tobytes())
        f.write(rec.tobytes())
    return Path(path)


_runs = [0]


def run_file(exe, mesh_path, o, d, m=None, skip=None, leaf=0):
    """The program's file mode over a mesh written by write_mesh -> prim uint32 [M] (NO_PRIM: no hit), t float32 [M], hit: the
    brute force over every triangle.  With leaf also tree_prim, tree_t, nodes, tris, max_stack [M] -- the library's traversal
    over the tree the library's builder made, whose invariants the program has checked -- and depth, tree_nodes, differ (the
    program's own count of rays whose traversal is not its brute force)."""
    mesh_path = Path(mesh_path)
    _runs[0] += 1
    rays, out = mesh_path.with_name(f"rays{_runs[0]}.bin"), mesh_path.with_name(f"out{_runs[0]}.bin")
    write_rays(rays, o, d, m, skip)
    lines = run(exe, "file", mesh_path, rays, out, *([leaf] if leaf else []))
    M = d.shape[1]
    w = np.fromfile(out, "<u4").reshape(M, 7 if leaf else 2)
    rays.unlink()
    out.unlink()
    r = SimpleNamespace(prim=w[:, 0].copy(), t=w[:, 1].copy().view("<f4"), lines=lines)
    r.hit = r.prim != NO_PRIM
    head = re.fullmatch(r"ok file: nt (\d+) leaf (\d+) depth (\d+) nodes (\d+) rays (\d+) hits (\d+) differ (\d+)", lines[-1])
    assert head and int(head.group(2)) == leaf and int(head.group(5)) == M and int(head.group(6)) == int(r.hit.sum()), lines
    r.nt = int(head.group(1))
    if leaf:
        r.tree_prim, r.tree_t = w[:, 2].copy(), w[:, 3].copy().view("<f4")
        r.nodes, r.tris, r.max_stack = w[:, 4].astype(np.int64), w[:, 5].astype(np.int64), w[:, 6].astype(np.int64)
        r.depth, r.tree_nodes, r.differ = int(head.group(3)), int(head.group(4)), int(head.group(7))
    return r


def mixed_stream(exe, mesh_path, mesh, M, seed):
    """test_gpu_nearest.mixed_rays for a mesh too large for nearest_np: random rays, half of them aimed at the mesh, the hostile
    rays, reaches about the scene's size, and for 0.3 of the rays that hit the triangle hit first skipped -- found by the
    program's brute force -> o, d, m, skip"""
    import nearest_util as U
    rng = np.random.default_rng(seed)
    ho, hd, hm, hs = U.hostile_rays(mesh, seed=seed)
    K = M - ho.shape[1]
    o, d = U.random_rays(rng, K)
    o[:, :K // 2], d[:, :K // 2] = U.rays_at_targets(rng, U.interior_targets(rng, mesh, K // 2, margin=0.0), spread=2.0)
    m = rng.uniform(0.3, 3.0, K).astype(np.float32)
    m[rng.random(K) < 0.3] = np.inf
    first = run_file(exe, mesh_path, o, d)
    skip = np.where(first.hit & (rng.random(K) < 0.3), first.prim, NO_PRIM).astype(np.uint32)
    return np.concatenate([o, ho], 1), np.concatenate([d, hd], 1), np.concatenate([m, hm]), np.concatenate([skip, hs])
