"""Nearest-hit queries over a triangle mesh on the device (include/rlshaders_amd_nearest.h, companion library
``librls_nearest.so``): the query every queue of ``trace`` and both walks ask the renderer for, answered through a BVH, so that
a path from an emit to its resolve stays on the device.

    scene = nearest.Scene(ctx, vertices, triangles, surface=ids, normals=vertex_normals)   # host arrays; the tree is built here
    walk.run(probes, P, nearest.tracer(scene))                                 # rlSss probes walked through the mesh
    shadow_walk.run(q, P, nearest.tracer(scene, opacity=table))                # shadow rays: surface indexes the opacity table
    f = scene.hits(nearest.Rays(P, q.dir, via=q.point), bin_of_surface=bins)   # a glossy queue's rays, no maxdist
    routes = trace.route_hits(ctx, f.bins(), n_bins)                           # ... routed by the node bin of the surface hit
    hitP, hitN = routes.gather(b, f.P, f.N)                                    # ... and gathered from the found planes

The result of a query is a function of the mesh and the ray alone (the header's statement; tests/nearest_util.py restates it in
numpy): the tree, its leaf size and the math mode of the context do not change a bit of it.  ``hits`` does not synchronise.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _capi as capi
from . import shadow_walk, trace, walk
from ._capi import check
from .walk import _IDS, WalkRays_, _flat, _rows, rays_struct

NEAREST_LIB_PATH = capi._PKG / "lib" / "librls_nearest.so"

RLS_NEAREST_STACK = 24
RLS_NEAREST_MAX_TRIANGLES = 1 << 22
RLS_NEAREST_MAX_LEAF = 8
RLS_NEAREST_DEFAULT_LEAF = 4
RLS_NEAREST_NO_PRIM = 0xFFFFFFFF


class NearestMesh_(C.Structure):
    """rls_nearest_mesh"""
    _fields_ = [("nv", C.c_int64), ("nt", C.c_int64), ("vertices", C.c_void_p), ("triangles", C.c_void_p), ("surface", C.c_void_p),
                ("normals", C.c_void_p), ("leaf_size", C.c_int)]


class NearestSceneInfo_(C.Structure):
    """rls_nearest_scene_info"""
    _fields_ = [("nv", C.c_int64), ("nt", C.c_int64), ("nodes", C.c_int64), ("leaf_size", C.c_int), ("depth", C.c_int),
                ("device_bytes", C.c_size_t)]


class NearestRays_(C.Structure):
    """rls_nearest_rays"""
    _fields_ = [("rays", C.c_int64), ("count", C.c_void_p), ("origin", capi.CVec3), ("via", C.c_void_p), ("dir", capi.CVec3),
                ("maxdist", C.c_void_p), ("ray", C.c_void_p)]


class NearestFound_(C.Structure):
    """rls_nearest_found"""
    _fields_ = [("hit", C.c_void_p), ("t", C.c_void_p), ("P", capi.Vec3), ("N", capi.Vec3), ("Ns", capi.Vec3), ("T", capi.Vec3),
                ("wo", capi.Vec3), ("prim", C.c_void_p), ("surface", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p),
                ("bin", C.c_void_p), ("bin_of_surface", C.c_void_p), ("bin_count", C.c_uint32), ("last", C.c_void_p)]


_ctx, _i64, _vp = C.c_void_p, C.c_int64, C.c_void_p
PROTOTYPES = {
    "rls_nearest_scene_create": (C.c_int, [_ctx, C.POINTER(NearestMesh_), C.POINTER(_vp)]),
    "rls_nearest_scene_destroy": (C.c_int, [_vp]),
    "rls_nearest_scene_get_info": (C.c_int, [_vp, C.POINTER(NearestSceneInfo_)]),
    "rls_nearest_hits": (C.c_int, [_ctx, _vp, C.POINTER(NearestRays_), C.POINTER(NearestFound_)]),
    "rls_nearest_walk_hits": (C.c_int, [_ctx, _vp, C.POINTER(WalkRays_), _i64, C.POINTER(NearestFound_)]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once) and prototype the companion library; RLSHADERS_AMD_NEAREST_LIB overrides its path.  The product library is
    loaded first (contexts, errors)."""
    global _lib
    if _lib is None:
        _lib = capi.load_companion("rlshaders_amd.nearest", NEAREST_LIB_PATH, "RLSHADERS_AMD_NEAREST_LIB", PROTOTYPES,
                                   "build_nearest_library", first=(capi.load,))
    return _lib


VECTORS = ("P", "N", "Ns", "T", "wo")
SCALARS = (("prim", torch.int32), ("surface", torch.int32), ("u", torch.float32), ("v", torch.float32))
ALL_PLANES = VECTORS + tuple(k for k, _ in SCALARS)


class Rays:
    """The rays of a query (rls_nearest_rays) over the caller's planes: origin float32 [3, .] (indexed by entry, or through
    ``via``: int32 [rays], a queue's point plane over sg->P), dir float32 [3, >= rays], maxdist float32 [rays] or None (+inf),
    count: an int64 device tensor of one element or None (all), ray: int32 [rays] ids for ``last`` or None (the entry's index).
    rays: the host bound, by default dir's width."""

    def __init__(self, origin: torch.Tensor, dir: torch.Tensor, maxdist: Optional[torch.Tensor] = None,
                 via: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None, ray: Optional[torch.Tensor] = None,
                 rays: Optional[int] = None):
        self.origin, self.dir, self.maxdist, self.via, self.count, self.ray = origin, dir, maxdist, via, count, ray
        self.rays = int(dir.shape[1]) if rays is None else int(rays)

    def struct(self) -> NearestRays_:
        r, n = NearestRays_(), self.rays
        r.rays = n
        r.count = None if self.count is None else _flat(self.count, 1, "rays.count", (torch.int64,))
        if n > 0:
            r.origin = _rows(self.origin, 1 if self.via is not None else n, "rays.origin", capi.CVec3)
            r.dir = _rows(self.dir, n, "rays.dir", capi.CVec3)
        r.via = None if self.via is None else _flat(self.via, n, "rays.via", _IDS)
        r.maxdist = None if self.maxdist is None else _flat(self.maxdist, n, "rays.maxdist", (torch.float32,))
        r.ray = None if self.ray is None else _flat(self.ray, n, "rays.ray", _IDS)
        return r


class Found:
    """The hits of a query (rls_nearest_found), indexed like its rays: hit uint8, t float32, and the planes asked for -- P, N,
    Ns, T, wo float32 [3, rays], prim, surface int32 (uint32 on the device), u, v float32, bin uint8 -- None where not asked
    for.  Planes other than hit (and bin) are written only where hit is set.  ``alloc(shape, dtype)``: where they come from."""

    def __init__(self, ctx, rays: int, planes=ALL_PLANES, bin: bool = False, alloc=None):
        unknown = set(planes) - set(ALL_PLANES)
        if unknown:
            raise ValueError(f"planes: unknown {sorted(unknown)}; known {ALL_PLANES}")
        dev = ctx.torch_device
        if alloc is None:
            alloc = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        self.rays = n = int(rays)
        self.hit, self.t = alloc((n,), torch.uint8), alloc((n,), torch.float32)
        for k in VECTORS:
            setattr(self, k, alloc((3, n), torch.float32) if k in planes else None)
        for k, dtype in SCALARS:
            setattr(self, k, alloc((n,), dtype) if k in planes else None)
        self.bin = alloc((n,), torch.uint8) if bin else None
        self.bin_of_surface = None

    def struct(self, n: int, bin_of_surface: Optional[torch.Tensor] = None, last: Optional[torch.Tensor] = None) -> NearestFound_:
        f = NearestFound_()
        if n > 0:
            f.hit = _flat(self.hit, n, "found.hit", (torch.uint8, torch.bool))
            f.t = _flat(self.t, n, "found.t", (torch.float32,))
            for k in VECTORS:
                if getattr(self, k) is not None:
                    setattr(f, k, _rows(getattr(self, k), n, "found." + k, capi.Vec3))
            for k, dtype in SCALARS:
                if getattr(self, k) is not None:
                    setattr(f, k, _flat(getattr(self, k), n, "found." + k, _IDS if dtype == torch.int32 else (dtype,)))
            if self.bin is not None:
                if bin_of_surface is None:
                    raise ValueError("found.bin is asked for without bin_of_surface")
                f.bin = _flat(self.bin, n, "found.bin", (torch.uint8,))
        if bin_of_surface is not None:
            f.bin_of_surface = _flat(bin_of_surface, 1, "bin_of_surface", (torch.uint8,))
            f.bin_count = int(bin_of_surface.shape[0])
        self.bin_of_surface = bin_of_surface
        f.last = None if last is None else _flat(last, 0, "last", _IDS)
        return f

    def _need(self, *names):
        missing = [k for k in names if getattr(self, k) is None]
        if missing:
            raise ValueError(f"nearest.Found: the planes {missing} were not asked for")

    def walk_found(self, objects: bool = True) -> walk.Found:
        """what ``ProbeWalk.step`` takes: hit, t, P, N, Ns and object = surface (objects=False: none, for a walk without
        ``own``), no adapter kernel"""
        self._need("P", "N", "Ns", *(["surface"] if objects else []))
        return walk.Found(self.hit, self.t, self.P, self.N, self.Ns, object=self.surface if objects else None)

    def shadow_found(self, opacity_table: torch.Tensor) -> shadow_walk.Found:
        """what ``ShadowWalk.step`` takes: hit, t, P and index = surface into ``opacity_table`` [3, surfaces]"""
        self._need("P", "surface")
        return shadow_walk.Found(self.hit, self.t, self.P, opacity_table, index=self.surface)

    def bins(self, bin_of_surface: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the node bin of every ray (``trace.route_hits``' input): bin_of_surface[min(surface, len - 1)], 255 for a miss, as
        the query wrote it; bin_of_surface: the table the query was given, to be sure of it"""
        self._need("bin")
        if bin_of_surface is not None and bin_of_surface is not self.bin_of_surface:
            raise ValueError("nearest.Found.bins: the query wrote the bins of another table")
        return self.bin

    def gatherable(self) -> tuple:
        """the per-ray planes a node call's dense batch is gathered from (``HitRoutes.gather(b, *found.gatherable())``):
        those of P, N, Ns, T, wo, surface, u, v that were asked for, in this order"""
        return tuple(getattr(self, k) for k in ("P", "N", "Ns", "T", "wo", "surface", "u", "v") if getattr(self, k) is not None)


def _u32(a, n, what):
    a = np.ascontiguousarray(np.asarray(a).astype(np.int64))
    if a.size != n or (a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF)):
        raise ValueError(f"{what}: expected {n} values in [0, 2^32)")
    return np.ascontiguousarray(a.astype(np.uint32))


class Scene:
    """A triangle mesh and its tree on ctx's device (rls_nearest_scene): vertices float32 [nv, 3] (finite), triangles [nt, 3]
    indices below nv, surface [nt] ids (default 0), normals float32 [nv, 3] per-vertex shading normals or None; host arrays
    (numpy, or anything numpy converts; CPU tensors too).  leaf_size 1 .. 8 (0: the default, 4) changes the tree, never a result.
    nt == 0 is a scene every ray misses; nt above RLS_NEAREST_MAX_TRIANGLES is refused."""

    def __init__(self, ctx, vertices, triangles, surface=None, normals=None, leaf_size: int = 0):
        self.ctx = ctx
        V = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
        nv = V.shape[0]
        tri = np.asarray(triangles).reshape(-1, 3)
        nt = tri.shape[0]
        T = _u32(tri, 3 * nt, "triangles")
        S = None if surface is None else _u32(surface, nt, "surface")
        Nn = None if normals is None else np.ascontiguousarray(np.asarray(normals, np.float32).reshape(-1, 3))
        if Nn is not None and Nn.shape[0] != nv:
            raise ValueError("normals: one per vertex")
        m = NearestMesh_()
        m.nv, m.nt, m.leaf_size = nv, nt, int(leaf_size)
        m.vertices, m.triangles = V.ctypes.data if nv else None, T.ctypes.data if nt else None
        m.surface = None if S is None or nt == 0 else S.ctypes.data
        m.normals = None if Nn is None or nv == 0 else Nn.ctypes.data
        h = C.c_void_p()
        check(load().rls_nearest_scene_create(ctx.handle, C.byref(m), C.byref(h)))
        self.handle = h
        info = NearestSceneInfo_()
        check(load().rls_nearest_scene_get_info(h, C.byref(info)))
        self.nv, self.nt, self.nodes, self.leaf_size, self.depth = info.nv, info.nt, info.nodes, info.leaf_size, info.depth
        self.device_bytes = info.device_bytes

    def close(self) -> None:
        if getattr(self, "handle", None):
            h, self.handle = self.handle, None
            check(load().rls_nearest_scene_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def hits(self, rays, active: Optional[int] = None, last: Optional[torch.Tensor] = None, found: Optional[Found] = None,
             planes=ALL_PLANES, bin_of_surface: Optional[torch.Tensor] = None, ctx=None) -> Found:
        """The nearest hit of every ray.  rays: a ``Rays``, or a walk's list (``ProbeWalk.rays`` / ``ShadowWalk.rays``: count,
        ray, origin, dir, maxdist), traced by rls_nearest_walk_hits with ``active`` as the bound on its device count (None: its
        capacity).  last: int32 [ids] (uint32 on the device), read as the triangle to skip and written with the triangle hit,
        indexed by the ray's id -- the list's ray plane, ``Rays.ray`` or the entry.  Without an id plane ``last`` must hold an
        entry per ray, which is checked here; with ``Rays.ray`` or a walk's list the ids are on the device and ``last`` must
        reach past the largest of them: that bound is the caller's, the kernel does not check it.  found: a ``Found`` to write again (no
        allocation: recordable by ``ctx.capture()``), else one with ``planes`` (and bin where bin_of_surface, uint8 [surfaces],
        is given) is made.  ctx: another context of the scene's device (a FAST one gives the same bytes)."""
        ctx = self.ctx if ctx is None else ctx
        if isinstance(rays, Rays):
            n = rays.rays if active is None else min(int(active), rays.rays)
            r = rays.struct()
            r.rays = n
        else:
            cap = int(rays.maxdist.shape[0])
            n = cap if active is None else min(int(active), cap)
            r = rays_struct(rays, cap, trials=False)
        if found is None:
            found = Found(ctx, n, planes=planes, bin=bin_of_surface is not None)
        elif found.rays < n:
            raise ValueError(f"found: made for {found.rays} rays, the query has {n}")
        if last is not None and isinstance(rays, Rays) and rays.ray is None and last.shape[0] < n:
            raise ValueError(f"last: {last.shape[0]} entries for {n} rays whose ids are their indices")
        f = found.struct(n, bin_of_surface, last)
        if isinstance(rays, Rays):
            check(load().rls_nearest_hits(ctx.handle, self.handle, C.byref(r), C.byref(f)))
        else:
            check(load().rls_nearest_walk_hits(ctx.handle, self.handle, C.byref(r), -1 if active is None else n, C.byref(f)))
        return found


class MovingMesh:
    """What the handles of the two moving-mesh libraries share (the box-only update's and the tree rebuild's module each subclass
    it): the handle borrows a ``Scene`` and keeps a reference to it.  A subclass sets PREFIX (its entry points are PREFIX +
    create, destroy, get_info, update, read_tree), load (its module's, a staticmethod) and Info and Mesh (its module's mirrors);
    every field of Info but ``updates`` becomes an attribute."""
    PREFIX = load = Info = Mesh = None

    def __init__(self, scene: "Scene"):
        self.scene, self.ctx = scene, scene.ctx
        lib = self.load()                                            # the entry points looked up once: update is a hot call
        self._entry = {verb: getattr(lib, self.PREFIX + verb) for verb in ("create", "destroy", "get_info", "update", "read_tree")}
        h = C.c_void_p()
        check(self._entry["create"](self.ctx.handle, scene.handle, C.byref(h)))
        self.handle = h
        self._held = ()
        for k, v in self.info().items():
            if k != "updates":
                setattr(self, k, v)

    def close(self) -> None:
        if getattr(self, "handle", None):
            h, self.handle = self.handle, None
            check(self._entry["destroy"](h))
        self.scene = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        i = self.Info()
        check(self._entry["get_info"](self.handle, C.byref(i)))
        return {k: bool(getattr(i, k)) if k == "has_normals" else getattr(i, k) for k, _ in self.Info._fields_}

    def _plane(self, a, what: str) -> torch.Tensor:
        """a device float32 [nv, 3], contiguous; a host array is uploaded (a copy: that path synchronises)"""
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3)))
        if a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != 3 or a.shape[0] != self.nv:
            raise ValueError(f"{what}: expected float32 [{self.nv}, 3]")
        if not a.is_cuda:
            a = a.to(self.ctx.torch_device)
        if not a.is_contiguous():
            raise ValueError(f"{what}: expected a contiguous tensor")
        return a

    def update(self, vertices, normals=None, parked: Optional[torch.Tensor] = None, ctx=None) -> Optional[torch.Tensor]:
        """Move the scene to ``vertices`` on the context's stream (the subclass says what that does to the tree): device float32
        tensors [nv, 3] (host arrays are uploaded first).  normals: None keeps the scene's; refused where the scene was made
        without normals.  parked: an int64 device tensor of one element, written with the number of triangles parked, and
        returned.  Neither synchronises nor allocates with device tensors, so it is recordable by ``ctx.capture()``; a replay
        reads the tensors as they are then."""
        ctx = self.ctx if ctx is None else ctx
        V = self._plane(vertices, "vertices")
        Nn = None if normals is None else self._plane(normals, "normals")
        m = self.Mesh()
        m.nv = self.nv
        m.vertices = V.data_ptr() if self.nv else None
        m.normals = None if Nn is None else (Nn.data_ptr() if self.nv else None)
        if parked is not None:
            m.parked = _flat(parked, 1, "parked", (torch.int64,))
        check(self._entry["update"](ctx.handle, self.handle, C.byref(m)))
        self._held = (V, Nn, parked)                                 # alive until the next update: the stream may still read them
        return parked

    def read_tree(self, ctx=None):
        """-> (boxes float32 [nodes, 6] lo xyz hi xyz, links uint32 [nodes, 2] first, meta, prims uint32 [nt] the triangle ids
        in leaf order), host arrays; synchronises."""
        ctx = self.ctx if ctx is None else ctx
        boxes, links = np.zeros((self.nodes, 6), np.float32), np.zeros((self.nodes, 2), np.uint32)
        prims = np.zeros((self.nt,), np.uint32)
        check(self._entry["read_tree"](ctx.handle, self.handle, boxes.ctypes.data, links.ctypes.data, prims.ctypes.data))
        return boxes, links, prims


class tracer:
    """A callable of the shape ``walk.run`` and ``shadow_walk.run`` take, ``tracer(rays, active) -> Found``, over a scene: the
    nearest hits of the listed rays, with ``last`` (one triangle id per queue ray, carried across the steps of a walk: a ray
    does not hit the triangle it stands on again) unless ``last=False``.  opacity: a table [3, surfaces] makes the result a
    ``shadow_walk.Found`` indexed by surface; without it a ``walk.Found``, with object = surface where ``objects`` is set (a
    probe walk with ``own``).  keep: found[k] = (active, the listed rays, the ``nearest.Found``) of call k, with prim, for the
    caller's records (e.g. to fold the visited hits).  The tracer carries ``last`` from call to call and cannot tell a new
    walk's first list from the next step of the old one without reading the device: call ``reset()`` before it serves another
    walk (``last`` forgets the triangles the previous walk ended on, ``found`` is emptied)."""

    def __init__(self, scene: Scene, opacity: Optional[torch.Tensor] = None, last=True, keep: bool = False, objects: bool = False):
        self.scene, self.opacity, self.keep, self.found, self.objects = scene, opacity, keep, [], objects
        self.last = last if isinstance(last, torch.Tensor) else None
        self._carry = last is not False

    def reset(self) -> "tracer":
        """before another walk: no ray skips a triangle, nothing is kept"""
        if self.last is not None:
            self.last.fill_(-1)
        self.found = []
        return self

    def __call__(self, rays, active):
        if self._carry and self.last is None:                        # ids are queue rays: below the list's capacity
            self.last = torch.full((max(int(rays.maxdist.shape[0]), 1),), -1, dtype=torch.int32, device=rays.maxdist.device)
        planes = ("P", "surface") if self.opacity is not None else ("P", "N", "Ns", "surface")
        f = self.scene.hits(rays, active=active, last=self.last if self._carry else None, planes=planes + ("prim",) if self.keep else planes)
        if self.keep:
            self.found.append((int(active), rays.ray[:int(active)].clone(), f))
        return f.shadow_found(self.opacity) if self.opacity is not None else f.walk_found(self.objects)


def host_stats(vertices, triangles, origin, dir, maxdist=None, skip=None, leaf_size: int = 0, per_ray: bool = False) -> dict:
    """The nodes and triangles the traversal visits for the given rays and the most stack entries a ray holds, counted on the CPU by the kernel's own traversal source
    over the library's own tree (csrc_nearest/nearest_stats.cpp, a stand-alone host program; no device).  vertices [nv, 3],
    triangles [nt, 3], origin / dir float32 [3, M] (numpy), maxdist [M] or None (+inf), skip [M] triangle ids or None.
    -> {"rays", "hits", "nodes", "triangles" (totals), "max_stack" (the largest of the rays'; at most depth - 1), "tree_nodes",
    "depth"} and, with per_ray, "per_ray": a row [hit, prim, nodes, triangles, max_stack] per ray."""
    import json
    import subprocess
    import tempfile
    from . import build
    exe = build.build_nearest_stats()
    V = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
    T = _u32(np.asarray(triangles).reshape(-1, 3), 3 * (np.asarray(triangles).size // 3), "triangles")
    o, d = np.asarray(origin, np.float32), np.asarray(dir, np.float32)
    M = d.shape[1]
    rec = np.empty((M, 8), np.uint32)
    rec[:, 0:3], rec[:, 3:6] = o.T.copy().view(np.uint32), d.T.copy().view(np.uint32)
    rec[:, 6] = (np.full(M, np.inf, np.float32) if maxdist is None else np.ascontiguousarray(maxdist, np.float32)).view(np.uint32)
    rec[:, 7] = RLS_NEAREST_NO_PRIM if skip is None else _u32(skip, M, "skip")
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "rays.bin"
        with open(path, "wb") as f:
            f.write(np.array([V.shape[0], T.size // 3, leaf_size or RLS_NEAREST_DEFAULT_LEAF, M], np.int64).tobytes())
            f.write(V.tobytes() + T.tobytes() + rec.tobytes())
        p = subprocess.run([str(exe), str(path)] + (["--per-ray"] if per_ray else []), capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"nearest_stats failed: {p.stderr}")
    return json.loads(p.stdout)
