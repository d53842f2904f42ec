"""Instanced scenes: nearest hits over many placed meshes (include/rlshaders_amd_nearest_group.h, companion library
``librls_nearest_group.so``).

    scene = nearest.Scene(ctx, vertices, triangles, surface=ids, normals=vertex_normals)   # one mesh, one tree
    group = nearest_group.Group(ctx, [nearest_group.Instance(scene, M, surface_base=8 * k) for k, M in enumerate(placements)])
    walk.run(probes, P, nearest_group.tracer(group))                           # the walks, through every instance
    f = group.hits(nearest.Rays(P, q.dir, via=q.point), bin_of_surface=bins)   # f.instance beside f.prim, f.surface based
    group.update(to_object, to_world)                                          # device float32 [instances, 12]; recordable

The result of a query is a function of the instances, their meshes and the ray alone (the header's statement;
tests/nearest_group_util.py restates it in numpy): neither tree, no leaf size and no math mode changes a bit of it.  After an
update every query returns what a fresh ``Group`` with those matrices over those scenes returns.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _capi as capi
from . import nearest
from ._capi import check
from .walk import _IDS, WalkRays_, _flat, rays_struct

NEAREST_GROUP_LIB_PATH = capi._PKG / "lib" / "librls_nearest_group.so"

RLS_NEAREST_GROUP_STACK = 16
RLS_NEAREST_GROUP_MAX_INSTANCES = 1 << 16
RLS_NEAREST_GROUP_MAX_LEAF = 4
RLS_NEAREST_GROUP_DEFAULT_LEAF = 2
RLS_NEAREST_NO_INSTANCE = 0xFFFFFFFF


class NearestInstance_(C.Structure):
    """rls_nearest_instance"""
    _fields_ = [("scene", C.c_void_p), ("to_object", C.c_float * 12), ("to_world", C.c_float * 12), ("surface_base", C.c_uint32)]


class NearestGroupInfo_(C.Structure):
    """rls_nearest_group_info"""
    _fields_ = [("instances", C.c_int64), ("scenes", C.c_int64), ("top_nodes", C.c_int64), ("top_depth", C.c_int), ("leaf_size", C.c_int),
                ("device_bytes", C.c_size_t), ("updates", C.c_int64)]


class NearestGroupMoves_(C.Structure):
    """rls_nearest_group_moves"""
    _fields_ = [("to_object", C.c_void_p), ("to_world", C.c_void_p), ("parked", C.c_void_p)]


class NearestGroupFound_(C.Structure):
    """rls_nearest_group_found"""
    _fields_ = [("found", nearest.NearestFound_), ("instance", C.c_void_p), ("last_instance", C.c_void_p)]


_ctx, _i64, _vp = C.c_void_p, C.c_int64, C.c_void_p
PROTOTYPES = {
    "rls_nearest_group_create": (C.c_int, [_ctx, C.POINTER(NearestInstance_), _i64, C.c_int, C.POINTER(_vp)]),
    "rls_nearest_group_destroy": (C.c_int, [_vp]),
    "rls_nearest_group_get_info": (C.c_int, [_vp, C.POINTER(NearestGroupInfo_)]),
    "rls_nearest_group_update": (C.c_int, [_ctx, _vp, C.POINTER(NearestGroupMoves_)]),
    "rls_nearest_group_hits": (C.c_int, [_ctx, _vp, C.POINTER(nearest.NearestRays_), C.POINTER(NearestGroupFound_)]),
    "rls_nearest_group_walk_hits": (C.c_int, [_ctx, _vp, C.POINTER(WalkRays_), _i64, C.POINTER(NearestGroupFound_)]),
    "rls_nearest_group_read_tree": (C.c_int, [_ctx, _vp, _vp, _vp, _vp, _vp, _vp]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once) and prototype the companion library; RLSHADERS_AMD_NEAREST_GROUP_LIB overrides its path.  The product
    library and the nearest-hit library (whose scenes it reads) are loaded first."""
    global _lib
    if _lib is None:
        _lib = capi.load_companion("rlshaders_amd.nearest_group", NEAREST_GROUP_LIB_PATH, "RLSHADERS_AMD_NEAREST_GROUP_LIB",
                                   PROTOTYPES, "build_nearest_group_library", first=(nearest.load,))
    return _lib


ALL_PLANES = nearest.ALL_PLANES + ("instance",)


def _matrix(M, what: str) -> np.ndarray:
    """a 3 x 4 (or the top of a 4 x 4) matrix, or 12 floats -> float64 [3, 4]"""
    a = np.asarray(M, np.float64)
    if a.shape == (4, 4):
        a = a[:3]
    if a.size != 12:
        raise ValueError(f"{what}: expected a 3 x 4 or 4 x 4 matrix")
    return a.reshape(3, 4)


class Instance:
    """A scene placed in the world (rls_nearest_instance): to_world a 3 x 4 (or 4 x 4 affine) matrix, object -> world;
    surface_base is added to the mesh's surface ids; to_object: world -> object, by default the float64 inverse of to_world
    rounded to float32.  The library never inverts a matrix and never checks that the two are inverses."""

    def __init__(self, scene: nearest.Scene, to_world, surface_base: int = 0, to_object=None):
        self.scene, self.surface_base = scene, int(surface_base)
        B = _matrix(to_world, "to_world")
        if to_object is None:
            with np.errstate(all="ignore"):
                try:
                    A = np.linalg.inv(np.vstack([B, [0.0, 0.0, 0.0, 1.0]]))[:3]
                except np.linalg.LinAlgError:
                    A = np.full((3, 4), np.nan)
        else:
            A = _matrix(to_object, "to_object")
        with np.errstate(all="ignore"):
            self.to_world, self.to_object = B.astype(np.float32), A.astype(np.float32)


class Found(nearest.Found):
    """``nearest.Found`` and ``instance`` int32 (uint32 on the device), written where hit is set; ``surface`` is the based id"""

    def __init__(self, ctx, rays: int, planes=ALL_PLANES, bin: bool = False, alloc=None):
        unknown = set(planes) - set(ALL_PLANES)
        if unknown:
            raise ValueError(f"planes: unknown {sorted(unknown)}; known {ALL_PLANES}")
        super().__init__(ctx, rays, planes=tuple(k for k in planes if k != "instance"), bin=bin, alloc=alloc)
        if alloc is None:
            alloc = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=ctx.torch_device)
        self.instance = alloc((self.rays,), torch.int32) if "instance" in planes else None

    def group_struct(self, n: int, bin_of_surface=None, last=None, last_instance=None) -> NearestGroupFound_:
        if (last is None) != (last_instance is None):
            raise ValueError("last and last_instance are a pair: both or neither")
        f = NearestGroupFound_()
        f.found = self.struct(n, bin_of_surface, last)
        if n > 0 and self.instance is not None:
            f.instance = _flat(self.instance, n, "found.instance", _IDS)
        f.last_instance = None if last_instance is None else _flat(last_instance, 0, "last_instance", _IDS)
        return f


class Group:
    """Instances under a top-level tree on ctx's device (rls_nearest_group).  instances: ``Instance``s, 0 ..
    RLS_NEAREST_GROUP_MAX_INSTANCES of them (none: a group every ray misses); one scene may stand in any number.  The group
    borrows the scenes and keeps references to them.  leaf_size 1 .. 4 (0: the default) changes the top tree, never a result."""

    def __init__(self, ctx, instances, leaf_size: int = 0):
        self.ctx = ctx
        instances = list(instances)
        self.scenes = [i.scene for i in instances]                   # alive as long as the group
        n = len(instances)
        arr = (NearestInstance_ * max(n, 1))()
        for k, i in enumerate(instances):
            arr[k].scene = i.scene.handle
            arr[k].to_object[:] = i.to_object.reshape(-1).tolist()
            arr[k].to_world[:] = i.to_world.reshape(-1).tolist()
            arr[k].surface_base = i.surface_base & 0xFFFFFFFF
        h = C.c_void_p()
        check(load().rls_nearest_group_create(ctx.handle, arr, n, int(leaf_size), C.byref(h)))
        self.handle = h
        self._held = ()
        for k, v in self.info().items():
            if k != "updates":
                setattr(self, k, v)

    def close(self) -> None:
        if getattr(self, "handle", None):
            h, self.handle = self.handle, None
            check(load().rls_nearest_group_destroy(h))
        self.scenes = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        i = NearestGroupInfo_()
        check(load().rls_nearest_group_get_info(self.handle, C.byref(i)))
        return {k: getattr(i, k) for k, _ in NearestGroupInfo_._fields_}

    def _plane(self, a, what: str) -> torch.Tensor:
        """a device float32 [instances, 12] (or [instances, 3, 4]), contiguous; a host array is uploaded (that path synchronises)"""
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 12)))
        if a.dtype != torch.float32 or a.numel() != 12 * self.instances:
            raise ValueError(f"{what}: expected float32 [{self.instances}, 12]")
        if not a.is_cuda:
            a = a.to(self.ctx.torch_device)
        if not a.is_contiguous():
            raise ValueError(f"{what}: expected a contiguous tensor")
        return a

    def update(self, to_object=None, to_world=None, parked: Optional[torch.Tensor] = None, ctx=None) -> Optional[torch.Tensor]:
        """Move the instances on the context's stream: both matrix planes, device float32 [instances, 12] (host arrays are
        uploaded first), or neither -- the matrices stay and the world boxes are taken again from the scenes as they are then
        (after a ``Refit.update`` / ``Rebuild.update`` of a member scene on the same stream).  parked: an int64 device tensor of
        one element, written with the number of instances parked, and returned.  Neither synchronises nor allocates with device
        tensors, so it is recordable by ``ctx.capture()``; a replay reads the tensors as they are then."""
        ctx = self.ctx if ctx is None else ctx
        if (to_object is None) != (to_world is None):
            raise ValueError("to_object and to_world: both or neither")
        A = None if to_object is None else self._plane(to_object, "to_object")
        B = None if to_world is None else self._plane(to_world, "to_world")
        m = NearestGroupMoves_()
        if A is not None and self.instances:
            m.to_object, m.to_world = A.data_ptr(), B.data_ptr()
        if parked is not None:
            m.parked = _flat(parked, 1, "parked", (torch.int64,))
        check(load().rls_nearest_group_update(ctx.handle, self.handle, C.byref(m)))
        self._held = (A, B, parked)                                  # alive until the next update: the stream may still read them
        return parked

    def read_tree(self, ctx=None):
        """-> (boxes float32 [top_nodes, 6] lo xyz hi xyz, links uint32 [top_nodes, 2] first, meta, order uint32 [instances] the
        instance ids in leaf order, world float32 [instances, 6] W_j by instance, parked uint8 [instances]), host arrays;
        synchronises."""
        ctx = self.ctx if ctx is None else ctx
        boxes, links = np.zeros((self.top_nodes, 6), np.float32), np.zeros((self.top_nodes, 2), np.uint32)
        order, world = np.zeros((self.instances,), np.uint32), np.zeros((self.instances, 6), np.float32)
        parked = np.zeros((self.instances,), np.uint8)
        check(load().rls_nearest_group_read_tree(ctx.handle, self.handle, boxes.ctypes.data, links.ctypes.data, order.ctypes.data,
                                                 world.ctypes.data, parked.ctypes.data))
        return boxes, links, order, world, parked

    def hits(self, rays, active: Optional[int] = None, last: Optional[torch.Tensor] = None, last_instance: Optional[torch.Tensor] = None,
             found: Optional[Found] = None, planes=ALL_PLANES, bin_of_surface: Optional[torch.Tensor] = None, ctx=None) -> Found:
        """The nearest hit of every ray over all instances; as ``nearest.Scene.hits``.  last and last_instance: int32 [ids], a
        pair -- read as the (instance, triangle) to skip and written with the one hit, indexed by the ray's id."""
        ctx = self.ctx if ctx is None else ctx
        listed = not isinstance(rays, nearest.Rays)
        if not listed:
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
        if last is not None and not listed and rays.ray is None and min(last.shape[0], last_instance.shape[0] if last_instance is not None else 0) < n:
            raise ValueError(f"last, last_instance: fewer entries than the {n} rays whose ids are their indices")
        f = found.group_struct(n, bin_of_surface, last, last_instance)
        if not listed:
            check(load().rls_nearest_group_hits(ctx.handle, self.handle, C.byref(r), C.byref(f)))
        else:
            check(load().rls_nearest_group_walk_hits(ctx.handle, self.handle, C.byref(r), -1 if active is None else n, C.byref(f)))
        return found


class tracer(nearest.tracer):
    """``nearest.tracer`` over a group: a callable of the shape ``walk.run`` and ``shadow_walk.run`` take.  It carries the pair
    ``last`` / ``last_instance`` from call to call (a ray does not hit the triangle OF THE INSTANCE it stands on again; the same
    triangle id of another instance is not skipped); keep: found[k] holds prim and instance too."""

    def __init__(self, group: Group, opacity: Optional[torch.Tensor] = None, last=True, keep: bool = False, objects: bool = False):
        super().__init__(group, opacity=opacity, last=last, keep=keep, objects=objects)
        self.group, self.last_instance = group, None

    def reset(self) -> "tracer":
        if self.last_instance is not None:
            self.last_instance.fill_(-1)
        return super().reset()

    def __call__(self, rays, active):
        if self._carry:
            n = max(int(rays.maxdist.shape[0]), 1)                   # ids are queue rays: below the list's capacity
            if self.last is None:
                self.last = torch.full((n,), -1, dtype=torch.int32, device=rays.maxdist.device)
            if self.last_instance is None:
                self.last_instance = torch.full((int(self.last.shape[0]),), -1, dtype=torch.int32, device=rays.maxdist.device)
        planes = ("P", "surface") if self.opacity is not None else ("P", "N", "Ns", "surface")
        f = self.group.hits(rays, active=active, last=self.last if self._carry else None,
                            last_instance=self.last_instance if self._carry else None,
                            planes=planes + ("prim", "instance") if self.keep else planes)
        if self.keep:
            self.found.append((int(active), rays.ray[:int(active)].clone(), f))
        return f.shadow_found(self.opacity) if self.opacity is not None else f.walk_found(self.objects)
