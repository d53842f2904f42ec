"""Moving meshes: rebuild the tree of a nearest-hit scene on the device (include/rlshaders_amd_nearest_rebuild.h, companion library
``librls_nearest_rebuild.so``).

    scene = nearest.Scene(ctx, vertices, triangles, surface=ids, normals=vertex_normals)   # the tree is built once, on the host
    rebuild = nearest_rebuild.Rebuild(scene)                # the update's working set is allocated here
    every so often:
        rebuild.update(deformed)                            # device float32 [nv, 3]; no synchronisation, recordable
        walk.run(probes, P, nearest.tracer(scene))          # ... every query on the same stream sees the new tree

After an update the scene holds the tree the host builder builds from the moved vertices: the same links, split axes and leaf
order, every box equal by value.  So every query returns, bit for bit, what a fresh ``nearest.Scene`` on the moved vertices
returns, and costs what it costs there.  A triangle with a NaN or an infinity among its coordinates is parked (it never hits);
``parked`` counts them.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _capi as capi
from . import nearest
from ._capi import check

NEAREST_REBUILD_LIB_PATH = capi._PKG / "lib" / "librls_nearest_rebuild.so"


class NearestRebuildInfo_(C.Structure):
    """rls_nearest_rebuild_info"""
    _fields_ = [("nv", C.c_int64), ("nt", C.c_int64), ("nodes", C.c_int64), ("levels", C.c_int), ("leaf_size", C.c_int),
                ("has_normals", C.c_int), ("device_bytes", C.c_size_t), ("updates", C.c_int64)]


class NearestRebuildMesh_(C.Structure):
    """rls_nearest_rebuild_mesh"""
    _fields_ = [("nv", C.c_int64), ("vertices", C.c_void_p), ("normals", C.c_void_p), ("parked", C.c_void_p)]


_ctx, _vp = C.c_void_p, C.c_void_p
PROTOTYPES = {
    "rls_nearest_rebuild_create": (C.c_int, [_ctx, _vp, C.POINTER(_vp)]),
    "rls_nearest_rebuild_destroy": (C.c_int, [_vp]),
    "rls_nearest_rebuild_get_info": (C.c_int, [_vp, C.POINTER(NearestRebuildInfo_)]),
    "rls_nearest_rebuild_update": (C.c_int, [_ctx, _vp, C.POINTER(NearestRebuildMesh_)]),
    "rls_nearest_rebuild_read_tree": (C.c_int, [_ctx, _vp, _vp, _vp, _vp]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once) and prototype the companion library; RLSHADERS_AMD_NEAREST_REBUILD_LIB overrides its path.  The product
    library and the nearest-hit library (whose scenes it reads) are loaded first."""
    global _lib
    if _lib is None:
        _lib = capi.load_companion("rlshaders_amd.nearest_rebuild", NEAREST_REBUILD_LIB_PATH, "RLSHADERS_AMD_NEAREST_REBUILD_LIB",
                                   PROTOTYPES, "build_nearest_rebuild_library", first=(nearest.load,))
    return _lib


class Rebuild:
    """The rebuild of a ``nearest.Scene`` (rls_nearest_rebuild): it borrows the scene and keeps a reference to it.  Creation reads
    the scene's links once (it may synchronise) and allocates the update's working set (``device_bytes``)."""

    def __init__(self, scene: "nearest.Scene"):
        self.scene, self.ctx = scene, scene.ctx
        h = C.c_void_p()
        check(load().rls_nearest_rebuild_create(self.ctx.handle, scene.handle, C.byref(h)))
        self.handle = h
        self._held = ()
        i = self.info()
        self.nv, self.nt, self.nodes, self.levels, self.has_normals = i["nv"], i["nt"], i["nodes"], i["levels"], i["has_normals"]
        self.leaf_size = i["leaf_size"]
        self.device_bytes = i["device_bytes"]

    def close(self) -> None:
        if getattr(self, "handle", None):
            h, self.handle = self.handle, None
            check(load().rls_nearest_rebuild_destroy(h))
        self.scene = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        i = NearestRebuildInfo_()
        check(load().rls_nearest_rebuild_get_info(self.handle, C.byref(i)))
        return dict(nv=i.nv, nt=i.nt, nodes=i.nodes, levels=i.levels, leaf_size=i.leaf_size, has_normals=bool(i.has_normals),
                    device_bytes=i.device_bytes, updates=i.updates)

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
        """Rebuild the scene's tree for ``vertices`` on the context's stream: device float32 tensors [nv, 3] (host arrays are uploaded
        first).  normals: None keeps the scene's; refused where the scene was made without normals.  parked: an int64 device
        tensor of one element, written with the number of triangles parked, and returned.  Neither synchronises nor allocates
        with device tensors, so it is recordable by ``ctx.capture()``; a replay reads the tensors as they are then."""
        ctx = self.ctx if ctx is None else ctx
        V = self._plane(vertices, "vertices")
        Nn = None if normals is None else self._plane(normals, "normals")
        m = NearestRebuildMesh_()
        m.nv = self.nv
        m.vertices = V.data_ptr() if self.nv else None
        m.normals = None if Nn is None else (Nn.data_ptr() if self.nv else None)
        if parked is not None:
            m.parked = nearest._flat(parked, 1, "parked", (torch.int64,))
        check(load().rls_nearest_rebuild_update(ctx.handle, self.handle, C.byref(m)))
        self._held = (V, Nn, parked)                                 # alive until the next update: the stream may still read them
        return parked

    def read_tree(self, ctx=None):
        """-> (boxes float32 [nodes, 6] lo xyz hi xyz, links uint32 [nodes, 2] first, meta, prims uint32 [nt] the triangle ids
        in leaf order), host arrays; synchronises."""
        ctx = self.ctx if ctx is None else ctx
        boxes, links = np.zeros((self.nodes, 6), np.float32), np.zeros((self.nodes, 2), np.uint32)
        prims = np.zeros((self.nt,), np.uint32)
        check(load().rls_nearest_rebuild_read_tree(ctx.handle, self.handle, boxes.ctypes.data, links.ctypes.data, prims.ctypes.data))
        return boxes, links, prims
