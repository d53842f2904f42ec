"""Moving meshes: refit the tree of a nearest-hit scene on the device (include/rlshaders_amd_nearest_refit.h, companion library
``librls_nearest_refit.so``).

    scene = nearest.Scene(ctx, vertices, triangles, surface=ids, normals=vertex_normals)   # the tree is built once, on the host
    refit = nearest_refit.Refit(scene)
    for frame in frames:
        refit.update(deformed)                              # device float32 [nv, 3]; no synchronisation, recordable
        walk.run(probes, P, nearest.tracer(scene))          # ... every query on the same stream sees the moved mesh

After an update every query returns, bit for bit, what a fresh ``nearest.Scene`` on the moved vertices returns: the result of a
query is a function of the mesh and the ray alone and the update makes every node box contain what is below it again.  Only the
cost can drift.  A triangle with a NaN or an infinity among its coordinates is parked (it never hits); ``parked`` counts them.
"""
from __future__ import annotations

import ctypes as C

from . import _capi as capi
from . import nearest

NEAREST_REFIT_LIB_PATH = capi._PKG / "lib" / "librls_nearest_refit.so"


class NearestRefitInfo_(C.Structure):
    """rls_nearest_refit_info"""
    _fields_ = [("nv", C.c_int64), ("nt", C.c_int64), ("nodes", C.c_int64), ("levels", C.c_int), ("has_normals", C.c_int),
                ("device_bytes", C.c_size_t), ("updates", C.c_int64)]


class NearestRefitMesh_(C.Structure):
    """rls_nearest_refit_mesh"""
    _fields_ = [("nv", C.c_int64), ("vertices", C.c_void_p), ("normals", C.c_void_p), ("parked", C.c_void_p)]


_ctx, _vp = C.c_void_p, C.c_void_p
PROTOTYPES = {
    "rls_nearest_refit_create": (C.c_int, [_ctx, _vp, C.POINTER(_vp)]),
    "rls_nearest_refit_destroy": (C.c_int, [_vp]),
    "rls_nearest_refit_get_info": (C.c_int, [_vp, C.POINTER(NearestRefitInfo_)]),
    "rls_nearest_refit_update": (C.c_int, [_ctx, _vp, C.POINTER(NearestRefitMesh_)]),
    "rls_nearest_refit_read_tree": (C.c_int, [_ctx, _vp, _vp, _vp, _vp]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once) and prototype the companion library; RLSHADERS_AMD_NEAREST_REFIT_LIB overrides its path.  The product
    library and the nearest-hit library (whose scenes it reads) are loaded first."""
    global _lib
    if _lib is None:
        _lib = capi.load_companion("rlshaders_amd.nearest_refit", NEAREST_REFIT_LIB_PATH, "RLSHADERS_AMD_NEAREST_REFIT_LIB",
                                   PROTOTYPES, "build_nearest_refit_library", first=(nearest.load,))
    return _lib


class Refit(nearest.MovingMesh):
    """The refit of a ``nearest.Scene`` (rls_nearest_refit): it borrows the scene and keeps a reference to it.  Creation reads
    the scene's tree once (it may synchronise).  ``update`` rewrites the boxes of the tree that is there."""
    PREFIX, Info, Mesh, load = "rls_nearest_refit_", NearestRefitInfo_, NearestRefitMesh_, staticmethod(load)
