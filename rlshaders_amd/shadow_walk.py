"""Shadow rays walked on the device (include/rlshaders_amd_shadow_walk.h, companion library ``librls_shadow_walk.so``): between
a light loop's emit and its resolve the renderer owes a visibility per shadow ray.  ``trace.shadow_visibility`` folds it from a
finished list of all hits of every ray; ``ShadowWalk`` forms the same plane from NEAREST hits, surface by surface, and ends a
ray at an opaque surface, at the light, or when its budget of steps is spent.

    q = trace.ggx_shadow_rays(ggx, shader, P, lights, spp_n=2, seed=7)   # the light loop's shadow rays
    w = shadow_walk.ShadowWalk(ctx, q, P, max_steps=8)                   # begin: T = 1, the rays with maxdist > 0 listed
    while w.active:                                                      # at most max_steps steps
        r = w.rays                                                       # views of the list: r.ray, r.origin, r.dir, r.maxdist
        w.step(my_nearest_hit(r.origin, r.dir, r.maxdist))               # Found(hit, t, P, opacity[, index]), an entry per listed ray
    dd, ds = q.resolve(w.visibility)                                     # T of every ray: what every resolve reads

    shadow_walk.run(q, P, tracer, max_steps=8)                           # the loop above; tracer(rays, active) -> Found

``active`` reads the device (it synchronises); the constructor and ``step`` do not -- the queue's ray count is read on the
device -- and with ``bound`` left at the list's capacity a whole walk can be recorded by ``ctx.capture()``: steps on an empty
list do nothing.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _capi as capi
from . import trace
from ._capi import check
from .walk import ListWalk, WalkRays_, _flat, _rows       # the active list (rls_walk_rays) and its host layer are the probe walk's

SHADOW_WALK_LIB_PATH = capi._PKG / "lib" / "librls_shadow_walk.so"

RLS_SHADOW_WALK_MAX_STEPS = 255


class ShadowWalkFound_(C.Structure):
    """rls_shadow_walk_found"""
    _fields_ = [("hit", C.c_void_p), ("t", C.c_void_p), ("P", capi.CVec3), ("opacity", capi.CRgb), ("index", C.c_void_p),
                ("table_count", C.c_uint32)]


class ShadowWalk_(C.Structure):
    """rls_shadow_walk"""
    _fields_ = [("rays", C.c_int64), ("count", C.c_void_p), ("max_steps", C.c_int), ("O", capi.CVec3), ("via", C.c_void_p),
                ("base", capi.CRgb), ("visibility", capi.Rgb), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


_ctx, _i64 = C.c_void_p, C.c_int64
PROTOTYPES = {
    "rls_shadow_walk_scratch_bytes": (C.c_int, [_i64, C.POINTER(C.c_size_t)]),
    "rls_shadow_walk_begin": (C.c_int, [_ctx, C.POINTER(ShadowWalk_), C.POINTER(trace.ShadowQueue_), C.POINTER(WalkRays_)]),
    "rls_shadow_walk_step": (C.c_int, [_ctx, C.POINTER(ShadowWalk_), C.POINTER(WalkRays_), C.POINTER(ShadowWalkFound_), _i64,
                                       C.POINTER(WalkRays_)]),
    "rls_shadow_walk_active": (C.c_int, [_ctx, C.POINTER(WalkRays_), C.POINTER(C.c_int64)]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once) and prototype the companion library; RLSHADERS_AMD_SHADOW_WALK_LIB overrides its path.  The product and the
    trace library are loaded first (contexts, errors; the queues the walk starts on)."""
    global _lib
    if _lib is None:
        _lib = capi.load_companion("rlshaders_amd.shadow_walk", SHADOW_WALK_LIB_PATH, "RLSHADERS_AMD_SHADOW_WALK_LIB", PROTOTYPES,
                                   "build_shadow_walk_library", first=(trace.load,))
    return _lib


def scratch_bytes(rays: int) -> int:
    b = C.c_size_t()
    check(load().rls_shadow_walk_scratch_bytes(int(rays), C.byref(b)))
    return int(b.value)


class Found:
    """The renderer's nearest hit of every listed ray (rls_shadow_walk_found), indexed like the list a step reads: hit uint8 (or
    bool), t float32 (the distance from the entry's origin), P float32 [3, >= active], and the hit's opacity: float32
    [3, >= active] per entry, or with ``index`` (int32 [>= active], uint32 on the device) a table [3, table_count] of out_opacity
    values, e.g. ``trace.ggx_opacity``'s; an index past the table reads its last entry."""

    def __init__(self, hit, t, P, opacity, index=None):
        self.hit, self.t, self.P, self.opacity, self.index = hit, t, P, opacity, index

    def struct(self, n: int) -> ShadowWalkFound_:
        f = ShadowWalkFound_()
        f.hit = _flat(self.hit, n, "found.hit", (torch.uint8, torch.bool))
        f.t = _flat(self.t, n, "found.t", (torch.float32,))
        f.P = _rows(self.P, n, "found.P", capi.CVec3)
        if self.index is None:
            f.opacity, f.index, f.table_count = _rows(self.opacity, n, "found.opacity", capi.CRgb), None, 0
        else:
            f.opacity = _rows(self.opacity, 1, "found.opacity", capi.CRgb)
            f.index, f.table_count = _flat(self.index, n, "found.index", (torch.int32,)), int(self.opacity.shape[1])
        return f


class RawQueue:
    """A shadow queue over the caller's own planes, as far as the walk reads it: dir float32 [3, rays], maxdist float32 [rays],
    point int32 [rays] (uint32 on the device), count: an int64 device tensor of one element holding the number of rays, or
    None for all of them."""

    def __init__(self, dir: torch.Tensor, maxdist: torch.Tensor, point: torch.Tensor, count: Optional[torch.Tensor] = None):
        self.capacity = int(maxdist.shape[0])
        self.dir, self.maxdist, self.point, self.count = dir, maxdist, point, count
        q = trace.ShadowQueue_()
        q.capacity = self.capacity
        if self.capacity > 0:
            q.dir = _rows(dir, self.capacity, "dir", capi.Vec3)
            q.maxdist = _flat(maxdist, self.capacity, "maxdist", (torch.float32,))
            q.point = _flat(point, self.capacity, "point", (torch.int32,))
        self.q = q


def _queue(queue):
    """-> (rls_shadow_queue, capacity, the device address of its ray count or None)"""
    if isinstance(queue, trace.HitQueues):
        return queue.q.shadow, queue.shadow_capacity, queue.shadow_offsets[queue.hit_capacity:].data_ptr()
    if isinstance(queue, trace.ShadowQueue):
        return queue.q, queue.capacity, queue.offsets[queue.n:].data_ptr()
    if isinstance(queue, RawQueue):
        return queue.q, queue.capacity, None if queue.count is None else _flat(queue.count, 1, "count", (torch.int64,))
    raise TypeError("queue: a trace.ShadowQueue (also the shadow queue of a node's queue set), a trace.HitQueues or a RawQueue")


class ShadowWalk(ListWalk):
    """The walk of a shadow queue's rays: begun on construction.  queue: a ``trace.ShadowQueue`` (``trace.ggx_shadow_rays``,
    ``disney_shadow_rays``, the shadow queue of a node's queue set), a ``trace.HitQueues`` (its shadow queue, with
    ``via=queues._hit_element`` and O the hit planes [3, max_hits * stride]) or a ``RawQueue``.  O [3, .]: the origins' table,
    indexed by the queue's point plane (sg->P per point), or through ``via`` (int64).  base [3, >= rays]: T's start, None for
    1; it may be ``out``.  max_steps: the surfaces a ray may cross, 1 .. 255.  out [3, >= rays]: the visibility planes;
    scratch: a uint8 tensor of scratch_bytes(rays); alloc(shape, dtype) -> a contiguous device tensor: where the walk's lists,
    visibility and scratch come from (torch.empty by default)."""

    def __init__(self, ctx, queue, O: torch.Tensor, base: Optional[torch.Tensor] = None, via: Optional[torch.Tensor] = None,
                 max_steps: int = 16, out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None, alloc=None):
        self.queue, self.O, self.base, self.via = queue, O, base, via
        self.q, rays, count = _queue(queue)
        self.capacity, self.max_steps = rays, int(max_steps)
        alloc = self._alloc(ctx, alloc)
        self.visibility = alloc((3, rays), torch.float32) if out is None else out
        w = ShadowWalk_()
        w.rays, w.count, w.max_steps = rays, count, self.max_steps
        if rays > 0:
            w.O = _rows(O, 1, "O", capi.CVec3)
            w.visibility = _rows(self.visibility, rays, "out", capi.Rgb)
        w.via = None if via is None else _flat(via, 0, "via", (torch.int64,))
        if base is not None and rays > 0:
            w.base = _rows(base, rays, "base", capi.CRgb)
        lib = load()
        self._start(ctx, w, self.q, rays, scratch_bytes(rays), scratch, alloc, lib.rls_shadow_walk_begin, lib.rls_shadow_walk_step,
                    lib.rls_shadow_walk_active)


def run(queue, O: torch.Tensor, tracer, base: Optional[torch.Tensor] = None, via: Optional[torch.Tensor] = None,
        max_steps: int = 16, out: Optional[torch.Tensor] = None, ctx=None) -> ShadowWalk:
    """Walk the queue's rays to the end: tracer(rays, active) -> Found, the nearest hits of the first ``active`` listed rays.  At
    most max_steps steps."""
    w = ShadowWalk(queue.ctx if ctx is None else ctx, queue, O, base=base, via=via, max_steps=max_steps, out=out)
    return w.drive(tracer, w.max_steps)
