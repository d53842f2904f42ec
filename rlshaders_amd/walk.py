"""rlSss's probe walk on the device (include/rlshaders_amd_walk.h, companion library ``librls_walk.so``): between
``trace.sss_probe_rays`` and ``ProbeQueue.resolve`` the reference walks every probe ray through the object
(SssSampler::traceProbe, src/rlSss.h:288-357).  ``ProbeWalk`` is that walk; the renderer's part is a nearest-hit query.

    p = trace.sss_probe_rays(sss, P, spp_n=4, seed=7)            # the probe rays, dense
    w = walk.ProbeWalk(ctx, p, P)                                # begin: the rays with maxdist > 0 listed
    while w.active:                                              # at most 12 steps: the walk's trial budget
        r = w.rays                                               # views of the list: r.ray, r.origin, r.dir, r.maxdist [.., active]
        w.step(my_nearest_hit(r.origin, r.dir, r.maxdist))       # Found(hit, t, P, N, Ns[, object]), one entry per listed ray
    res = p.resolve(*w.hits(E))                                  # count, P, N as the resolves read them, E the caller's

    walk.run(p, P, tracer)                                       # the loop above; tracer(rays, active) -> Found

``active`` reads the device (it synchronises); ``step`` does not, and with ``bound`` left at the list's capacity a whole walk
of 12 steps can be recorded by ``ctx.capture()``: steps on an empty list do nothing.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Optional

import torch

from . import _capi as capi
from . import trace
from ._capi import check
from .closures import cvec3

WALK_LIB_PATH = capi._PKG / "lib" / "librls_walk.so"

RLS_WALK_TRIALS = 12
RLS_WALK_FOREIGN_STOPS = 0
RLS_WALK_FOREIGN_SKIPS = 1
FOREIGN = {"stop": RLS_WALK_FOREIGN_STOPS, "skip": RLS_WALK_FOREIGN_SKIPS}


class WalkRays_(C.Structure):
    """rls_walk_rays"""
    _fields_ = [("capacity", C.c_int64), ("count", C.c_void_p), ("ray", C.c_void_p), ("origin", capi.Vec3), ("dir", capi.Vec3),
                ("maxdist", C.c_void_p), ("trials", C.c_void_p)]


class WalkFound_(C.Structure):
    """rls_walk_found"""
    _fields_ = [("hit", C.c_void_p), ("t", C.c_void_p), ("P", capi.CVec3), ("N", capi.CVec3), ("Ns", capi.CVec3),
                ("object", C.c_void_p)]


class WalkHits_(C.Structure):
    """rls_walk_hits"""
    _fields_ = [("max_hits", C.c_int), ("stride", C.c_int64), ("count", C.c_void_p), ("P", capi.Vec3), ("N", capi.Vec3)]


class Walk_(C.Structure):
    """rls_walk"""
    _fields_ = [("rays", C.c_int64), ("spp", C.c_int), ("point", C.c_void_p), ("P", capi.CVec3), ("own", C.c_void_p),
                ("foreign", C.c_int), ("hits", WalkHits_), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


_ctx, _i64 = C.c_void_p, C.c_int64
PROTOTYPES = {
    "rls_walk_scratch_bytes": (C.c_int, [_i64, C.POINTER(C.c_size_t)]),
    "rls_walk_begin": (C.c_int, [_ctx, C.POINTER(Walk_), C.POINTER(trace.ProbeQueue_), C.POINTER(WalkRays_)]),
    "rls_walk_step": (C.c_int, [_ctx, C.POINTER(Walk_), C.POINTER(WalkRays_), C.POINTER(WalkFound_), _i64, C.POINTER(WalkRays_)]),
    "rls_walk_active": (C.c_int, [_ctx, C.POINTER(WalkRays_), C.POINTER(C.c_int64)]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once) and prototype the companion library; RLSHADERS_AMD_WALK_LIB overrides its path.  The product and the trace
    library are loaded first (contexts, errors; the queues the walk starts on)."""
    global _lib
    if _lib is None:
        _lib = capi.load_companion("rlshaders_amd.walk", WALK_LIB_PATH, "RLSHADERS_AMD_WALK_LIB", PROTOTYPES, "build_walk_library",
                                   first=(trace.load,))
    return _lib


def scratch_bytes(rays: int) -> int:
    b = C.c_size_t()
    check(load().rls_walk_scratch_bytes(int(rays), C.byref(b)))
    return int(b.value)


# ---- the checks of a caller's tensor, for this module and for the others whose libraries take planes and lists of this one's
def _rows(t: torch.Tensor, n: int, what: str, cls):
    """three planes of >= n floats (a plane of one element has no inner stride to speak of)"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.shape[0] != 3 or \
            t.shape[1] < n or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{what}: expected a float32 CUDA tensor [3, >= {n}] with unit inner stride")
    return cls(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())


def _flat(t: torch.Tensor, n: int, what: str, dtypes) -> int:
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or not t.is_cuda or t.dim() != 1 or t.shape[0] < n or \
            not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous CUDA tensor [>= {n}] of {' or '.join(str(d) for d in dtypes)}")
    return t.data_ptr()


class Found:
    """The renderer's nearest hit of every listed ray (rls_walk_found), indexed like the list a step reads: hit uint8 (or bool),
    t float32 (sg->Rl from the step's origin), P, N, Ns float32 [3, >= active], object int32 ids or None."""

    def __init__(self, hit, t, P, N, Ns, object=None):
        self.hit, self.t, self.P, self.N, self.Ns, self.object = hit, t, P, N, Ns, object

    def struct(self, n: int) -> WalkFound_:
        f = WalkFound_()
        f.hit = _flat(self.hit, n, "found.hit", (torch.uint8, torch.bool))
        f.t = _flat(self.t, n, "found.t", (torch.float32,))
        f.P, f.N, f.Ns = (_rows(t, n, "found." + k, capi.CVec3) for k, t in (("P", self.P), ("N", self.N), ("Ns", self.Ns)))
        f.object = None if self.object is None else _flat(self.object, n, "found.object", (torch.int32,))
        return f


_IDS = (torch.int32, torch.uint32)


def rays_struct(l, cap: int, trials: bool = True) -> WalkRays_:
    """rls_walk_rays over the tensors of l (count, ray, origin, dir, maxdist and, with ``trials``, trials), each checked to hold
    cap entries"""
    s = WalkRays_()
    s.capacity, s.count = cap, _flat(l.count, 1, "list.count", (torch.int64,))
    if cap > 0:
        s.ray = _flat(l.ray, cap, "list.ray", _IDS)
        s.origin, s.dir = _rows(l.origin, cap, "list.origin", capi.Vec3), _rows(l.dir, cap, "list.dir", capi.Vec3)
        s.maxdist = _flat(l.maxdist, cap, "list.maxdist", (torch.float32,))
        if trials:
            s.trials = _flat(l.trials, cap, "list.trials", (torch.uint8,))
    return s


class _List:
    """one active list's device buffers, its struct and the reference a call passes"""

    def __init__(self, alloc, cap: int):
        self.count = alloc((1,), torch.int64)
        self.ray = alloc((cap,), torch.int32)                        # uint32 on the device; rays < 2^31 here
        self.origin = alloc((3, cap), torch.float32)
        self.dir = alloc((3, cap), torch.float32)
        self.maxdist = alloc((cap,), torch.float32)
        self.trials = alloc((cap,), torch.uint8)
        self.s = rays_struct(self, cap)
        self.p = C.byref(self.s)


class ListWalk:
    """What a walk over two lists of rls_walk_rays is, whichever rays it walks: alloc's default, the scratch, the two lists a step
    swaps, and begin / rays / active / step over the three entry points its subclass names.  A subclass allocates what is its
    own through ``_alloc``, fills its struct but for the scratch, and calls ``_start``."""

    @staticmethod
    def _alloc(ctx, alloc):
        if alloc is not None:
            return alloc
        dev = ctx.torch_device
        return lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)

    def _start(self, ctx, w, q, rays: int, need: int, scratch, alloc, begin, step, active):
        """w: the walk's struct, q: its queue's; need: the scratch's bytes; begin, step, active: the library's functions"""
        self.scratch = alloc((need,), torch.uint8) if scratch is None else scratch
        if self.scratch.dtype != torch.uint8 or not self.scratch.is_contiguous() or self.scratch.numel() < need:
            raise ValueError(f"scratch: expected a contiguous uint8 CUDA tensor of >= {need} bytes")
        self.lists = [_List(alloc, rays), _List(alloc, rays)]
        w.scratch, w.scratch_bytes = self.scratch.data_ptr(), self.scratch.numel()
        self.ctx, self.w, self._rays = ctx, w, rays
        self._wp, self._qp, self._begin, self._step, self._active = C.byref(w), C.byref(q), begin, step, active
        self.begin()

    def begin(self):
        """(re)start the walk on the queue as it is now"""
        self.at = 0                                                 # the list the next step reads
        check(self._begin(self.ctx.handle, self._wp, self._qp, self.lists[0].p))
        return self

    @property
    def rays(self) -> SimpleNamespace:
        """the list the next step reads, as tensors of its capacity: entries [0, active) are the active rays; trials: the steps
        left"""
        l = self.lists[self.at]
        return SimpleNamespace(count=l.count, ray=l.ray, origin=l.origin, dir=l.dir, maxdist=l.maxdist, trials=l.trials)

    @property
    def active(self) -> int:
        """the active rays, read from the device (synchronises)"""
        n = C.c_int64()
        check(self._active(self.ctx.handle, self.lists[self.at].p, C.byref(n)))
        return int(n.value)

    def step(self, found, bound: Optional[int] = None):
        """one step over the nearest hits of the listed rays (the module's ``Found``); bound: an upper bound on the active count
        (it sizes the grid and the planes ``found`` must hold), by default the list's capacity"""
        b = self._rays if bound is None else min(int(bound), self._rays)
        check(self._step(self.ctx.handle, self._wp, self.lists[self.at].p, C.byref(found.struct(b)), -1 if bound is None else b,
                         self.lists[self.at ^ 1].p))
        self.at ^= 1
        return self

    def drive(self, tracer, steps: int):
        """to the end, in at most ``steps`` steps: tracer(rays, active) -> Found, the nearest hits of the first ``active`` listed
        rays"""
        for _ in range(steps):
            m = self.active
            if m == 0:
                break
            self.step(tracer(self.rays, m), bound=m)
        return self


class ProbeWalk(ListWalk):
    """The walk of a probe queue's rays (``trace.sss_probe_rays``, or ``trace.skin_node_rays(...).probe``) about the shading
    points P [3, n]: begun on construction.  own: int32 [n], the id of each point's own object, or None for one object everywhere;
    foreign: "stop" (the compiled reference) or "skip" (include/rlshaders_amd_walk.h).  alloc(shape, dtype) -> a contiguous device
    tensor: where the walk's lists and hits come from (torch.empty by default); scratch: a uint8 tensor of scratch_bytes(rays);
    point: int32 [rays], each ray's point (the queue's ``point`` plane) where it is not j // spp_n^2."""

    def __init__(self, ctx, queue, P: torch.Tensor, own: Optional[torch.Tensor] = None, max_hits: int = trace.RLS_MAX_PROBE_HITS,
                 foreign: str = "stop", scratch: Optional[torch.Tensor] = None, alloc=None, point: Optional[torch.Tensor] = None):
        self.queue, self.P, self.own, self.point = queue, P, own, point
        rays = self.count = int(queue.count)
        self.max_hits = int(max_hits)
        alloc = self._alloc(ctx, alloc)
        self.hit_count = alloc((rays,), torch.uint8)
        self.hit_P = alloc((3, self.max_hits, rays), torch.float32)
        self.hit_N = alloc((3, self.max_hits, rays), torch.float32)
        w = Walk_()
        w.rays, w.spp = rays, queue.spp_n * queue.spp_n
        w.point = None if point is None else _flat(point, rays, "point", (torch.int32,))
        w.P = cvec3(P, queue.n, "P") if queue.n > 0 else capi.CVec3(None, None, None)
        w.own = None if own is None else _flat(own, queue.n, "own", (torch.int32,))
        if foreign not in FOREIGN:
            raise ValueError("foreign: 'stop' or 'skip'")
        w.foreign = FOREIGN[foreign]
        w.hits.max_hits, w.hits.stride, w.hits.count = self.max_hits, rays, self.hit_count.data_ptr()
        w.hits.P = capi.Vec3(*[self.hit_P[k].data_ptr() for k in range(3)])
        w.hits.N = capi.Vec3(*[self.hit_N[k].data_ptr() for k in range(3)])
        lib = load()
        self._start(ctx, w, queue.q, rays, scratch_bytes(rays), scratch, alloc, lib.rls_walk_begin, lib.rls_walk_step,
                    lib.rls_walk_active)

    def hits(self, E: Optional[torch.Tensor] = None) -> tuple:
        """(count, P, N, E): the arguments of ``ProbeQueue.resolve`` and of ``trace.sss_hit_rays`` (E: the caller's irradiance
        planes [3, max_hits, rays], passed through)"""
        return self.hit_count, self.hit_P, self.hit_N, E


def run(queue, P: torch.Tensor, tracer, own: Optional[torch.Tensor] = None, max_hits: int = trace.RLS_MAX_PROBE_HITS,
        foreign: str = "stop", ctx=None) -> ProbeWalk:
    """Walk the queue's rays to the end: tracer(rays, active) -> Found, the nearest hits of the first ``active`` listed rays.  At most
    RLS_WALK_TRIALS steps, the walk's trial budget."""
    w = ProbeWalk(queue.ctx if ctx is None else ctx, queue, P, own=own, max_hits=max_hits, foreign=foreign)
    return w.drive(tracer, RLS_WALK_TRIALS)
