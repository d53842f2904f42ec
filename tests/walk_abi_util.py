"""helpers of the probe walk's CPU tests (test_walk_abi.py, test_cmake_walk.py): what include/rlshaders_amd_walk.h declares and
librls_walk.so exports, and valid arguments over dummy memory for the refusal table, after trace_abi_util.Dummies; and what
the shadow walk's tests share with them (shadow_walk_abi_util.py, test_shadow_walk_abi.py): the world of a walk over two lists
and the refusal rows of the list checks.  pytest does not collect this module."""
import ctypes as C
import re

import pytest

from trace_abi_util import ROOT, Dummies, code_text, dynamic_symbols, put

HEADER = ROOT / "include" / "rlshaders_amd_walk.h"


@pytest.fixture(scope="module")
def walk_lib():
    from rlshaders_amd import build
    build.build_trace_library()
    return build.build_walk_library()


def declared_walk_symbols():
    return sorted(set(re.findall(r"\b(rls_[a-z0-9_]+)\s*\(", code_text(HEADER))))


def walk_declarations():
    """entry point -> its parameter list"""
    return {m.group(1): m.group(2)
            for m in re.finditer(r"rls_status\s+(rls_walk_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code_text(HEADER), flags=re.S)}


def exported_walk_symbols(lib):
    return sorted(l.split()[-1] for l in dynamic_symbols(lib).splitlines() if l.split() and l.split()[-1].startswith("rls_"))


def walk_structs():
    return re.findall(r"typedef struct (\w+)\s*\{", code_text(HEADER))


def walk_struct_members(c_name):
    """the members of a struct of the walk's header, in order (it has no array member)"""
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (c_name, c_name), code_text(HEADER), flags=re.S).group(1)
    return [re.search(r"(\w+)\s*$", part.strip()).group(1) for d in body.split(";") if d.strip() for part in d.split(",")]


class ListWalkWorld(Dummies):
    """what the worlds of the two walks share: two lists over dummy memory, the pointers a call passes, and begin / step / active
    over the entry points <prefix>_begin, _step, _active of the walk's library"""

    def __init__(self, wlib, prefix):
        super().__init__()
        from rlshaders_amd import walk
        self.walk, self.wlib = walk, wlib
        self.entries = {verb: getattr(wlib, f"{prefix}_{verb}") for verb in ("begin", "step", "active")}
        self.bound = -1
        self.host = C.c_int64()
        self.hostp = C.byref(self.host)

    def over(self, w, q, f):
        """the walk, its queue, the found hits; two lists of w.rays"""
        self.w, self.q, self.f = w, q, f
        self.lists = [self.list_at(0), self.list_at(4096)]
        self.wp, self.qp, self.fp = C.byref(w), C.byref(q), C.byref(f)
        self.inp, self.outp = C.byref(self.lists[0]), C.byref(self.lists[1])

    def list_at(self, off):
        """a list whose planes start `off` bytes into the dummy block (two lists must not share planes)"""
        capi, l, p = self.capi, self.walk.WalkRays_(), self.p + off
        l.capacity, l.count, l.ray, l.maxdist, l.trials = self.w.rays, p, p, p, p
        l.origin, l.dir = capi.Vec3(p, p, p), capi.Vec3(p, p, p)
        return l

    def begin(self):
        return self.entries["begin"](self.ctxp, self.wp, self.qp, self.outp)

    def step(self):
        return self.entries["step"](self.ctxp, self.wp, self.inp, self.fp, self.bound, self.outp)

    def active(self):
        return self.entries["active"](self.ctxp, self.inp, self.hostp)


# ---- the refusals both walks' libraries state in one header (csrc_walk/rls_walk_list.hpp): each suite adds its own rows
_PLANES = "%s.ray, %s.origin, %s.dir, %s.maxdist or %s.trials plane is NULL"
LIST_OUT = [
    ("out NULL", lambda w: put(w, "outp", None), "out is NULL"),
    ("out.count NULL", lambda w: put(w.lists[1], "count", None), "out.count is NULL"),
    ("out.capacity short", lambda w: put(w.lists[1], "capacity", w.w.rays - 1), "out.capacity < walk.rays"),
    ("out.trials NULL", lambda w: put(w.lists[1], "trials", None), _PLANES.replace("%s", "out")),
    ("out.dir NULL", lambda w: put(w.lists[1], "dir", w.half3(w.capi.Vec3)), _PLANES.replace("%s", "out")),
]
LIST_IN = [
    ("in NULL", lambda w: put(w, "inp", None), "in is NULL"),
    ("in.count NULL", lambda w: put(w.lists[0], "count", None), "in.count is NULL"),
    ("in.capacity short", lambda w: put(w.lists[0], "capacity", w.w.rays - 1), "in.capacity < walk.rays"),
    ("in.ray NULL", lambda w: put(w.lists[0], "ray", None), _PLANES.replace("%s", "in")),
    ("out is in", lambda w: put(w, "outp", w.inp), "out is in: a step reads one list and writes the other"),
]
ACTIVE = [
    ("ctx NULL", lambda w: put(w, "ctxp", None), "ctx is NULL"),
    ("rays NULL", lambda w: put(w, "inp", None), "rays or rays.count is NULL"),
    ("rays.count NULL", lambda w: put(w.lists[0], "count", None), "rays or rays.count is NULL"),
    ("host_count NULL", lambda w: put(w, "hostp", None), "host_count is NULL"),
]


class WalkWorld(ListWalkWorld):
    """a valid walk of 32 rays (8 points at spp_n = 2) over dummy memory: the walk, the queue, two lists, the found hits"""

    def __init__(self):
        from rlshaders_amd import walk
        super().__init__(walk.load(), "rls_walk")
        capi, rays, w = self.capi, self.n * 4, walk.Walk_()
        w.rays, w.spp, w.P, w.foreign = rays, 4, self.v3(capi.CVec3), 0
        w.hits.max_hits, w.hits.stride, w.hits.count = 12, rays, self.p
        w.hits.P, w.hits.N = self.v3(capi.Vec3), self.v3(capi.Vec3)
        w.scratch, w.scratch_bytes = self.p, self._scratch(self.wlib.rls_walk_scratch_bytes, rays)
        self.over(w, self.probe_queue(),
                  walk.WalkFound_(self.p, self.p, self.v3(capi.CVec3), self.v3(capi.CVec3), self.v3(capi.CVec3), None))
