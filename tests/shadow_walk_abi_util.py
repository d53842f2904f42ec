"""helpers of the shadow walk's CPU tests (test_shadow_walk_abi.py, test_cmake_shadow_walk.py): what
include/rlshaders_amd_shadow_walk.h declares and librls_shadow_walk.so exports, and valid arguments over dummy memory for the
refusal table, after trace_abi_util.Dummies.  pytest does not collect this module."""
import ctypes as C
import re

import pytest

from trace_abi_util import ROOT, Dummies, code_text, dynamic_symbols

HEADER = ROOT / "include" / "rlshaders_amd_shadow_walk.h"


@pytest.fixture(scope="module")
def shadow_walk_lib():
    from rlshaders_amd import build
    build.build_trace_library()
    return build.build_shadow_walk_library()


def declared_symbols():
    return sorted(set(re.findall(r"\b(rls_[a-z0-9_]+)\s*\(", code_text(HEADER))))


def declarations():
    """entry point -> its parameter list"""
    return {m.group(1): m.group(2)
            for m in re.finditer(r"rls_status\s+(rls_shadow_walk_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code_text(HEADER), flags=re.S)}


def exported_symbols(lib):
    return sorted(l.split()[-1] for l in dynamic_symbols(lib).splitlines() if l.split() and l.split()[-1].startswith("rls_"))


def structs():
    return re.findall(r"typedef struct (\w+)\s*\{", code_text(HEADER))


def struct_members(c_name):
    """the members of a struct of the header, in order (it has no array member)"""
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (c_name, c_name), code_text(HEADER), flags=re.S).group(1)
    return [re.search(r"(\w+)\s*$", part.strip()).group(1) for d in body.split(";") if d.strip() for part in d.split(",")]


class ShadowWalkWorld(Dummies):
    """a valid walk of 192 rays (the capacity of a node's light loop over 8 points, 2 lights, spp_n = 2) over dummy memory: the
    walk, the queue, two lists, the found hits"""

    def __init__(self):
        super().__init__()
        from rlshaders_amd import shadow_walk
        capi = self.capi
        self.sw, self.wlib = shadow_walk, shadow_walk.load()
        self.q = self.shadow_queue(3)
        self.q.point = self.p
        rays = self.rays = self.q.capacity
        self.w = shadow_walk.ShadowWalk_()
        self.w.rays, self.w.count, self.w.max_steps, self.w.O = rays, self.p, 8, self.v3(capi.CVec3)
        self.w.visibility = self.v3(capi.Rgb)
        self.w.scratch, self.w.scratch_bytes = self.p, self._scratch(self.wlib.rls_shadow_walk_scratch_bytes, rays)
        self.lists = [self.list_at(0), self.list_at(4096)]
        self.f = shadow_walk.ShadowWalkFound_(self.p, self.p, self.v3(capi.CVec3), self.v3(capi.CRgb), None, 0)
        self.wp, self.qp, self.fp = C.byref(self.w), C.byref(self.q), C.byref(self.f)
        self.inp, self.outp = C.byref(self.lists[0]), C.byref(self.lists[1])
        self.bound = -1
        self.host = C.c_int64()
        self.hostp = C.byref(self.host)

    def list_at(self, off):
        """a list whose planes start `off` bytes into the dummy block (two lists must not share planes)"""
        capi, l, p = self.capi, self.sw.WalkRays_(), self.p + off
        l.capacity, l.count, l.ray, l.maxdist, l.trials = self.rays, p, p, p, p
        l.origin, l.dir = capi.Vec3(p, p, p), capi.Vec3(p, p, p)
        return l

    def begin(self):
        return self.wlib.rls_shadow_walk_begin(self.ctxp, self.wp, self.qp, self.outp)

    def step(self):
        return self.wlib.rls_shadow_walk_step(self.ctxp, self.wp, self.inp, self.fp, self.bound, self.outp)

    def active(self):
        return self.wlib.rls_shadow_walk_active(self.ctxp, self.inp, self.hostp)
