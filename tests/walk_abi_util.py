"""helpers of the probe walk's CPU tests (test_walk_abi.py, test_cmake_walk.py): what include/rlshaders_amd_walk.h declares and
librls_walk.so exports, and valid arguments over dummy memory for the refusal table, after trace_abi_util.Dummies.  pytest does
not collect this module."""
import ctypes as C
import re

import pytest

from trace_abi_util import ROOT, Dummies, code_text, dynamic_symbols

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


class WalkWorld(Dummies):
    """a valid walk of 32 rays (8 points at spp_n = 2) over dummy memory: the walk, the queue, two lists, the found hits"""

    def __init__(self):
        super().__init__()
        from rlshaders_amd import walk
        capi = self.capi
        self.walk, self.wlib = walk, walk.load()
        rays = self.n * 4
        self.w = walk.Walk_()
        self.w.rays, self.w.spp, self.w.P, self.w.foreign = rays, 4, self.v3(capi.CVec3), 0
        self.w.hits.max_hits, self.w.hits.stride, self.w.hits.count = 12, rays, self.p
        self.w.hits.P, self.w.hits.N = self.v3(capi.Vec3), self.v3(capi.Vec3)
        self.w.scratch, self.w.scratch_bytes = self.p, self._scratch(self.wlib.rls_walk_scratch_bytes, rays)
        self.q = self.probe_queue()
        self.lists = [self.list_at(0), self.list_at(4096)]
        self.f = walk.WalkFound_(self.p, self.p, self.v3(capi.CVec3), self.v3(capi.CVec3), self.v3(capi.CVec3), None)
        self.wp, self.qp, self.fp = C.byref(self.w), C.byref(self.q), C.byref(self.f)
        self.inp, self.outp = C.byref(self.lists[0]), C.byref(self.lists[1])
        self.bound = -1
        self.host = C.c_int64()
        self.hostp = C.byref(self.host)

    def list_at(self, off):
        """a list whose planes start `off` bytes into the dummy block (two lists must not share planes)"""
        capi, l, p = self.capi, self.walk.WalkRays_(), self.p + off
        l.capacity, l.count, l.ray, l.maxdist, l.trials = self.n * 4, p, p, p, p
        l.origin, l.dir = capi.Vec3(p, p, p), capi.Vec3(p, p, p)
        return l

    def begin(self):
        return self.wlib.rls_walk_begin(self.ctxp, self.wp, self.qp, self.outp)

    def step(self):
        return self.wlib.rls_walk_step(self.ctxp, self.wp, self.inp, self.fp, self.bound, self.outp)

    def active(self):
        return self.wlib.rls_walk_active(self.ctxp, self.inp, self.hostp)
