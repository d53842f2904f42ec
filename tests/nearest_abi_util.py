"""helpers of the nearest-hit library's CPU tests (test_nearest_abi.py, test_cmake_nearest.py): what
include/rlshaders_amd_nearest.h declares and librls_nearest.so exports, and valid arguments over dummy memory for the refusal
table, after trace_abi_util.Dummies.  pytest does not collect this module."""
import ctypes as C
import re

import numpy as np
import pytest

from trace_abi_util import ROOT, Dummies, code_text, dynamic_symbols

HEADER = ROOT / "include" / "rlshaders_amd_nearest.h"


@pytest.fixture(scope="module")
def nearest_lib():
    from rlshaders_amd import build
    return build.build_nearest_library()


def declared_symbols():
    return sorted(set(re.findall(r"\b(rls_[a-z0-9_]+)\s*\(", code_text(HEADER))))


def declarations():
    """entry point -> its parameter list"""
    return {m.group(1): m.group(2)
            for m in re.finditer(r"rls_status\s+(rls_nearest_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code_text(HEADER), flags=re.S)}


def exported_symbols(lib):
    return sorted(l.split()[-1] for l in dynamic_symbols(lib).splitlines() if l.split() and l.split()[-1].startswith("rls_"))


def structs():
    return re.findall(r"typedef struct (\w+)\s*\{", code_text(HEADER))


def struct_members(c_name):
    """the members of a struct of the header, in order (it has no array member)"""
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (c_name, c_name), code_text(HEADER), flags=re.S).group(1)
    return [re.search(r"(\w+)\s*$", part.strip()).group(1) for d in body.split(";") if d.strip() for part in d.split(",")]


class NearestWorld(Dummies):
    """valid arguments of every entry point over dummy memory: a mesh of one triangle (host memory, really read), 192 rays, a
    list of 192 entries, every found plane set; the scene pointer is dummy memory too (a refused call does not read it)"""

    def __init__(self):
        super().__init__()
        from rlshaders_amd import nearest
        capi = self.capi
        self.nearest, self.nlib = nearest, nearest.load()
        self.V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
        self.T = np.array([[0, 1, 2]], np.uint32)
        self.mesh = nearest.NearestMesh_(3, 1, self.V.ctypes.data, self.T.ctypes.data, None, None, 0)
        self.rays = 192
        p = self.p
        self.r = nearest.NearestRays_(self.rays, p, self.v3(capi.CVec3), None, self.v3(capi.CVec3), p, None)
        self.f = nearest.NearestFound_(p, p, *[self.v3(capi.Vec3) for _ in range(5)], p, p, p, p, p, p, 4, p)
        self.list = nearest.WalkRays_(self.rays, p, p, self.v3(capi.Vec3), self.v3(capi.Vec3), p, p)
        self.scene = C.c_void_p()
        self.meshp, self.outp = C.byref(self.mesh), C.byref(self.scene)
        self.scenep, self.rp, self.fp, self.listp = p, C.byref(self.r), C.byref(self.f), C.byref(self.list)
        self.bound = -1
        self.info = nearest.NearestSceneInfo_()
        self.infop = C.byref(self.info)

    def create(self):
        return self.nlib.rls_nearest_scene_create(self.ctxp, self.meshp, self.outp)

    def hits(self):
        return self.nlib.rls_nearest_hits(self.ctxp, self.scenep, self.rp, self.fp)

    def walk_hits(self):
        return self.nlib.rls_nearest_walk_hits(self.ctxp, self.scenep, self.listp, self.bound, self.fp)

    def get_info(self):
        return self.nlib.rls_nearest_scene_get_info(self.scenep, self.infop)
