"""helpers of the shadow walk's CPU tests (test_shadow_walk_abi.py, test_cmake_shadow_walk.py): what
include/rlshaders_amd_shadow_walk.h declares and librls_shadow_walk.so exports, and valid arguments over dummy memory for the
refusal table, after trace_abi_util.Dummies.  pytest does not collect this module."""
import re

import pytest

from trace_abi_util import ROOT, code_text, dynamic_symbols
from walk_abi_util import ListWalkWorld

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


class ShadowWalkWorld(ListWalkWorld):
    """a valid walk of 192 rays (the capacity of a node's light loop over 8 points, 2 lights, spp_n = 2) over dummy memory: the
    walk, the queue, two lists, the found hits"""

    def __init__(self):
        from rlshaders_amd import shadow_walk
        super().__init__(shadow_walk.load(), "rls_shadow_walk")
        capi, q, w = self.capi, self.shadow_queue(3), shadow_walk.ShadowWalk_()
        q.point = self.p
        rays = self.rays = q.capacity
        w.rays, w.count, w.max_steps, w.O = rays, self.p, 8, self.v3(capi.CVec3)
        w.visibility = self.v3(capi.Rgb)
        w.scratch, w.scratch_bytes = self.p, self._scratch(self.wlib.rls_shadow_walk_scratch_bytes, rays)
        self.over(w, q, shadow_walk.ShadowWalkFound_(self.p, self.p, self.v3(capi.CVec3), self.v3(capi.CRgb), None, 0))
