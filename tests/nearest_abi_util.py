"""helpers of the nearest-hit libraries' CPU tests (test_nearest_abi.py, test_nearest_refit_abi.py, test_nearest_rebuild_abi.py,
test_cmake_nearest*.py): what a header declares and its library exports, written once for the three headers; valid arguments
over dummy memory for the refusal tables, after trace_abi_util.Dummies; and, written once for the two moving-mesh libraries
(nearest_refit_util.py and nearest_rebuild_util.py bind them to a noun), their world, their refusal tables and the compiled probe
of their structs.  pytest does not collect this module."""
import ctypes as C
import importlib
import re
import subprocess

import numpy as np
import pytest

from trace_abi_util import ROOT, Dummies, code_text, dynamic_symbols, put

HEADER = ROOT / "include" / "rlshaders_amd_nearest.h"
SCENE_HEADER = ROOT / "rlshaders_amd" / "csrc_nearest" / "rls_nearest_scene.hpp"
UPDATE_LAYER = ROOT / "rlshaders_amd" / "csrc_nearest" / "rls_nearest_update.hpp"   # the two moving-mesh units' shared host layer


@pytest.fixture(scope="module")
def nearest_lib():
    from rlshaders_amd import build
    return build.build_nearest_library()


def exported_symbols(lib):
    return sorted(l.split()[-1] for l in dynamic_symbols(lib).splitlines() if l.split() and l.split()[-1].startswith("rls_"))


def header_abi(header, prefix):
    """-> declared_symbols, declarations, structs, struct_members of a header whose entry points start with `prefix`"""
    def declared_symbols():
        return sorted(set(re.findall(r"\b(rls_[a-z0-9_]+)\s*\(", code_text(header))))

    def declarations():
        """entry point -> its parameter list"""
        return {m.group(1): m.group(2)
                for m in re.finditer(r"rls_status\s+(%s[a-z0-9_]+)\s*\(([^;]*?)\)\s*;" % prefix, code_text(header), flags=re.S)}

    def structs():
        return re.findall(r"typedef struct (\w+)\s*\{", code_text(header))

    def struct_members(c_name):
        """the members of a struct of the header, in order (it has no array member)"""
        body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (c_name, c_name), code_text(header), flags=re.S).group(1)
        return [re.search(r"(\w+)\s*$", part.strip()).group(1) for d in body.split(";") if d.strip() for part in d.split(",")]

    return declared_symbols, declarations, structs, struct_members


declared_symbols, declarations, structs, struct_members = header_abi(HEADER, "rls_nearest_")


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


# ---- the two moving-mesh libraries: NOUN is "refit" or "rebuild" ---------------------------------------------------------------------
def scene_layout_tag():
    """kNearestSceneLayout, from the private header"""
    return int(re.search(r"kNearestSceneLayout\s*=\s*(0x[0-9a-fA-F]+)ull", SCENE_HEADER.read_text()).group(1), 16)


class MovingWorld(Dummies):
    """valid arguments of every entry point of rlshaders_amd.nearest_<NOUN> over dummy memory.  The scene is 4 KiB that start with
    this build's layout tag and device 0 (the dummy context's); the handle is 4 KiB that start with a public info struct of 3
    vertices with normals and device 0 -- the two structs lead with just these members (csrc_nearest/rls_nearest_scene.hpp, the
    library's unit), so every check is reached; a refused call reads nothing else."""
    NOUN = None

    def __init__(self):
        super().__init__()
        self.mod = importlib.import_module("rlshaders_amd.nearest_" + self.NOUN)
        self.rlib, cls = self.mod.load(), getattr(self.mod, self.NOUN.capitalize())
        self.scene = C.create_string_buffer(4096)
        C.c_uint64.from_buffer(self.scene, 0).value = scene_layout_tag()
        self.handle = C.create_string_buffer(4096)
        self.handle_info = cls.Info.from_buffer(self.handle, 0)
        self.handle_info.nv, self.handle_info.nt, self.handle_info.has_normals = 3, 1, 1
        self.mesh = cls.Mesh(3, self.p, self.p, self.p)
        self.out = C.c_void_p()
        self.info = cls.Info()
        self.scenep, self.handlep = C.addressof(self.scene), C.addressof(self.handle)
        self.meshp, self.outp, self.infop = C.byref(self.mesh), C.byref(self.out), C.byref(self.info)

    def scene_device(self, device):
        C.c_int.from_buffer(self.scene, 8).value = device

    def handle_device(self, device):
        C.c_int.from_buffer(self.handle, C.sizeof(self.info)).value = device

    def entry(self, verb):
        return getattr(self.rlib, f"rls_nearest_{self.NOUN}_{verb}")

    def create(self):
        return self.entry("create")(self.ctxp, self.scenep, self.outp)

    def update(self):
        return self.entry("update")(self.ctxp, self.handlep, self.meshp)

    def get_info(self):
        return self.entry("get_info")(self.handlep, self.infop)

    def read_tree(self):
        return self.entry("read_tree")(self.ctxp, self.handlep, self.p, self.p, self.p)


def refusal_tables(noun):
    """-> the rows (what, edit of a MovingWorld, text) of every argument check, by verb"""
    layout = f"scene is not a scene of this build's layout (librls_nearest.so and librls_nearest_{noun}.so must be of one build)"
    ctx = ("ctx NULL", lambda w: put(w, "ctxp", None), "ctx is NULL")
    handle = (f"{noun} NULL", lambda w: put(w, "handlep", None), f"{noun} is NULL")
    device = ("another device", lambda w: w.handle_device(1), f"the {noun}'s scene lives on another device than ctx")
    return dict(
        create=[
            ctx,
            ("out NULL", lambda w: put(w, "outp", None), "out is NULL"),
            ("scene NULL", lambda w: put(w, "scenep", None), "scene is NULL"),
            ("a zeroed scene", lambda w: put(w, "scenep", w.p), layout),
            ("another layout", lambda w: C.c_uint64.from_buffer(w.scene, 0).__setattr__("value", scene_layout_tag() - 1), layout),
            ("another device", lambda w: w.scene_device(1), "the scene lives on another device than ctx"),
        ],
        update=[
            ctx,
            handle,
            ("mesh NULL", lambda w: put(w, "meshp", None), "mesh is NULL"),
            ("nv more", lambda w: put(w.mesh, "nv", 4), "mesh.nv is not the scene's"),
            ("nv less", lambda w: put(w.mesh, "nv", 2), "mesh.nv is not the scene's"),
            ("vertices NULL", lambda w: put(w.mesh, "vertices", None), "mesh.vertices is NULL"),
            ("normals without", lambda w: put(w.handle_info, "has_normals", 0), "mesh.normals is set but the scene was made without normals"),
            device,
        ],
        get_info=[handle, ("info NULL", lambda w: put(w, "infop", None), "info is NULL")],
        read_tree=[ctx, handle, device])


def compiled_layout(tmp, header, structs, struct_members):
    """what the C compiler says: sizeof of every struct of the header, offsetof of every member"""
    lines = []
    for c_name in structs():
        lines.append(f'  printf("sizeof {c_name} %zu\\n", sizeof({c_name}));')
        lines += [f'  printf("{c_name}.{m} %zu\\n", offsetof({c_name}, {m}));' for m in struct_members(c_name)]
    src, exe = tmp / "probe.c", tmp / "probe"
    src.write_text("\n".join(['#include <stddef.h>', '#include <stdio.h>', f'#include "{header.name}"',
                              'int main(void) {', *lines, '  return 0; }']) + "\n")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{header.parent}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out = [l for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if l]
    assert len(out) == len(lines)
    return {k: int(v) for k, v in (l.rsplit(" ", 1) for l in out)}


def host_layer(unit):
    """-> (the text of a moving-mesh unit together with the shared host layer it includes, the messages of their argument checks)"""
    text = unit.read_text() + UPDATE_LAYER.read_text()
    return text, re.findall(r'RLS_REQUIRE(?:_IN)?\([^;]*?"([^"]+)"\s*\)\s*;', text, flags=re.S)
