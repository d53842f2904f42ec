"""CPU: the ABI of the nearest-hit companion library (include/rlshaders_amd_nearest.h, librls_nearest.so,
rlshaders_amd/nearest.py).

The header declares, the library exports and nearest.PROTOTYPES binds the same entry points with the same arity; every
ctypes.Structure of nearest.py mirrors one struct of the header in member order, sizeof and every offsetof (from a compiled
probe), and the walks' list is the probe walk's mirror of rls_walk_rays; the header is C99 / C++14 clean; the library holds ONE
gfx950 code object with one kernel that uses no scratch memory, links the product library by $ORIGIN and no other companion, and
none of the other libraries knows an rls_nearest_ name; every argument check refuses
with "<entry>: <text>" over dummy memory (no device needed)."""
import ctypes as C
import inspect
import re
import subprocess

import pytest

from nearest_abi_util import (HEADER, NearestWorld, declarations, declared_symbols, exported_symbols, nearest_lib,  # noqa: F401
                              struct_members, structs)
from trace_abi_util import INVALID, ROOT, dynamic_symbols, put, refusals

ARITY = dict(rls_nearest_scene_create=3, rls_nearest_scene_destroy=1, rls_nearest_scene_get_info=2, rls_nearest_hits=4,
             rls_nearest_walk_hits=5)
CONSTANTS = ("RLS_NEAREST_STACK", "RLS_NEAREST_MAX_TRIANGLES", "RLS_NEAREST_MAX_LEAF", "RLS_NEAREST_DEFAULT_LEAF", "RLS_NEAREST_NO_PRIM")
STRUCTS = ["rls_nearest_found", "rls_nearest_mesh", "rls_nearest_rays", "rls_nearest_scene_info"]
HIP = ROOT / "rlshaders_amd" / "csrc_nearest" / "nearest.hip"


def mirrors():
    from rlshaders_amd import nearest
    classes = [c for _, c in inspect.getmembers(nearest, inspect.isclass)
               if issubclass(c, C.Structure) and c.__module__ == nearest.__name__]
    assert len({c.__doc__ for c in classes}) == len(classes)
    return {c.__doc__: c for c in classes}


def _compile_and_run(tmp_path, lines):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(['#include <stddef.h>', '#include <stdio.h>', '#include "rlshaders_amd_nearest.h"',
                              'int main(void) {', *lines, '  return 0; }']) + "\n")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return [l for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if l]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """what the C compiler says: sizeof of every struct of the header, offsetof of every member, the value of every constant"""
    lines = [f'  printf("{name} %lld\\n", (long long)({name}));' for name in CONSTANTS]
    for c_name in structs():
        lines.append(f'  printf("sizeof {c_name} %zu\\n", sizeof({c_name}));')
        lines += [f'  printf("{c_name}.{m} %zu\\n", offsetof({c_name}, {m}));' for m in struct_members(c_name)]
    out = _compile_and_run(tmp_path_factory.mktemp("probe"), lines)
    assert len(out) == len(lines)
    return {k: int(v) for k, v in (l.rsplit(" ", 1) for l in out)}


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_exports_exactly_the_header_and_the_bindings(nearest_lib):
    from rlshaders_amd import nearest
    declared, decl = declared_symbols(), declarations()
    assert declared and all(s.startswith("rls_nearest_") for s in declared), declared
    assert exported_symbols(nearest_lib) == declared
    assert sorted(nearest.PROTOTYPES) == declared == sorted(decl) == sorted(ARITY)
    lib, out = nearest.load(), dynamic_symbols(nearest_lib)
    for name, n in ARITY.items():
        assert len(decl[name].split(",")) == n, (name, decl[name])
        assert f" T {name}\n" in out, name
        restype, argtypes = nearest.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == n and getattr(lib, name).argtypes == argtypes, name
    for cls, methods in dict(Scene=("hits", "close"), Found=("struct", "walk_found", "shadow_found", "bins", "gatherable"),
                             Rays=("struct",), tracer=("__call__",)).items():
        assert all(callable(getattr(getattr(nearest, cls), m)) for m in methods), cls
    sig = inspect.signature(nearest.Scene.__init__)
    assert list(sig.parameters) == ["self", "ctx", "vertices", "triangles", "surface", "normals", "leaf_size"]
    assert list(inspect.signature(nearest.Scene.hits).parameters)[:4] == ["self", "rays", "active", "last"]


def test_other_libraries_know_nothing_of_the_nearest_hit(nearest_lib):
    from rlshaders_amd import _capi, build, shadow_walk, trace, walk
    build.build_trace_library(), build.build_walk_library(), build.build_shadow_walk_library()
    for lib in (build.LIB, build.TRACE_LIB, build.WALK_LIB, build.SHADOW_WALK_LIB, build.RR_LIB):
        assert "rls_nearest_" not in dynamic_symbols(lib), lib
        assert b"rls_nearest_" not in lib.read_bytes(), lib
    assert not [s for s in list(_capi.PROTOTYPES) + list(trace.PROTOTYPES) + list(walk.PROTOTYPES) + list(shadow_walk.PROTOTYPES)
                if s.startswith("rls_nearest_")]
    for h in ("rlshaders_amd.h", "rlshaders_amd_trace.h", "rlshaders_amd_walk.h", "rlshaders_amd_shadow_walk.h"):
        text = (ROOT / "include" / h).read_text()
        assert "rlshaders_amd_nearest.h" not in text and "rls_nearest_" not in text, h
    for m in ("trace.py", "walk.py", "shadow_walk.py"):
        text = (ROOT / "rlshaders_amd" / m).read_text()
        assert "rls_nearest" not in text and "import nearest" not in text and "librls_nearest" not in text, m


# ---- structs and constants: nearest.py against the compiler ------------------------------------------------------------------------
def test_every_struct_mirror_has_the_headers_layout(probe):
    from rlshaders_amd import nearest, walk
    assert sorted(mirrors()) == sorted(structs()) == STRUCTS
    for c_name, cls in mirrors().items():
        assert [f[0] for f in cls._fields_] == struct_members(c_name), c_name
        assert C.sizeof(cls) == probe[f"sizeof {c_name}"], c_name
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == probe[f"{c_name}.{f}"], (c_name, f)
    # the walks' list is the probe walk's type, in C (the header includes rlshaders_amd_walk.h) and in Python
    assert nearest.WalkRays_ is walk.WalkRays_ and '#include "rlshaders_amd_walk.h"' in HEADER.read_text()
    assert "rls_walk_rays" not in structs()
    for name in CONSTANTS:
        assert getattr(nearest, name) == probe[name], name
    assert probe["RLS_NEAREST_STACK"] == 24 and probe["RLS_NEAREST_MAX_TRIANGLES"] == 1 << 22


# ---- the header ----------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_cxx(tmp_path):
    body = ("rls_nearest_mesh m = {0}; rls_nearest_rays r = {0}; rls_nearest_found f = {0}; rls_walk_rays l = {0}; "
            "rls_nearest_scene *s = 0; rls_nearest_scene_info i = {0}; m.leaf_size = RLS_NEAREST_DEFAULT_LEAF; "
            "return (int)rls_nearest_scene_create(0, &m, &s) + (int)rls_nearest_hits(0, s, &r, &f) + "
            "(int)rls_nearest_walk_hits(0, s, &l, -1, &f) + (int)rls_nearest_scene_get_info(s, &i) + "
            "(int)rls_nearest_scene_destroy(s);")
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_nearest.h"\nint main(void){ ' + body + ' }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-Wno-missing-field-initializers", "-Wno-missing-braces",
                            "-fsyntax-only", f"-I{ROOT / 'include'}", "-x", "c" if cc == "gcc" else "c++", str(src)],
                           capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)
    text = HEADER.read_text()
    assert "THE STATEMENT" in text and "never by an epsilon" in text and "RLS_NEAREST_MAX_TRIANGLES" in text


# ---- the device code -----------------------------------------------------------------------------------------------------------
def test_one_gfx950_code_object_one_kernel_no_scratch(nearest_lib, tmp_path):
    from rlshaders_amd import build
    from rlshaders_amd.codeid import code_objects, fatbin, kernel_digests
    objs = code_objects(fatbin(nearest_lib))
    assert len(objs) == 1 and b"gfx950" in objs[0]
    kernels = list(kernel_digests(objs[0]))
    assert len(kernels) == 1 and "nearest_kernel" in kernels[0], kernels
    d = subprocess.run(["readelf", "-d", str(nearest_lib)], capture_output=True, text=True, check=True).stdout
    assert "[librlshaders_amd.so]" in d and "$ORIGIN" in d
    assert "librls_trace" not in d and "librls_walk" not in d and "librls_shadow_walk" not in d
    for lib in (build.LIB, build.TRACE_LIB, build.build_walk_library(), build.build_shadow_walk_library()):
        for elf in code_objects(fatbin(lib)):
            assert b"nearest_kernel" not in elf, lib
    # the traversal stack lives in LDS: the kernel's metadata reports no private (scratch) segment and no spilled vector register
    (tmp_path / "nearest.co").write_bytes(objs[0])
    note = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(tmp_path / "nearest.co")], capture_output=True,
                          text=True, check=True).stdout
    assert re.search(r"\.private_segment_fixed_size:\s*0\b", note) and re.search(r"\.vgpr_spill_count:\s*0\b", note), note[-2000:]
    lds = int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", note).group(1))
    assert lds == 24 * 256 * 4                                       # RLS_NEAREST_STACK words a lane


# ---- the refusals: no device needed ------------------------------------------------------------------------------------------------
def _mesh(w, **kw):
    for k, v in kw.items():
        setattr(w.mesh, k, v)


CREATE = [
    ("ctx NULL", lambda w: put(w, "ctxp", None), "ctx is NULL"),
    ("out NULL", lambda w: put(w, "outp", None), "out is NULL"),
    ("mesh NULL", lambda w: put(w, "meshp", None), "mesh is NULL"),
    ("nt < 0", lambda w: _mesh(w, nt=-1), "mesh.nv or mesh.nt < 0"),
    ("nv 2^32", lambda w: _mesh(w, nv=1 << 32), "mesh.nv > 2^32 - 1 (a vertex index is 32-bit)"),
    ("nt past the limit", lambda w: _mesh(w, nt=(1 << 22) + 1),
     "mesh.nt > 2^22: the traversal stack of 24 entries bounds the tree's depth"),
    ("leaf 9", lambda w: _mesh(w, leaf_size=9), "mesh.leaf_size must be in [1, 8], or 0 for the default"),
    ("leaf -1", lambda w: _mesh(w, leaf_size=-1), "mesh.leaf_size must be in [1, 8], or 0 for the default"),
    ("vertices NULL", lambda w: _mesh(w, vertices=None), "mesh.vertices is NULL"),
    ("triangles NULL", lambda w: _mesh(w, triangles=None), "mesh.triangles is NULL"),
    ("index past nv", lambda w: w.T.__setitem__((0, 2), 3), "mesh.triangles holds an index >= mesh.nv"),
    ("NaN vertex", lambda w: w.V.__setitem__((1, 1), float("nan")), "mesh.vertices holds a NaN or an inf"),
    ("inf vertex", lambda w: w.V.__setitem__((2, 0), float("-inf")), "mesh.vertices holds a NaN or an inf"),
]
FOUND = [
    ("found NULL", lambda w: put(w, "fp", None), "found is NULL"),
    ("found.hit NULL", lambda w: put(w.f, "hit", None), "found.hit or found.t plane is NULL"),
    ("found.t NULL", lambda w: put(w.f, "t", None), "found.hit or found.t plane is NULL"),
    ("found.N half", lambda w: put(w.f, "N", w.half3(w.capi.Vec3)), "found.P, N, Ns, T or wo is partly NULL: all three planes or none"),
    ("found.wo half", lambda w: put(w.f, "wo", w.half3(w.capi.Vec3)), "found.P, N, Ns, T or wo is partly NULL: all three planes or none"),
    ("bin without table", lambda w: put(w.f, "bin_of_surface", None),
     "found.bin is set with found.bin_of_surface NULL or found.bin_count == 0"),
    ("bin, empty table", lambda w: put(w.f, "bin_count", 0), "found.bin is set with found.bin_of_surface NULL or found.bin_count == 0"),
]
HITS = [
    ("ctx NULL", lambda w: put(w, "ctxp", None), "ctx is NULL"),
    ("scene NULL", lambda w: put(w, "scenep", None), "scene is NULL"),
    ("rays NULL", lambda w: put(w, "rp", None), "rays is NULL"),
    ("rays < 0", lambda w: put(w.r, "rays", -1), "rays < 0"),
    ("rays 2^32", lambda w: put(w.r, "rays", 1 << 32), "rays > 2^32 - 1 (a ray id is 32-bit)"),
    ("origin half", lambda w: put(w.r, "origin", w.half3(w.capi.CVec3)), "rays.origin or rays.dir plane is NULL"),
    ("dir NULL", lambda w: put(w.r, "dir", w.none3(w.capi.CVec3)), "rays.origin or rays.dir plane is NULL"),
] + FOUND
WALK_HITS = [
    ("ctx NULL", lambda w: put(w, "ctxp", None), "ctx is NULL"),
    ("scene NULL", lambda w: put(w, "scenep", None), "scene is NULL"),
    ("list NULL", lambda w: put(w, "listp", None), "list is NULL"),
    ("list.count NULL", lambda w: put(w.list, "count", None), "list.count is NULL"),
    ("list.capacity < 0", lambda w: put(w.list, "capacity", -1), "list.capacity < 0"),
    ("list.ray NULL", lambda w: put(w.list, "ray", None), "list.ray or list.maxdist plane is NULL"),
    ("list.maxdist NULL", lambda w: put(w.list, "maxdist", None), "list.ray or list.maxdist plane is NULL"),
    ("list.origin half", lambda w: put(w.list, "origin", w.half3(w.capi.Vec3)), "rays.origin or rays.dir plane is NULL"),
] + FOUND
INFO = [
    ("scene NULL", lambda w: put(w, "scenep", None), "scene is NULL"),
    ("info NULL", lambda w: put(w, "infop", None), "info is NULL"),
]


@pytest.mark.parametrize("entry,call,table", [("rls_nearest_scene_create", NearestWorld.create, CREATE),
                                              ("rls_nearest_hits", NearestWorld.hits, HITS),
                                              ("rls_nearest_walk_hits", NearestWorld.walk_hits, WALK_HITS),
                                              ("rls_nearest_scene_get_info", NearestWorld.get_info, INFO)],
                         ids=["create", "hits", "walk_hits", "get_info"])
def test_every_argument_check_refuses_by_name(nearest_lib, entry, call, table):
    wrong = refusals(NearestWorld, call, entry, table)
    assert not wrong, "\n".join(wrong)


def test_empty_queries_and_destroy_of_null_need_no_device(nearest_lib):
    """rays == 0 returns before the context or the scene is read; so does a list of capacity 0, and a bound of 0"""
    w = NearestWorld()
    w.r.rays = 0
    assert w.hits() == 0
    w.bound = 0
    assert w.walk_hits() == 0
    w = NearestWorld()
    w.list.capacity = 0
    assert w.walk_hits() == 0
    assert w.nlib.rls_nearest_scene_destroy(None) == 0


def test_the_checks_are_written_once():
    """every message of the host layer appears once in nearest.hip, and every message the tables above ask for is one of them"""
    text = HIP.read_text()
    messages = re.findall(r'RLS_REQUIRE(?:_IN)?\([^;]*?"([^"]+)"\s*\)\s*;', text, flags=re.S)
    assert len(messages) >= 20, len(messages)
    twice = sorted(m for m in set(messages) if messages.count(m) > 1)
    assert twice == ["ctx is NULL", "scene is NULL"], twice         # the two entry points' own first lines, ahead of the shared path
    for _, _, want in CREATE + HITS + WALK_HITS + INFO:
        assert text.count(f'"{want}"') >= 1, want
