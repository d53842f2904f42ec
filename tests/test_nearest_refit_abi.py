"""CPU: the ABI of the refit companion library (include/rlshaders_amd_nearest_refit.h, librls_nearest_refit.so,
rlshaders_amd/nearest_refit.py).

The header declares, the library exports and nearest_refit.PROTOTYPES binds the same entry points with the same arity; every
ctypes.Structure of nearest_refit.py mirrors one struct of the header in member order, sizeof and every offsetof (from a compiled
probe); the header is C99 / C++14 clean; the library holds ONE gfx950 code object whose kernels use no scratch memory and spill
nothing, links the product library by $ORIGIN and no other companion, and no other library, header or module knows an
rls_nearest_refit_ name; every argument check refuses with "<entry>: <text>" over dummy memory (no device needed), the layout
tag of a scene included; the nearest-hit library's device code is the one it was before the scene's struct moved to a header."""
import ctypes as C
import inspect
import re
import subprocess

import pytest

from nearest_abi_util import compiled_layout, host_layer, refusal_tables
from nearest_refit_util import (HEADER, SCENE_HEADER, RefitWorld, declarations, declared_symbols, exported_symbols, refit_lib,  # noqa: F401
                                struct_members, structs)
from trace_abi_util import ROOT, dynamic_symbols, refusals

ARITY = dict(rls_nearest_refit_create=3, rls_nearest_refit_destroy=1, rls_nearest_refit_get_info=2, rls_nearest_refit_update=3,
             rls_nearest_refit_read_tree=5)
STRUCTS = ["rls_nearest_refit_info", "rls_nearest_refit_mesh"]
CSRC = ROOT / "rlshaders_amd" / "csrc_nearest"
HIP = CSRC / "refit.hip"
NEAREST_DEVICE_CODE = "73baa46bb6e900d2"


def mirrors():
    from rlshaders_amd import nearest_refit
    classes = [c for _, c in inspect.getmembers(nearest_refit, inspect.isclass)
               if issubclass(c, C.Structure) and c.__module__ == nearest_refit.__name__]
    assert len({c.__doc__ for c in classes}) == len(classes)
    return {c.__doc__: c for c in classes}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """what the C compiler says: sizeof of every struct of the header, offsetof of every member"""
    return compiled_layout(tmp_path_factory.mktemp("probe"), HEADER, structs, struct_members)


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_exports_exactly_the_header_and_the_bindings(refit_lib):
    from rlshaders_amd import nearest_refit
    declared, decl = declared_symbols(), declarations()
    assert declared and all(s.startswith("rls_nearest_refit_") for s in declared), declared
    assert exported_symbols(refit_lib) == declared
    assert sorted(nearest_refit.PROTOTYPES) == declared == sorted(decl) == sorted(ARITY)
    lib, out = nearest_refit.load(), dynamic_symbols(refit_lib)
    for name, n in ARITY.items():
        assert len(decl[name].split(",")) == n, (name, decl[name])
        assert f" T {name}\n" in out, name
        restype, argtypes = nearest_refit.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == n and getattr(lib, name).argtypes == argtypes, name
    assert all(callable(getattr(nearest_refit.Refit, m)) for m in ("update", "read_tree", "info", "close"))
    assert list(inspect.signature(nearest_refit.Refit.__init__).parameters) == ["self", "scene"]
    assert list(inspect.signature(nearest_refit.Refit.update).parameters)[:4] == ["self", "vertices", "normals", "parked"]


def test_no_other_library_header_or_module_knows_the_refit(refit_lib):
    from rlshaders_amd import _capi, build, nearest, shadow_walk, trace, walk
    build.build_trace_library(), build.build_walk_library(), build.build_shadow_walk_library(), build.build_nearest_library()
    for lib in (build.LIB, build.TRACE_LIB, build.WALK_LIB, build.SHADOW_WALK_LIB, build.RR_LIB, build.NEAREST_LIB):
        assert "rls_nearest_refit_" not in dynamic_symbols(lib), lib
        assert b"rls_nearest_refit" not in lib.read_bytes(), lib
    assert not [s for m in (_capi, trace, walk, shadow_walk, nearest) for s in m.PROTOTYPES if s.startswith("rls_nearest_refit_")]
    for h in sorted((ROOT / "include").glob("*.h")):
        if h != HEADER:
            assert "nearest_refit" not in h.read_text(), h
    for m in sorted((ROOT / "rlshaders_amd").glob("*.py")):
        if m.name not in ("nearest_refit.py", "build.py"):
            assert "nearest_refit" not in m.read_text(), m
    # the nearest-hit library keeps its exports, and its device code is the one from before the scene's struct moved
    from nearest_abi_util import declared_symbols as nearest_declared
    from rlshaders_amd.codeid import DeviceCode
    assert exported_symbols(build.NEAREST_LIB) == nearest_declared() and len(nearest_declared()) == 5
    assert DeviceCode(build.NEAREST_LIB).library_id == NEAREST_DEVICE_CODE
    # the refit reads a scene through the private header alone: it includes neither the nearest library's unit nor its kernel
    text = host_layer(HIP)[0] + (CSRC / "rls_nearest_refit.hpp").read_text()
    assert '#include "rls_nearest_scene.hpp"' in text and "nearest.hip" not in re.sub(r"//[^\n]*", "", text)
    assert "rls_nearest_device.hpp" not in re.sub(r"//[^\n]*", "", text)
    assert "struct rls_nearest_scene {" in SCENE_HEADER.read_text() and "struct rls_nearest_scene {" not in (CSRC / "nearest.hip").read_text()


# ---- structs: nearest_refit.py against the compiler ----------------------------------------------------------------------------------
def test_every_struct_mirror_has_the_headers_layout(probe):
    assert sorted(mirrors()) == sorted(structs()) == STRUCTS
    for c_name, cls in mirrors().items():
        assert [f[0] for f in cls._fields_] == struct_members(c_name), c_name
        assert C.sizeof(cls) == probe[f"sizeof {c_name}"], c_name
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == probe[f"{c_name}.{f}"], (c_name, f)
    assert '#include "rlshaders_amd_nearest.h"' in HEADER.read_text()


# ---- the header ----------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_cxx(tmp_path):
    body = ("rls_nearest_refit_mesh m = {0}; rls_nearest_refit_info i = {0}; rls_nearest_refit *r = 0; rls_nearest_scene *s = 0; "
            "return (int)rls_nearest_refit_create(0, s, &r) + (int)rls_nearest_refit_update(0, r, &m) + "
            "(int)rls_nearest_refit_get_info(r, &i) + (int)rls_nearest_refit_read_tree(0, r, 0, 0, 0) + "
            "(int)rls_nearest_refit_destroy(r);")
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_nearest_refit.h"\nint main(void){ ' + body + ' }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-Wno-missing-field-initializers", "-Wno-missing-braces",
                            "-fsyntax-only", f"-I{ROOT / 'include'}", "-x", "c" if cc == "gcc" else "c++", str(src)],
                           capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)
    text = HEADER.read_text()
    assert "PARKED" in text and "found.last" in text and "BORROWS" in text and "bit for bit" in text


# ---- the device code -----------------------------------------------------------------------------------------------------------
def test_one_gfx950_code_object_no_scratch_no_spill(refit_lib, tmp_path):
    from rlshaders_amd.codeid import code_objects, fatbin, kernel_digests
    objs = code_objects(fatbin(refit_lib))
    assert len(objs) == 1 and b"gfx950" in objs[0]
    kernels = list(kernel_digests(objs[0]))
    assert kernels and all("refit_" in k for k in kernels) and any("refit_records_kernel" in k for k in kernels), kernels
    assert b"nearest_kernel" not in objs[0]
    d = subprocess.run(["readelf", "-d", str(refit_lib)], capture_output=True, text=True, check=True).stdout
    assert "[librlshaders_amd.so]" in d and "$ORIGIN" in d
    for other in ("librls_trace", "librls_walk", "librls_shadow_walk", "librls_nearest.so", "librls_ggx_rr"):
        assert other not in d, other
    (tmp_path / "refit.co").write_bytes(objs[0])
    note = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(tmp_path / "refit.co")], capture_output=True,
                          text=True, check=True).stdout
    names = re.findall(r"\.name:\s*(\S+)", note)
    private = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", note)
    spills = re.findall(r"\.vgpr_spill_count:\s*(\d+)", note)
    assert len([n for n in names if "refit_" in n and "kernel" in n]) >= len(kernels)
    assert len(private) == len(spills) == len(kernels) and set(private) == {"0"} and set(spills) == {"0"}, note[-3000:]


# ---- the refusals: no device needed ------------------------------------------------------------------------------------------------
TABLES = refusal_tables("refit")                                   # the rows of create, update, get_info and read_tree
assert [len(TABLES[verb]) for verb in ("create", "update", "get_info", "read_tree")] == [6, 8, 2, 3]


@pytest.mark.parametrize("verb", ["create", "update", "get_info", "read_tree"])
def test_every_argument_check_refuses_by_name(refit_lib, verb):
    wrong = refusals(RefitWorld, getattr(RefitWorld, verb), "rls_nearest_refit_" + verb, TABLES[verb])
    assert not wrong, "\n".join(wrong)


def test_info_of_dummy_memory_and_destroy_of_null(refit_lib):
    w = RefitWorld()
    assert w.get_info() == 0 and (w.info.nv, w.info.nt, w.info.has_normals, w.info.updates) == (3, 1, 1, 0)
    assert w.rlib.rls_nearest_refit_destroy(None) == 0
    assert w.out.value is None


def test_the_checks_are_written_once():
    """every message of the host layer appears once in refit.hip and the shared layer it includes, and every message the tables
    above ask for is one of them"""
    text, messages = host_layer(HIP)
    assert len(messages) >= 12, len(messages)
    twice = sorted(m for m in set(messages) if messages.count(m) > 1)
    # the entry points' own first lines, ahead of the shared paths
    assert twice == ["ctx is NULL", "refit is NULL", "the refit's scene lives on another device than ctx"], twice
    for _, _, want in sum(TABLES.values(), []):
        assert text.count(f'"{want}"') >= 1, want
    # nothing of the nearest library's messages moved or changed with the struct
    assert "layout" not in "".join(re.findall(r'"([^"]*)"', (CSRC / "nearest.hip").read_text()))
