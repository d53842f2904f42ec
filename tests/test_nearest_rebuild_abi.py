"""CPU: the ABI of the rebuild companion library (include/rlshaders_amd_nearest_rebuild.h, librls_nearest_rebuild.so,
rlshaders_amd/nearest_rebuild.py).

The header declares, the library exports and nearest_rebuild.PROTOTYPES binds the same entry points with the same arity; every
ctypes.Structure of nearest_rebuild.py mirrors one struct of the header in member order, sizeof and every offsetof (from a
compiled probe); the header is C99 / C++14 clean and includes the nearest-hit header alone; the library holds ONE gfx950 code
object whose kernels use no scratch memory and spill nothing, links the product library by $ORIGIN and no other companion, and no
other library, header or module knows an rls_nearest_rebuild_ name, nor do this library's header and module name the box-only
update's library; every argument check refuses with "<entry>: <text>" over dummy memory (no device needed), the layout tag of a
scene included; the two other nearest libraries keep their exports and their device code."""
import ctypes as C
import inspect
import re
import subprocess

import pytest

from nearest_abi_util import UPDATE_LAYER, compiled_layout, host_layer, refusal_tables
from nearest_rebuild_util import (HEADER, RebuildWorld, declarations, declared_symbols, exported_symbols, rebuild_lib,  # noqa: F401
                                  struct_members, structs)
from trace_abi_util import ROOT, dynamic_symbols, refusals

ARITY = dict(rls_nearest_rebuild_create=3, rls_nearest_rebuild_destroy=1, rls_nearest_rebuild_get_info=2, rls_nearest_rebuild_update=3,
             rls_nearest_rebuild_read_tree=5)
STRUCTS = ["rls_nearest_rebuild_info", "rls_nearest_rebuild_mesh"]
CSRC = ROOT / "rlshaders_amd" / "csrc_nearest"
HIP = CSRC / "rebuild.hip"
NEAREST_DEVICE_CODE = "73baa46bb6e900d2"
OTHER = "nearest_" + "refit"                                        # the name this library's header and module do not hold


def mirrors():
    from rlshaders_amd import nearest_rebuild
    classes = [c for _, c in inspect.getmembers(nearest_rebuild, inspect.isclass)
               if issubclass(c, C.Structure) and c.__module__ == nearest_rebuild.__name__]
    assert len({c.__doc__ for c in classes}) == len(classes)
    return {c.__doc__: c for c in classes}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """what the C compiler says: sizeof of every struct of the header, offsetof of every member"""
    return compiled_layout(tmp_path_factory.mktemp("probe"), HEADER, structs, struct_members)


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_exports_exactly_the_header_and_the_bindings(rebuild_lib):
    from rlshaders_amd import nearest_rebuild
    declared, decl = declared_symbols(), declarations()
    assert declared and all(s.startswith("rls_nearest_rebuild_") for s in declared), declared
    assert exported_symbols(rebuild_lib) == declared
    assert sorted(nearest_rebuild.PROTOTYPES) == declared == sorted(decl) == sorted(ARITY)
    lib, out = nearest_rebuild.load(), dynamic_symbols(rebuild_lib)
    for name, n in ARITY.items():
        assert len(decl[name].split(",")) == n, (name, decl[name])
        assert f" T {name}\n" in out, name
        restype, argtypes = nearest_rebuild.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == n and getattr(lib, name).argtypes == argtypes, name
    assert all(callable(getattr(nearest_rebuild.Rebuild, m)) for m in ("update", "read_tree", "info", "close"))
    assert list(inspect.signature(nearest_rebuild.Rebuild.__init__).parameters) == ["self", "scene"]
    assert list(inspect.signature(nearest_rebuild.Rebuild.update).parameters)[:4] == ["self", "vertices", "normals", "parked"]


def test_no_other_library_header_or_module_knows_the_rebuild(rebuild_lib):
    from rlshaders_amd import _capi, build, nearest, shadow_walk, trace, walk
    from rlshaders_amd import nearest_refit as box_only
    build.build_trace_library(), build.build_walk_library(), build.build_shadow_walk_library(), build.build_nearest_library()
    build.build_nearest_refit_library()
    for lib in (build.LIB, build.TRACE_LIB, build.WALK_LIB, build.SHADOW_WALK_LIB, build.RR_LIB, build.NEAREST_LIB, build.NEAREST_REFIT_LIB):
        assert "rls_nearest_rebuild_" not in dynamic_symbols(lib), lib
        assert b"rls_nearest_rebuild" not in lib.read_bytes(), lib
    assert not [s for m in (_capi, trace, walk, shadow_walk, nearest, box_only) for s in m.PROTOTYPES if s.startswith("rls_nearest_rebuild_")]
    for h in sorted((ROOT / "include").glob("*.h")):
        if h != HEADER:
            assert "nearest_rebuild" not in h.read_text(), h
    for m in sorted((ROOT / "rlshaders_amd").glob("*.py")):
        if m.name not in ("nearest_rebuild.py", "build.py"):
            assert "nearest_rebuild" not in m.read_text(), m
    # and the other way round: this library's header and module do not name the box-only update's
    assert OTHER not in HEADER.read_text() and OTHER not in (ROOT / "rlshaders_amd" / "nearest_rebuild.py").read_text()
    # the two other nearest libraries keep their exports and their device code
    from nearest_abi_util import declared_symbols as nearest_declared
    from nearest_refit_util import declared_symbols as refit_declared, exported_symbols as refit_exported
    from rlshaders_amd.codeid import DeviceCode
    assert exported_symbols(build.NEAREST_LIB) == nearest_declared() and len(nearest_declared()) == 5
    assert refit_exported(build.NEAREST_REFIT_LIB) == refit_declared() and len(refit_declared()) == 5
    assert DeviceCode(build.NEAREST_LIB).library_id == NEAREST_DEVICE_CODE
    # the rebuild reads a scene through the private header alone, and takes the records and boxes from the refit's kernel header:
    # it includes neither library's unit nor the traversal
    text = re.sub(r"//[^\n]*", "", host_layer(HIP)[0] + (CSRC / "rls_nearest_rebuild.hpp").read_text())
    assert '#include "rls_nearest_scene.hpp"' in text and '#include "rls_nearest_refit.hpp"' in text
    assert "nearest.hip" not in text and "refit.hip" not in text and "rls_nearest_device.hpp" not in text
    for own in ("refit_records_kernel", "refit_level_kernel", "refit_node", "refit_record("):
        assert not re.search(r"\b(void|bool)\s+" + re.escape(own.rstrip("(")) + r"\s*\(", text), own     # used, not written again


# ---- structs: nearest_rebuild.py against the compiler ------------------------------------------------------------------------------
def test_every_struct_mirror_has_the_headers_layout(probe):
    assert sorted(mirrors()) == sorted(structs()) == STRUCTS
    for c_name, cls in mirrors().items():
        assert [f[0] for f in cls._fields_] == struct_members(c_name), c_name
        assert C.sizeof(cls) == probe[f"sizeof {c_name}"], c_name
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == probe[f"{c_name}.{f}"], (c_name, f)
    assert struct_members("rls_nearest_rebuild_info") == ["nv", "nt", "nodes", "levels", "leaf_size", "has_normals", "device_bytes", "updates"]
    assert struct_members("rls_nearest_rebuild_mesh") == ["nv", "vertices", "normals", "parked"]
    assert re.findall(r'#include\s+"([^"]+)"', HEADER.read_text()) == ["rlshaders_amd_nearest.h"]


# ---- the header ----------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_cxx(tmp_path):
    body = ("rls_nearest_rebuild_mesh m = {0}; rls_nearest_rebuild_info i = {0}; rls_nearest_rebuild *r = 0; rls_nearest_scene *s = 0; "
            "return (int)rls_nearest_rebuild_create(0, s, &r) + (int)rls_nearest_rebuild_update(0, r, &m) + "
            "(int)rls_nearest_rebuild_get_info(r, &i) + (int)rls_nearest_rebuild_read_tree(0, r, 0, 0, 0) + "
            "(int)rls_nearest_rebuild_destroy(r);")
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_nearest_rebuild.h"\nint main(void){ ' + body + ' }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-Wno-missing-field-initializers", "-Wno-missing-braces",
                            "-fsyntax-only", f"-I{ROOT / 'include'}", "-x", "c" if cc == "gcc" else "c++", str(src)],
                           capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)
    text = HEADER.read_text()
    for must in ("THE STATEMENT", "PARKED", "found.last", "BORROWS", "bit for bit", "by value", "SIGN"):
        assert must in text, must


# ---- the device code -----------------------------------------------------------------------------------------------------------
def test_one_gfx950_code_object_no_scratch_no_spill(rebuild_lib, tmp_path):
    from rlshaders_amd.codeid import code_objects, fatbin, kernel_digests
    objs = code_objects(fatbin(rebuild_lib))
    assert len(objs) == 1 and b"gfx950" in objs[0]
    kernels = list(kernel_digests(objs[0]))
    assert kernels and all("rebuild_" in k or "refit_" in k for k in kernels), kernels
    for k in ("rebuild_init_kernel", "rebuild_sort_count_kernel", "rebuild_sort_scatter_kernel", "rebuild_scan_reduce_kernel",
              "rebuild_scan_sums_kernel", "rebuild_scan_apply_kernel", "rebuild_mark_kernel", "rebuild_partition_kernel",
              "rebuild_leaf_kernel", "refit_records_kernel", "refit_level_kernel"):
        assert any(k in name for name in kernels), k
    assert b"nearest_kernel" not in objs[0]
    d = subprocess.run(["readelf", "-d", str(rebuild_lib)], capture_output=True, text=True, check=True).stdout
    assert "[librlshaders_amd.so]" in d and "$ORIGIN" in d
    for other in ("librls_trace", "librls_walk", "librls_shadow_walk", "librls_nearest.so", "librls_nearest_refit", "librls_ggx_rr"):
        assert other not in d, other
    (tmp_path / "rebuild.co").write_bytes(objs[0])
    note = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(tmp_path / "rebuild.co")], capture_output=True,
                          text=True, check=True).stdout
    private = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", note)
    vspills = re.findall(r"\.vgpr_spill_count:\s*(\d+)", note)
    sspills = re.findall(r"\.sgpr_spill_count:\s*(\d+)", note)
    assert len(private) == len(vspills) == len(sspills) == len(kernels), note[-3000:]
    assert set(private) == {"0"} and set(vspills) == {"0"} and set(sspills) == {"0"}, note[-3000:]


# ---- the refusals: no device needed ------------------------------------------------------------------------------------------------
TABLES = refusal_tables("rebuild")                                 # the rows of create, update, get_info and read_tree
assert [len(TABLES[verb]) for verb in ("create", "update", "get_info", "read_tree")] == [6, 8, 2, 3]


@pytest.mark.parametrize("verb", ["create", "update", "get_info", "read_tree"])
def test_every_argument_check_refuses_by_name(rebuild_lib, verb):
    wrong = refusals(RebuildWorld, getattr(RebuildWorld, verb), "rls_nearest_rebuild_" + verb, TABLES[verb])
    assert not wrong, "\n".join(wrong)


def test_info_of_dummy_memory_and_destroy_of_null(rebuild_lib):
    w = RebuildWorld()
    assert w.get_info() == 0 and (w.info.nv, w.info.nt, w.info.has_normals, w.info.updates) == (3, 1, 1, 0)
    assert w.rlib.rls_nearest_rebuild_destroy(None) == 0
    assert w.out.value is None


def test_the_checks_are_written_once():
    """every message of the host layer appears once in rebuild.hip and the shared layer it includes, and every message the
    tables above ask for is one of them"""
    text, messages = host_layer(HIP)
    assert len(messages) >= 12, len(messages)
    twice = sorted(m for m in set(messages) if messages.count(m) > 1)
    # the entry points' own first lines, ahead of the shared paths
    assert twice == ["ctx is NULL", "rebuild is NULL", "the rebuild's scene lives on another device than ctx"], twice
    for _, _, want in sum(TABLES.values(), []):
        assert text.count(f'"{want}"') >= 1, want


def test_the_shared_host_layer_names_neither_library():
    """csrc_nearest/rls_nearest_update.hpp holds neither library's noun as a word, so no message of it can leak into the other
    library; the mesh checks are written in it alone"""
    shared = UPDATE_LAYER.read_text()
    for noun in ("refit is", "rebuild is", "refit's", "rebuild's", "librls_nearest_re"):
        assert noun not in shared, noun
    everything = shared + HIP.read_text() + (CSRC / "refit.hip").read_text()
    for _, _, want in TABLES["update"][2:7]:                        # mesh NULL .. normals without: four messages
        assert everything.count(f'"{want}"') == 1 and shared.count(f'"{want}"') == 1, want
