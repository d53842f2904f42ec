"""CPU: the ABI of the shadow walk's companion library (include/rlshaders_amd_shadow_walk.h, librls_shadow_walk.so,
rlshaders_amd/shadow_walk.py).

The header declares, the library exports and shadow_walk.PROTOTYPES binds the same entry points with the same arity; every
ctypes.Structure of shadow_walk.py mirrors one struct of the header in member order, sizeof and every offsetof (from a compiled
probe), and the list it shares with the probe walk is that module's mirror of rls_walk_rays; the header is C99 / C++14 clean; the
library holds ONE gfx950 code object with the walk's kernels and the scan it includes, links the product library by $ORIGIN and
neither other companion, and none of the other three libraries, headers and modules knows an rls_shadow_walk_ name; every
argument check refuses with "<entry>: <text>" over dummy memory (no device needed)."""
import ctypes as C
import inspect
import re
import subprocess

import pytest

from shadow_walk_abi_util import (HEADER, ShadowWalkWorld, declarations, declared_symbols, exported_symbols,  # noqa: F401
                                  shadow_walk_lib, struct_members, structs)
from trace_abi_util import INVALID, ROOT, dynamic_symbols, put, refusals
from walk_abi_util import ACTIVE, LIST_IN, LIST_OUT

ARITY = dict(rls_shadow_walk_scratch_bytes=2, rls_shadow_walk_begin=4, rls_shadow_walk_step=6, rls_shadow_walk_active=3)
CONSTANTS = ("RLS_SHADOW_WALK_MAX_STEPS",)
KERNELS = ("shadow_begin_kernel", "shadow_step_kernel", "shadow_place_kernel", "trace_scan_block_kernel",
           "trace_scan_totals_kernel", "trace_scan_add_kernel")
HIP = ROOT / "rlshaders_amd" / "csrc_shadow_walk" / "shadow_walk.hip"
SHARED = ROOT / "rlshaders_amd" / "csrc_walk" / "rls_walk_list.hpp"


def mirrors():
    from rlshaders_amd import shadow_walk
    classes = [c for _, c in inspect.getmembers(shadow_walk, inspect.isclass)
               if issubclass(c, C.Structure) and c.__module__ == shadow_walk.__name__]
    assert len({c.__doc__ for c in classes}) == len(classes)
    return {c.__doc__: c for c in classes}


def _compile_and_run(tmp_path, lines):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(['#include <stddef.h>', '#include <stdio.h>', '#include "rlshaders_amd_shadow_walk.h"',
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
def test_exports_exactly_the_header_and_the_bindings(shadow_walk_lib):
    from rlshaders_amd import shadow_walk, walk
    declared, decl = declared_symbols(), declarations()
    assert declared and all(s.startswith("rls_shadow_walk_") for s in declared), declared
    assert exported_symbols(shadow_walk_lib) == declared
    assert sorted(shadow_walk.PROTOTYPES) == declared == sorted(decl) == sorted(ARITY)
    lib, out = shadow_walk.load(), dynamic_symbols(shadow_walk_lib)
    for name, n in ARITY.items():
        assert len(decl[name].split(",")) == n, (name, decl[name])
        assert f" T {name}\n" in out, name
        restype, argtypes = shadow_walk.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == n and getattr(lib, name).argtypes == argtypes, name
    for cls, methods in dict(ShadowWalk=("begin", "step"), Found=("struct",)).items():
        assert all(callable(getattr(getattr(shadow_walk, cls), m)) for m in methods), cls
    assert callable(shadow_walk.run) and isinstance(shadow_walk.ShadowWalk.active, property)
    assert isinstance(shadow_walk.ShadowWalk.rays, property)
    sig = inspect.signature(shadow_walk.ShadowWalk.__init__)
    assert list(sig.parameters)[:4] == ["self", "ctx", "queue", "O"]
    assert all(sig.parameters[k].default is None for k in ("base", "via", "out", "scratch", "alloc")) and "max_steps" in sig.parameters
    assert list(inspect.signature(shadow_walk.Found.__init__).parameters) == ["self", "hit", "t", "P", "opacity", "index"]
    # the list walk's host layer is written once, in walk.ListWalk: neither walk states it again
    for cls in (shadow_walk.ShadowWalk, walk.ProbeWalk):
        assert issubclass(cls, walk.ListWalk) and not {"begin", "step", "active", "rays"} & set(vars(cls)), cls


def test_other_libraries_know_nothing_of_the_shadow_walk(shadow_walk_lib):
    from rlshaders_amd import _capi, build, trace, walk
    build.build_walk_library()
    for lib in (build.LIB, build.TRACE_LIB, build.WALK_LIB):
        assert "rls_shadow_walk_" not in dynamic_symbols(lib), lib
        assert b"rls_shadow_walk_" not in lib.read_bytes(), lib
    assert not [s for s in list(_capi.PROTOTYPES) + list(trace.PROTOTYPES) + list(walk.PROTOTYPES) if s.startswith("rls_shadow_walk_")]
    for h in ("rlshaders_amd.h", "rlshaders_amd_trace.h", "rlshaders_amd_walk.h"):
        text = (ROOT / "include" / h).read_text()
        assert "rlshaders_amd_shadow_walk.h" not in text and "rls_shadow_walk_" not in text, h
    for m in ("trace.py", "walk.py"):
        assert "shadow_walk" not in (ROOT / "rlshaders_amd" / m).read_text(), m


# ---- structs and constants: shadow_walk.py against the compiler ------------------------------------------------------------------
def test_every_struct_mirror_has_the_headers_layout(probe):
    from rlshaders_amd import shadow_walk, walk
    assert sorted(mirrors()) == sorted(structs()) == ["rls_shadow_walk", "rls_shadow_walk_found"]
    for c_name, cls in mirrors().items():
        assert [f[0] for f in cls._fields_] == struct_members(c_name), c_name
        assert C.sizeof(cls) == probe[f"sizeof {c_name}"], c_name
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == probe[f"{c_name}.{f}"], (c_name, f)
    # the active list is the probe walk's type, in C (the header includes rlshaders_amd_walk.h) and in Python
    assert shadow_walk.WalkRays_ is walk.WalkRays_ and '#include "rlshaders_amd_walk.h"' in HEADER.read_text()
    assert "rls_walk_rays" not in structs()
    for name in CONSTANTS:
        assert getattr(shadow_walk, name) == probe[name], name
    assert probe["RLS_SHADOW_WALK_MAX_STEPS"] == 255


# ---- the header ----------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_cxx(tmp_path):
    body = ("rls_shadow_walk w = {0}; rls_walk_rays a = {0}, b = {0}; rls_shadow_walk_found f = {0}; rls_shadow_queue q = {0}; "
            "size_t bytes = 0; int64_t m = 0; w.max_steps = RLS_SHADOW_WALK_MAX_STEPS; "
            "return (int)rls_shadow_walk_scratch_bytes(0, &bytes) + (int)rls_shadow_walk_begin(0, &w, &q, &a) + "
            "(int)rls_shadow_walk_step(0, &w, &a, &f, -1, &b) + (int)rls_shadow_walk_active(0, &b, &m);")
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_shadow_walk.h"\nint main(void){ ' + body + ' }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-Wno-missing-field-initializers", "-Wno-missing-braces",
                            "-fsyntax-only", f"-I{ROOT / 'include'}", "-x", "c" if cc == "gcc" else "c++", str(src)],
                           capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)
    text = HEADER.read_text()
    assert "keeps the T it has" in text and "The type is reused, not restated" in text      # what the issue asks the header to say


# ---- the device code -----------------------------------------------------------------------------------------------------------
def test_one_gfx950_code_object_linked_by_origin(shadow_walk_lib):
    from rlshaders_amd.codeid import DeviceCode, code_objects, fatbin, kernel_digests
    objs = code_objects(fatbin(shadow_walk_lib))
    assert len(objs) == 1 and b"gfx950" in objs[0]
    dc = DeviceCode(shadow_walk_lib)
    for k in KERNELS:
        assert k.encode() in objs[0], k
    assert dc.unit_of_kernel("shadow_step_kernel") is not None
    # the code object's kernels, all of them: the walk's three (the place kernel in its two forms), the scan's three, and the one
    # non-template kernel csrc_trace/rls_trace_queue.hpp defines beside the scan, carried unused as in librls_walk.so
    got = sorted(re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", k).split("E")[0].split("IL")[0] for k in kernel_digests(objs[0]))
    assert got == sorted(KERNELS + ("shadow_place_kernel", "hits_compact_kernel")), got
    d = subprocess.run(["readelf", "-d", str(shadow_walk_lib)], capture_output=True, text=True, check=True).stdout
    assert "[librlshaders_amd.so]" in d and "$ORIGIN" in d and "librls_trace" not in d and "librls_walk" not in d
    # the shadow walk's kernels are in no other library
    from rlshaders_amd import build
    for lib in (build.LIB, build.TRACE_LIB, build.build_walk_library()):
        for elf in code_objects(fatbin(lib)):
            assert not [k for k in KERNELS[:3] if k.encode() in elf], lib


# ---- the scratch size and the refusals: no device needed -----------------------------------------------------------------------
def test_scratch_size():
    from rlshaders_amd import shadow_walk
    lib, b = shadow_walk.load(), C.c_size_t()
    up = lambda x: (x + 255) // 256 * 256
    for rays in (0, 1, 255, 256, 257, 2048 * 256 + 1, (1 << 32) - 1):
        tiles = max((rays + 255) // 256, 1)
        want = up(2 * rays) + up(4 * rays) + up(8 * (tiles + 1)) + up(8 * ((tiles + 2047) // 2048))
        assert shadow_walk.scratch_bytes(rays) == want, rays
    assert lib.rls_shadow_walk_scratch_bytes(-1, C.byref(b)) == INVALID
    assert lib.rls_shadow_walk_scratch_bytes(1 << 32, C.byref(b)) == INVALID
    assert lib.rls_shadow_walk_scratch_bytes(1, None) == INVALID


WALK = [
    ("ctx NULL", lambda w: put(w, "ctxp", None), "ctx is NULL"),
    ("walk NULL", lambda w: put(w, "wp", None), "walk is NULL"),
    ("rays < 0", lambda w: put(w.w, "rays", -1), "rays < 0"),
    ("rays 2^32", lambda w: put(w.w, "rays", 1 << 32), "rays > 2^32 - 1 (the list's ray index is 32-bit)"),
    ("max_steps 0", lambda w: put(w.w, "max_steps", 0), "walk.max_steps must be in [1, 255]"),
    ("max_steps 256", lambda w: put(w.w, "max_steps", 256), "walk.max_steps must be in [1, 255]"),
    ("base half", lambda w: put(w.w, "base", w.half3(w.capi.CRgb)), "walk.base is partly NULL: all three planes or none"),
    ("visibility NULL", lambda w: put(w.w, "visibility", w.none3(w.capi.Rgb)), "walk.visibility plane is NULL"),
    ("visibility half", lambda w: put(w.w, "visibility", w.half3(w.capi.Rgb)), "walk.visibility plane is NULL"),
    ("scratch NULL", lambda w: put(w.w, "scratch", None), "walk.scratch is NULL or smaller than rls_shadow_walk_scratch_bytes"),
    ("scratch short", lambda w: put(w.w, "scratch_bytes", w.w.scratch_bytes - 1),
     "walk.scratch is NULL or smaller than rls_shadow_walk_scratch_bytes"),
]
BEGIN = WALK + LIST_OUT + [
    ("O NULL", lambda w: put(w.w, "O", w.half3(w.capi.CVec3)), "walk.O plane is NULL"),
    ("queue NULL", lambda w: put(w, "qp", None), "queue is NULL"),
    ("queue.capacity short", lambda w: put(w.q, "capacity", w.w.rays - 1), "queue.capacity < walk.rays"),
    ("queue.maxdist NULL", lambda w: put(w.q, "maxdist", None), "queue.dir or queue.maxdist plane is NULL"),
    ("queue.dir NULL", lambda w: put(w.q, "dir", w.half3(w.capi.Vec3)), "queue.dir or queue.maxdist plane is NULL"),
    ("queue.point NULL", lambda w: put(w.q, "point", None), "queue.point is NULL: the walk reads every ray's origin through it"),
]
STEP = WALK + LIST_OUT + LIST_IN + [
    ("found NULL", lambda w: put(w, "fp", None), "found is NULL"),
    ("found.hit NULL", lambda w: put(w.f, "hit", None), "found.hit, found.t, found.P or found.opacity plane is NULL"),
    ("found.opacity half", lambda w: put(w.f, "opacity", w.half3(w.capi.CRgb)), "found.hit, found.t, found.P or found.opacity plane is NULL"),
    ("index, empty table", lambda w: put(w.f, "index", w.p), "found.index is set with found.table_count == 0"),
]


@pytest.mark.parametrize("entry,call,table", [("rls_shadow_walk_begin", ShadowWalkWorld.begin, BEGIN),
                                              ("rls_shadow_walk_step", ShadowWalkWorld.step, STEP),
                                              ("rls_shadow_walk_active", ShadowWalkWorld.active, ACTIVE)],
                         ids=["begin", "step", "active"])
def test_every_argument_check_refuses_by_name(shadow_walk_lib, entry, call, table):
    wrong = refusals(ShadowWalkWorld, call, entry, table)
    assert not wrong, "\n".join(wrong)


def test_scratch_bytes_refuses_by_name(shadow_walk_lib):
    from trace_abi_util import last_error
    from rlshaders_amd import shadow_walk
    lib, b = shadow_walk.load(), C.c_size_t()
    for args, text in (((-1, C.byref(b)), "rays < 0"), ((1, None), "bytes is NULL")):
        assert lib.rls_shadow_walk_scratch_bytes(*args) == INVALID and last_error() == f"rls_shadow_walk_scratch_bytes: {text}"


def test_the_checks_are_written_once():
    """every message of the host layer appears once in shadow_walk.hip and the list machinery it shares with the probe walk
    (csrc_walk/rls_walk_list.hpp) taken together, apart from the in / out pair of one check, and every message the tables above
    ask for is one of them; what the shared header says, shadow_walk.hip does not say again"""
    hip, shared = HIP.read_text(), SHARED.read_text()
    pattern = r'RLS_REQUIRE(?:_IN)?\([^;]*?"([^"]+)"\s*\)\s*;'
    text = hip + shared
    messages = re.findall(pattern, text, flags=re.S)
    assert len(messages) >= 20 and len(messages) == len(set(messages)), sorted(m for m in set(messages) if messages.count(m) > 1)
    for _, _, want in WALK + BEGIN + STEP + ACTIVE:
        assert text.count(f'"{want}"') == 1, want
    in_shared = re.findall(pattern, shared, flags=re.S)
    assert in_shared and not [m for m in in_shared if f'"{m}"' in hip]
