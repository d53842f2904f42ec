"""CPU: the ABI of the probe walk's companion library (include/rlshaders_amd_walk.h, librls_walk.so, rlshaders_amd/walk.py).

The header declares, the library exports and walk.PROTOTYPES binds the same entry points with the same arity; every
ctypes.Structure of walk.py mirrors one struct of the header in member order, sizeof and every offsetof (from a compiled probe);
the header is C99 / C++14 clean; the library holds ONE gfx950 code object with the walk's kernels and the scan it includes, links
the product library by $ORIGIN, and neither of the other two libraries knows an rls_walk_ name; every argument check refuses
with "<entry>: <text>" over dummy memory (no device needed)."""
import ctypes as C
import inspect
import re
import subprocess

import pytest

from trace_abi_util import INVALID, ROOT, dynamic_symbols, put, refusals
from walk_abi_util import (ACTIVE, HEADER, LIST_IN, LIST_OUT, WalkWorld, declared_walk_symbols, exported_walk_symbols,  # noqa: F401
                           walk_declarations, walk_lib, walk_struct_members, walk_structs)

ARITY = dict(rls_walk_scratch_bytes=2, rls_walk_begin=4, rls_walk_step=6, rls_walk_active=3)
CONSTANTS = ("RLS_WALK_TRIALS", "RLS_WALK_FOREIGN_STOPS", "RLS_WALK_FOREIGN_SKIPS")
KERNELS = ("walk_begin_kernel", "walk_step_kernel", "walk_place_kernel", "trace_scan_block_kernel", "trace_scan_totals_kernel",
           "trace_scan_add_kernel")


def mirrors():
    from rlshaders_amd import walk
    classes = [c for _, c in inspect.getmembers(walk, inspect.isclass) if issubclass(c, C.Structure) and c.__module__ == walk.__name__]
    assert len({c.__doc__ for c in classes}) == len(classes)
    return {c.__doc__: c for c in classes}


def _compile_and_run(tmp_path, lines):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(['#include <stddef.h>', '#include <stdio.h>', '#include "rlshaders_amd_walk.h"', 'int main(void) {',
                              *lines, '  return 0; }']) + "\n")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return [l for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if l]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """what the C compiler says: sizeof of every struct of the header, offsetof of every member, the value of every constant"""
    lines = [f'  printf("{name} %lld\\n", (long long)({name}));' for name in CONSTANTS + ("RLS_MAX_PROBE_HITS",)]
    for c_name in walk_structs():
        lines.append(f'  printf("sizeof {c_name} %zu\\n", sizeof({c_name}));')
        lines += [f'  printf("{c_name}.{m} %zu\\n", offsetof({c_name}, {m}));' for m in walk_struct_members(c_name)]
    out = _compile_and_run(tmp_path_factory.mktemp("probe"), lines)
    assert len(out) == len(lines)
    return {k: int(v) for k, v in (l.rsplit(" ", 1) for l in out)}


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_exports_exactly_the_header_and_the_bindings(walk_lib):
    from rlshaders_amd import walk
    declared, decl = declared_walk_symbols(), walk_declarations()
    assert declared and all(s.startswith("rls_walk_") for s in declared), declared
    assert exported_walk_symbols(walk_lib) == declared
    assert sorted(walk.PROTOTYPES) == declared == sorted(decl) == sorted(ARITY)
    lib, out = walk.load(), dynamic_symbols(walk_lib)
    for name, n in ARITY.items():
        assert len(decl[name].split(",")) == n, (name, decl[name])
        assert f" T {name}\n" in out, name
        restype, argtypes = walk.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == n and getattr(lib, name).argtypes == argtypes, name
    for cls, methods in dict(ProbeWalk=("begin", "step", "hits"), Found=("struct",)).items():
        assert all(callable(getattr(getattr(walk, cls), m)) for m in methods), cls
    assert callable(walk.run) and isinstance(walk.ProbeWalk.active, property) and isinstance(walk.ProbeWalk.rays, property)
    sig = inspect.signature(walk.ProbeWalk.__init__)
    assert list(sig.parameters)[:4] == ["self", "ctx", "queue", "P"]
    assert sig.parameters["own"].default is None and sig.parameters["max_hits"].default == 12 and sig.parameters["foreign"].default == "stop"


def test_other_libraries_know_nothing_of_the_walk(walk_lib):
    from rlshaders_amd import _capi, build, trace
    for lib in (build.LIB, build.TRACE_LIB):
        assert "rls_walk_" not in dynamic_symbols(lib), lib
        assert b"rls_walk_" not in lib.read_bytes(), lib
    assert not [s for s in list(_capi.PROTOTYPES) + list(trace.PROTOTYPES) if s.startswith("rls_walk_")]
    for h in ("rlshaders_amd.h", "rlshaders_amd_trace.h"):
        assert "rlshaders_amd_walk.h" not in (ROOT / "include" / h).read_text() and "rls_walk_" not in (ROOT / "include" / h).read_text()


# ---- structs and constants: walk.py against the compiler -----------------------------------------------------------------------
def test_every_struct_mirror_has_the_headers_layout(probe):
    from rlshaders_amd import trace, walk
    assert sorted(mirrors()) == sorted(walk_structs()) == ["rls_walk", "rls_walk_found", "rls_walk_hits", "rls_walk_rays"]
    for c_name, cls in mirrors().items():
        assert [f[0] for f in cls._fields_] == walk_struct_members(c_name), c_name
        assert C.sizeof(cls) == probe[f"sizeof {c_name}"], c_name
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == probe[f"{c_name}.{f}"], (c_name, f)
    # rls_walk_hits: the members of rls_probe_hits without the irradiance, in its order and at its offsets
    assert [f[0] for f in walk.WalkHits_._fields_] == [f[0] for f in trace.ProbeHits_._fields_[:-1]]
    for f, _ in walk.WalkHits_._fields_:
        assert getattr(walk.WalkHits_, f).offset == getattr(trace.ProbeHits_, f).offset, f
    assert dict(walk.Walk_._fields_)["hits"] is walk.WalkHits_
    for name in CONSTANTS:
        assert getattr(walk, name) == probe[name], name
    assert probe["RLS_WALK_TRIALS"] == probe["RLS_MAX_PROBE_HITS"] == 12 and probe["RLS_WALK_FOREIGN_STOPS"] == 0


# ---- the header ----------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_cxx(tmp_path):
    body = ("rls_walk w = {0}; rls_walk_rays a = {0}, b = {0}; rls_walk_found f = {0}; rls_probe_queue q = {0}; size_t bytes = 0; "
            "int64_t m = 0; w.foreign = RLS_WALK_FOREIGN_SKIPS; w.hits.max_hits = RLS_WALK_TRIALS; "
            "return (int)rls_walk_scratch_bytes(0, &bytes) + (int)rls_walk_begin(0, &w, &q, &a) + "
            "(int)rls_walk_step(0, &w, &a, &f, -1, &b) + (int)rls_walk_active(0, &b, &m);")
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_walk.h"\nint main(void){ ' + body + ' }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-Wno-missing-field-initializers", "-Wno-missing-braces",
                            "-fsyntax-only", f"-I{ROOT / 'include'}", "-x", "c" if cc == "gcc" else "c++", str(src)],
                           capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)
    text = HEADER.read_text()
    assert "AiTraceProbe is closed" in text and "COMPILED reference" in text       # which policy the reference is


# ---- the device code -----------------------------------------------------------------------------------------------------------
def test_one_gfx950_code_object_linked_by_origin(walk_lib):
    from rlshaders_amd.codeid import DeviceCode, code_objects, fatbin
    objs = code_objects(fatbin(walk_lib))
    assert len(objs) == 1 and b"gfx950" in objs[0]
    dc = DeviceCode(walk_lib)
    for k in KERNELS:
        assert k.encode() in objs[0], k
    assert dc.unit_of_kernel("walk_step_kernel") is not None
    # the code object's kernels, all of them: the walk's three (the place kernel in its two forms), the scan's three, and the one
    # non-template kernel csrc_trace/rls_trace_queue.hpp defines beside the scan, carried unused (that header is the trace
    # library's and has no switch for it)
    from rlshaders_amd.codeid import kernel_digests
    got = sorted(re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", k).split("E")[0].split("IL")[0] for k in kernel_digests(objs[0]))
    assert got == sorted(KERNELS + ("walk_place_kernel", "hits_compact_kernel")), got
    d = subprocess.run(["readelf", "-d", str(walk_lib)], capture_output=True, text=True, check=True).stdout
    assert "[librlshaders_amd.so]" in d and "$ORIGIN" in d and "librls_trace" not in d
    # the walk's kernels are in neither other library
    from rlshaders_amd import build
    for lib in (build.LIB, build.TRACE_LIB):
        for elf in code_objects(fatbin(lib)):
            assert not [k for k in KERNELS[:3] if k.encode() in elf], lib


# ---- the scratch size and the refusals: no device needed -----------------------------------------------------------------------
def test_scratch_size():
    from rlshaders_amd import walk
    lib, b = walk.load(), C.c_size_t()
    up = lambda x: (x + 255) // 256 * 256
    for rays in (0, 1, 255, 256, 257, 2048 * 256 + 1, (1 << 32) - 1):
        tiles = max((rays + 255) // 256, 1)
        want = up(rays) + up(4 * rays) + up(8 * (tiles + 1)) + up(8 * ((tiles + 2047) // 2048))
        assert walk.scratch_bytes(rays) == want, rays
    assert lib.rls_walk_scratch_bytes(-1, C.byref(b)) == INVALID and lib.rls_walk_scratch_bytes(1 << 32, C.byref(b)) == INVALID
    assert lib.rls_walk_scratch_bytes(1, None) == INVALID


WALK = [
    ("ctx NULL", lambda w: put(w, "ctxp", None), "ctx is NULL"),
    ("walk NULL", lambda w: put(w, "wp", None), "walk is NULL"),
    ("rays < 0", lambda w: put(w.w, "rays", -1), "rays < 0"),
    ("rays 2^32", lambda w: put(w.w, "rays", 1 << 32), "rays > 2^32 - 1 (the list's ray index is 32-bit)"),
    ("spp 0", lambda w: put(w.w, "spp", 0), "walk.spp < 1 and walk.point is NULL"),
    ("foreign 2", lambda w: put(w.w, "foreign", 2), "walk.foreign is neither RLS_WALK_FOREIGN_STOPS nor RLS_WALK_FOREIGN_SKIPS"),
    ("max_hits 0", lambda w: put(w.w.hits, "max_hits", 0), "walk.hits.max_hits must be in [1, 12]"),
    ("max_hits 13", lambda w: put(w.w.hits, "max_hits", 13), "walk.hits.max_hits must be in [1, 12]"),
    ("stride short", lambda w: put(w.w.hits, "stride", w.w.rays - 1), "walk.hits.stride < walk.rays"),
    ("P NULL", lambda w: put(w.w, "P", w.half3(w.capi.CVec3)), "walk.P plane is NULL"),
    ("hits.count NULL", lambda w: put(w.w.hits, "count", None), "walk.hits.count, walk.hits.P or walk.hits.N plane is NULL"),
    ("hits.N NULL", lambda w: put(w.w.hits, "N", w.half3(w.capi.Vec3)), "walk.hits.count, walk.hits.P or walk.hits.N plane is NULL"),
    ("scratch NULL", lambda w: put(w.w, "scratch", None), "walk.scratch is NULL or smaller than rls_walk_scratch_bytes"),
    ("scratch short", lambda w: put(w.w, "scratch_bytes", w.w.scratch_bytes - 1), "walk.scratch is NULL or smaller than rls_walk_scratch_bytes"),
]
BEGIN = WALK + LIST_OUT + [
    ("queue NULL", lambda w: put(w, "qp", None), "queue is NULL"),
    ("queue.capacity short", lambda w: put(w.q, "capacity", w.w.rays - 1), "queue.capacity < walk.rays"),
    ("queue.maxdist NULL", lambda w: put(w.q, "maxdist", None), "queue.origin, queue.dir or queue.maxdist plane is NULL"),
    ("queue.origin NULL", lambda w: put(w.q, "origin", w.half3(w.capi.Vec3)), "queue.origin, queue.dir or queue.maxdist plane is NULL"),
]
STEP = WALK + LIST_OUT + LIST_IN + [
    ("found NULL", lambda w: put(w, "fp", None), "found is NULL"),
    ("found.hit NULL", lambda w: put(w.f, "hit", None), "found.hit, found.t, found.P, found.N or found.Ns plane is NULL"),
    ("found.Ns NULL", lambda w: put(w.f, "Ns", w.half3(w.capi.CVec3)), "found.hit, found.t, found.P, found.N or found.Ns plane is NULL"),
    ("own without object", lambda w: put(w.w, "own", w.p), "walk.own and found.object must be both set or both NULL"),
    ("object without own", lambda w: put(w.f, "object", w.p), "walk.own and found.object must be both set or both NULL"),
]


@pytest.mark.parametrize("entry,call,table", [("rls_walk_begin", WalkWorld.begin, BEGIN), ("rls_walk_step", WalkWorld.step, STEP),
                                              ("rls_walk_active", WalkWorld.active, ACTIVE)], ids=["begin", "step", "active"])
def test_every_argument_check_refuses_by_name(walk_lib, entry, call, table):
    wrong = refusals(WalkWorld, call, entry, table)
    assert not wrong, "\n".join(wrong)


def test_the_checks_are_written_once():
    """every message of the host layer appears once in walk.hip and the list machinery it shares with the shadow walk
    (rls_walk_list.hpp) taken together, apart from the in / out pair of one check; what the shared header says, walk.hip does
    not say again"""
    import re
    hip = (ROOT / "rlshaders_amd" / "csrc_walk" / "walk.hip").read_text()
    shared = (ROOT / "rlshaders_amd" / "csrc_walk" / "rls_walk_list.hpp").read_text()
    pattern = r'RLS_REQUIRE(?:_IN)?\([^;]*?"([^"]+)"\s*\)\s*;'
    messages = re.findall(pattern, hip + shared, flags=re.S)
    assert len(messages) >= 20 and len(messages) == len(set(messages)), sorted(m for m in set(messages) if messages.count(m) > 1)
    in_shared = re.findall(pattern, shared, flags=re.S)
    assert in_shared and not [m for m in in_shared if f'"{m}"' in hip]
