"""CPU: the caller-traced light loops in the companion library (rls_trace_ggx_direct_emit / _resolve,
rls_trace_disney_direct_emit / _resolve, rls_trace_shadow_scratch_bytes; librls_trace.so).

The header section compiles as C99 and C++14; both code objects carry the emit kernels (EXACT <G, 0>, FAST <G, 1>), the
EXACT one the mode-free compaction and resolve; the product library carries none of them; the Python bindings prototype
the five entry points and rls_shadow_queue has the header's layout; the host-side argument checks that need no device."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
ENTRY = ("rls_trace_shadow_scratch_bytes", "rls_trace_ggx_direct_emit", "rls_trace_disney_direct_emit",
         "rls_trace_ggx_direct_resolve", "rls_trace_disney_direct_resolve")
EMIT_KERNELS = ("ggx_direct_emit_kernel", "disney_direct_emit_kernel")
SHARED_KERNELS = ("shadow_compact_kernel<1>", "shadow_compact_kernel<3>", "shadow_resolve_kernel<1>",
                  "shadow_resolve_kernel<3>")


@pytest.fixture(scope="module")
def trace_lib():
    from rlshaders_amd import build
    return build.build_trace_library()


def test_header_section_compiles_as_c_and_cxx(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_trace.h"\n'
                   'int main(void){ rls_shadow_queue q = {0}; size_t b = 0; (void)q;\n'
                   '  if ((RLS_SHADOW_LIGHT_MASK | RLS_SHADOW_BSDF | RLS_SHADOW_SPECULAR | RLS_SHADOW_DIFFUSE) != 0x3F) return 2;\n'
                   '  if (RLS_SHADOW_LIGHT_MASK != RLS_MAX_LIGHTS - 1) return 3;\n'
                   '  return rls_trace_shadow_scratch_bytes(1, 1, 1, &b) == RLS_OK ? 0 : 1; }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{ROOT / 'include'}",
                            "-x", "c" if cc == "gcc" else "c++", str(src)], capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)


def test_both_code_objects_carry_the_emit_kernels(trace_lib):
    from rlshaders_amd.codeid import DeviceCode, code_objects, fatbin
    assert len(code_objects(fatbin(trace_lib))) == 2
    dc = DeviceCode(trace_lib)
    units = {0: set(), 1: set()}
    for fast in (0, 1):
        for k in EMIT_KERNELS:
            for g in (1, 4, 16, 64):
                u = dc.unit_of_kernel(f"{k}<{g}, {fast}>")
                assert u is not None, (k, g, fast)
                units[fast].add(u)
    assert len(units[0]) == 1 and len(units[1]) == 1 and units[0] != units[1]
    for k in SHARED_KERNELS:                     # free of the math mode: in the EXACT unit alone
        assert dc.unit_of_kernel(k) in units[0], k


def test_no_light_loop_trace_kernel_in_the_product_library(trace_lib):
    from rlshaders_amd import build
    from rlshaders_amd.codeid import code_objects, fatbin
    for elf in code_objects(fatbin(build.build_library())):
        for k in EMIT_KERNELS + ("shadow_compact_kernel", "shadow_resolve_kernel"):
            assert k.encode() not in elf, k
    syms = subprocess.run(["nm", "-D", "--defined-only", str(build.LIB)], capture_output=True, text=True, check=True).stdout
    for e in ENTRY:
        assert e not in syms


def test_bindings_prototype_the_entry_points(trace_lib):
    from rlshaders_amd import _capi as capi, trace
    sq = C.POINTER(trace.ShadowQueue_)
    want = {"rls_trace_shadow_scratch_bytes": (4, None), "rls_trace_ggx_direct_emit": (11, 10),
            "rls_trace_disney_direct_emit": (10, 9), "rls_trace_ggx_direct_resolve": (11, 7),
            "rls_trace_disney_direct_resolve": (9, 5)}
    lib = trace.load()
    for e, (nargs, qat) in want.items():
        restype, argtypes = trace.PROTOTYPES[e]
        assert restype is C.c_int and len(argtypes) == nargs, e
        if qat is not None:
            assert argtypes[qat] == sq, e
        assert getattr(lib, e).argtypes == argtypes
    assert trace.PROTOTYPES["rls_trace_ggx_direct_emit"][1][3] == C.POINTER(capi.GgxShader)
    for f in (trace.ggx_shadow_rays, trace.disney_shadow_rays, trace.ShadowQueue, trace.ggx_shader):
        assert callable(f)
    out = subprocess.run(["nm", "-D", "--defined-only", str(trace_lib)], capture_output=True, text=True, check=True).stdout
    for e in ENTRY:
        assert f" T {e}" in out


def test_struct_layout_matches_the_header(tmp_path):
    from rlshaders_amd import trace
    py = trace.ShadowQueue_
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "rlshaders_amd_trace.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(rls_shadow_queue));']
    for f, _ in py._fields_:
        lines.append(f'  printf("{f} %zu\\n", offsetof(rls_shadow_queue, {f}));')
    lines += ['  printf("bits %d %d %d %d\\n", RLS_SHADOW_LIGHT_MASK, RLS_SHADOW_BSDF, RLS_SHADOW_SPECULAR, RLS_SHADOW_DIFFUSE);',
              '  return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    got = [l for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if l]
    want = [f"size {C.sizeof(py)}"] + [f"{f} {getattr(py, f).offset}" for f, _ in py._fields_]
    want.append(f"bits {trace.RLS_SHADOW_LIGHT_MASK} {trace.RLS_SHADOW_BSDF} {trace.RLS_SHADOW_SPECULAR} {trace.RLS_SHADOW_DIFFUSE}")
    assert got == want


def test_scratch_bytes_and_its_argument_checks(trace_lib):
    """no device needed: the staging of n points is 10 float planes and a 32-bit tag per slot, n_lights * 3 * spp_n^2 slots a
    point, plus the scan's tile sums; the documented refusals"""
    from rlshaders_amd import trace
    lib = trace.load()
    b = C.c_size_t()
    for n, nl, spp_n in ((1, 1, 1), (1000, 2, 4), (5, 8, 16), (0, 3, 2)):
        assert lib.rls_trace_shadow_scratch_bytes(n, nl, spp_n, C.byref(b)) == 0
        slots = n * nl * 3 * spp_n * spp_n
        assert 11 * 4 * slots <= b.value <= 11 * 4 * slots + 12 * 256 + 8 * (n // 2048 + 1)
        assert trace.shadow_scratch_bytes(n, nl, spp_n) == b.value
    for args in ((-1, 1, 1), (1, 0, 1), (1, 9, 1), (1, 1, 0), (1, 1, 17)):
        assert lib.rls_trace_shadow_scratch_bytes(*args, C.byref(b)) == 1, args
    assert lib.rls_trace_shadow_scratch_bytes(1, 1, 1, None) == 1
    # the entry points refuse a NULL context before anything else
    q = trace.ShadowQueue_()
    from rlshaders_amd import _capi as capi
    assert lib.rls_trace_disney_direct_emit(None, 1, None, capi.CVec3(), None, 1, 1, 0, 0, C.byref(q)) == 1
    assert lib.rls_trace_ggx_direct_resolve(None, 1, None, None, None, 1, 1, C.byref(q), capi.CRgb(), capi.Rgb(), capi.Rgb()) == 1
