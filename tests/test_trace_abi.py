"""CPU: the companion library of the caller-traced rlGgx integrators (include/rlshaders_amd_trace.h, librls_trace.so).

Its header is C99 / C++14 clean; the library builds for gfx950 and exports exactly the rls_trace_* symbols the header
declares, each bound in rlshaders_amd/trace.py; building it leaves the product library's device code -- frozen,
tests/test_profile_binding.py -- as it is, and none of its kernels is in the product library."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "rlshaders_amd_trace.h"
TRACE_KERNELS = ("ggx_glossy_emit_kernel", "ggx_refract_emit_kernel", "trace_scan_block_kernel", "trace_scan_totals_kernel",
                 "trace_scan_add_kernel", "trace_compact_kernel", "trace_resolve_kernel")


def declared_trace_symbols():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(rls_[a-z0-9_]+)\s*\(", text)))


def exported_trace_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("rls_"))


@pytest.fixture(scope="module")
def trace_lib():
    from rlshaders_amd import build
    return build.build_trace_library()


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_trace.h"\n'
                   'int main(void){ rls_ray_queue q = {0}; size_t b = 0; (void)q;\n'
                   '  return rls_trace_scratch_bytes(1, 1, &b) == RLS_OK && RLS_RAY_TIR_MIRROR == 1 ? 0 : 1; }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{ROOT / 'include'}",
                            "-x", "c" if cc == "gcc" else "c++", str(src)], capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)


def test_exports_exactly_the_header_and_the_bindings(trace_lib):
    from rlshaders_amd import trace
    declared = declared_trace_symbols()
    assert declared and all(s.startswith("rls_trace_") for s in declared), declared
    assert exported_trace_symbols(trace_lib) == declared
    assert sorted(trace.PROTOTYPES) == declared
    trace.load()          # binds every prototype (no device needed)


def test_not_in_the_drop_in_surface():
    """the 82-entry drop-in header and its ctypes prototypes are left alone"""
    from rlshaders_amd import _capi
    from test_capi_symbols import declared_symbols
    assert not [s for s in declared_symbols() if s.startswith("rls_trace_")]
    assert not [s for s in _capi.PROTOTYPES if s.startswith("rls_trace_")]
    assert "rlshaders_amd_trace.h" not in (ROOT / "include" / "rlshaders_amd.h").read_text()


def test_code_objects_are_gfx950(trace_lib):
    from rlshaders_amd.codeid import DeviceCode, code_objects, fatbin
    objs = code_objects(fatbin(trace_lib))
    assert len(objs) == 2                       # the EXACT and FAST units
    for elf in objs:
        assert b"gfx950" in elf
    dc = DeviceCode(trace_lib)
    for k in ("ggx_glossy_emit_kernel<1, 0>", "ggx_glossy_emit_kernel<64, 1>", "ggx_refract_emit_kernel<4, 0>",
              "ggx_refract_emit_kernel<16, 1>", "trace_resolve_kernel<3>", "trace_compact_kernel<1>"):
        assert dc.unit_of_kernel(k) is not None, k


def test_links_the_product_library_by_origin(trace_lib):
    d = subprocess.run(["readelf", "-d", str(trace_lib)], capture_output=True, text=True, check=True).stdout
    assert "[librlshaders_amd.so]" in d and "$ORIGIN" in d


def test_product_library_is_unchanged(trace_lib):
    import json
    from rlshaders_amd import build
    from rlshaders_amd.codeid import DeviceCode
    main = DeviceCode(build.build_library())
    recorded = json.loads((ROOT / "profiles" / "r06_library_id.json").read_text())
    assert main.library_id == recorded["library_id"]
    from rlshaders_amd.codeid import code_objects, fatbin
    objs = code_objects(fatbin(build.LIB))
    assert len(objs) >= 12
    for elf in objs:
        for k in TRACE_KERNELS:
            assert k.encode() not in elf, k
    syms = subprocess.run(["nm", "-D", "--defined-only", str(build.LIB)], capture_output=True, text=True, check=True).stdout
    assert "rls_trace_" not in syms
