"""CPU: the caller-traced rlSss integrator in the companion library (rls_trace_sss_probe_emit / rls_trace_sss_scatter_resolve,
librls_trace.so).

Both code objects carry its two kernels (EXACT <0>, FAST <1>); the product library carries neither; the Python bindings
prototype both entry points and the structs have the header's layout.  tests/native/trace_sss_checks.cpp runs their
argument checks with dummy planes and no GPU, in both math modes: statuses, message texts, and that a passing argument set
reaches the launch (RLS_ERR_HIP).  Like tests/test_argument_checks.py it skips where torch sees a GPU."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "native" / "trace_sss_checks.cpp"
KERNELS = ("sss_probe_emit_kernel", "sss_scatter_resolve_kernel")
ENTRY = ("rls_trace_sss_probe_emit", "rls_trace_sss_scatter_resolve")


@pytest.fixture(scope="module")
def trace_lib():
    from rlshaders_amd import build
    return build.build_trace_library()


def test_both_code_objects_carry_the_sss_kernels(trace_lib):
    from rlshaders_amd.codeid import DeviceCode, code_objects, fatbin
    assert len(code_objects(fatbin(trace_lib))) == 2
    dc = DeviceCode(trace_lib)
    units = {}
    for fast in (0, 1):
        for k in KERNELS:
            u = dc.unit_of_kernel(f"{k}<{fast}>")
            assert u is not None, (k, fast)
            units.setdefault(fast, set()).add(u)
    # the EXACT kernels in one code object, the FAST ones in the other
    assert len(units[0]) == 1 and len(units[1]) == 1 and units[0] != units[1]


def test_no_sss_trace_kernel_in_the_product_library(trace_lib):
    from rlshaders_amd import build
    from rlshaders_amd.codeid import code_objects, fatbin
    for elf in code_objects(fatbin(build.build_library())):
        for k in KERNELS:
            assert k.encode() not in elf, k
    syms = subprocess.run(["nm", "-D", "--defined-only", str(build.LIB)], capture_output=True, text=True, check=True).stdout
    for e in ENTRY:
        assert e not in syms


def test_bindings_prototype_the_sss_entry_points(trace_lib):
    import ctypes as C
    from rlshaders_amd import _capi as capi, trace
    restype, argtypes = trace.PROTOTYPES["rls_trace_sss_probe_emit"]
    assert restype is C.c_int and len(argtypes) == 8
    assert argtypes[2] == C.POINTER(capi.SssClosure) and argtypes[7] == C.POINTER(trace.ProbeQueue_)
    restype, argtypes = trace.PROTOTYPES["rls_trace_sss_scatter_resolve"]
    assert restype is C.c_int and len(argtypes) == 11
    assert argtypes[5] == C.POINTER(trace.ProbeQueue_) and argtypes[6] == C.POINTER(trace.ProbeHits_)
    lib = trace.load()
    for e in ENTRY:
        assert getattr(lib, e).argtypes == trace.PROTOTYPES[e][1]
    assert callable(trace.sss_probe_rays)
    out = subprocess.run(["nm", "-D", "--defined-only", str(trace_lib)], capture_output=True, text=True, check=True).stdout
    for e in ENTRY:
        assert f" T {e}" in out


def test_struct_layouts_match_the_header(tmp_path):
    """offsetof / sizeof of rls_probe_queue and rls_probe_hits in C against the ctypes mirrors"""
    from rlshaders_amd import trace
    fields = {"rls_probe_queue": trace.ProbeQueue_, "rls_probe_hits": trace.ProbeHits_}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "rlshaders_amd_trace.h"', 'int main(void) {']
    for cname, py in fields.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines += ['  printf("max %d\\n", RLS_MAX_PROBE_HITS);', '  return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    want = []
    for cname, py in fields.items():
        want.append(f"{cname} size {C_sizeof(py)}")
        for f, _ in py._fields_:
            want.append(f"{cname} {f} {getattr(py, f).offset}")
    want.append(f"max {trace.RLS_MAX_PROBE_HITS}")
    assert [l for l in got if l] == want


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


@pytest.fixture(scope="module")
def cases(tmp_path_factory, trace_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the driver hands dummy planes to the entry points")
    from rlshaders_amd import build
    exe = tmp_path_factory.mktemp("trace_sss_checks") / "trace_sss_checks"
    cmd = [build._hipcc(), "-std=c++17", "-O1", "-x", "hip", "--offload-host-only", "-Wall", "-DRLS_FAST=0", str(DRIVER),
           "-o", str(exe), f"-L{build.LIBDIR}", "-lrls_trace", "-lrlshaders_amd", f"-Wl,-rpath,{build.LIBDIR}"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    rows = []
    for line in p.stdout.splitlines():
        verb, what, fast, status, want, text, message = line.split("\t")
        rows.append(dict(verb=verb, what=what, fast=int(fast), status=int(status), want=int(want), text=text,
                         message=message))
    return rows


def test_argument_checks_in_both_modes(cases):
    for fast in (0, 1):
        emits = {c["what"] for c in cases if c["fast"] == fast and c["verb"] == "emit"}
        resolves = {c["what"] for c in cases if c["fast"] == fast and c["verb"] == "resolve"}
        assert emits >= {"valid", "spp_n 0", "spp_n 17", "queue NULL", "queue.origin NULL", "queue.maxdist NULL",
                         "queue.capacity short", "closure NULL", "N NULL", "P NULL", "n == 0"}
        assert resolves >= {"valid", "spp_n 0", "spp_n 17", "max_hits 0", "max_hits 13", "hits NULL", "hits.stride short",
                            "hits.count NULL", "hits.irradiance NULL", "queue.capacity short", "result NULL", "n == 0"}
    wrong = []
    for c in cases:
        ok = c["status"] == c["want"]
        entry = "rls_trace_sss_probe_emit" if c["verb"] == "emit" else "rls_trace_sss_scatter_resolve"
        if ok and c["want"] == 1:                           # RLS_ERR_INVALID_ARGUMENT: "<entry point>: <text>"
            prefix, _, text = c["message"].partition(": ")
            ok = prefix == entry and text == c["text"]
        elif ok and c["want"] == 3:                         # RLS_ERR_HIP: every check passed, the launch found no device
            ok = c["message"].startswith("HIP error ")
        if not ok:
            wrong.append(f'{c["verb"]} {c["what"]} [fast={c["fast"]}]: status {c["status"]} "{c["message"]}", '
                         f'want {c["want"]} "{c["text"]}"')
    assert not wrong, "\n".join(wrong)
