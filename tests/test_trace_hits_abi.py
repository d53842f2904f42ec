"""CPU: the caller-traced shading of rlSss's probe hits in the companion library (rls_trace_sss_hits_scratch_bytes /
rls_trace_sss_hits_emit / rls_trace_sss_hits_resolve, librls_trace.so).

The header declares the three entry points and rls_hit_queues; the built library exports them and both code objects carry the
math-mode kernels (EXACT <0>, FAST <1>), the product library none; the Python bindings prototype them and the ctypes struct has
the header's layout (sizeof / offsetof from a compiled probe); the scratch-size verb, which needs no device, checks its
arguments and sizes its parts."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "rlshaders_amd_trace.h"
MODE_KERNELS = ("sss_hits_gate_kernel", "sss_hits_emit_kernel")
PLAIN_KERNELS = ("sss_hits_list_kernel", "hits_compact_kernel", "sss_hits_fill_kernel", "sss_hits_resolve_kernel")
ENTRY = ("rls_trace_sss_hits_scratch_bytes", "rls_trace_sss_hits_emit", "rls_trace_sss_hits_resolve")
INVALID = 1


@pytest.fixture(scope="module")
def trace_lib():
    from rlshaders_amd import build
    return build.build_trace_library()


def test_header_declares_the_entry_points_and_the_struct():
    text = HEADER.read_text()
    for e in ENTRY:
        assert re.search(rf"^rls_status {e}\(", text, re.M), e
    m = re.search(r"typedef struct rls_hit_queues \{(.*?)\} rls_hit_queues;", text, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = re.findall(r"(\w+)\s*;", body)
    assert names == ["hit_capacity", "hit_count", "hit_element", "shadow", "diffuse", "scratch", "scratch_bytes"]
    assert "rls_shadow_queue shadow" in body and "rls_ray_queue diffuse" in body


def test_library_exports_and_kernels(trace_lib):
    from rlshaders_amd import build
    from rlshaders_amd.codeid import DeviceCode, code_objects, fatbin
    out = subprocess.run(["nm", "-D", "--defined-only", str(trace_lib)], capture_output=True, text=True, check=True).stdout
    for e in ENTRY:
        assert f" T {e}" in out, e
    dc = DeviceCode(trace_lib)
    units = {0: set(), 1: set()}
    for fast in (0, 1):
        u = dc.unit_of_kernel(f"sss_hits_gate_kernel<{fast}>")
        assert u is not None, fast
        units[fast].add(u)
        for g in (1, 4, 16, 64):
            u = dc.unit_of_kernel(f"sss_hits_emit_kernel<{g}, {fast}>")
            assert u is not None, (g, fast)
            units[fast].add(u)
    assert len(units[0]) == 1 and len(units[1]) == 1 and units[0] != units[1]
    for k in PLAIN_KERNELS:                                         # the mode-free kernels: the EXACT unit alone
        assert dc.unit_of_kernel(k) == next(iter(units[0])), k
    syms = subprocess.run(["nm", "-D", "--defined-only", str(build.build_library())], capture_output=True, text=True,
                          check=True).stdout
    for e in ENTRY:
        assert e not in syms
    for elf in code_objects(fatbin(build.LIB)):
        for k in MODE_KERNELS + PLAIN_KERNELS:
            assert k.encode() not in elf, k


def test_bindings_prototype_the_entry_points(trace_lib):
    from rlshaders_amd import _capi as capi, trace
    restype, argtypes = trace.PROTOTYPES["rls_trace_sss_hits_scratch_bytes"]
    assert restype is C.c_int and len(argtypes) == 7
    restype, argtypes = trace.PROTOTYPES["rls_trace_sss_hits_emit"]
    assert restype is C.c_int and len(argtypes) == 16
    assert argtypes[2] == C.POINTER(capi.SssClosure) and argtypes[5] == C.POINTER(trace.ProbeQueue_)
    assert argtypes[6] == C.POINTER(trace.ProbeHits_) and argtypes[7] is capi.CVec3 and argtypes[15] == C.POINTER(trace.HitQueues_)
    restype, argtypes = trace.PROTOTYPES["rls_trace_sss_hits_resolve"]
    assert restype is C.c_int and len(argtypes) == 10
    assert argtypes[1] == C.POINTER(trace.ProbeHits_) and argtypes[6] == C.POINTER(trace.HitQueues_)
    lib = trace.load()
    for e in ENTRY:
        assert getattr(lib, e).argtypes == trace.PROTOTYPES[e][1]
    assert callable(trace.sss_hit_rays) and callable(trace.HitQueues.resolve)


def test_struct_layout_matches_the_header(tmp_path):
    """offsetof / sizeof of rls_hit_queues (and the two queue structs it embeds) in C against the ctypes mirrors"""
    from rlshaders_amd import trace
    fields = {"rls_hit_queues": trace.HitQueues_, "rls_shadow_queue": trace.ShadowQueue_, "rls_ray_queue": trace.RayQueue_}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "rlshaders_amd_trace.h"', 'int main(void) {']
    for cname, py in fields.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines += ['  return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    want = []
    for cname, py in fields.items():
        want.append(f"{cname} size {C.sizeof(py)}")
        for f, _ in py._fields_:
            want.append(f"{cname} {f} {getattr(py, f).offset}")
    assert [l for l in got if l] == want


def test_scratch_bytes(trace_lib):
    """no device needed: the argument checks, and the parts the size is made of (each a multiple of 256 bytes; the staging grows
    with hit_capacity x n_lights x 2 x hit_spp_n^2 slots of five float planes and a 32-bit tag)"""
    from rlshaders_amd import trace
    lib = trace.load()
    b = C.c_size_t()
    sb = lib.rls_trace_sss_hits_scratch_bytes
    assert sb(67, 2, 3, 804, 2, 2, None) == INVALID
    for args in ((-1, 2, 3, 8, 2, 2), (67, 0, 3, 8, 2, 2), (67, 17, 3, 8, 2, 2), (67, 2, 0, 8, 2, 2), (67, 2, 13, 8, 2, 2),
                 (67, 2, 3, -1, 2, 2), (67, 2, 3, 8, -1, 2), (67, 2, 3, 8, 9, 2), (67, 2, 3, 8, 2, 0), (67, 2, 3, 8, 2, 17)):
        assert sb(*args, C.byref(b)) == INVALID, args
    size = lambda *a: trace.sss_hits_scratch_bytes(*a)
    a256 = lambda x: (x + 255) // 256 * 256
    for n, spp_n, cap, nl, hs in ((67, 2, 804, 2, 2), (0, 1, 0, 0, 1), (5000, 1, 100, 8, 4), (67, 2, 803, 0, 1)):
        rays, slots = n * spp_n * spp_n, cap * nl * 2 * hs * hs
        tiles = max((rays + 2047) // 2048, (cap + 2047) // 2048, 1)
        want = a256(rays * 2) + a256((rays + 1) * 8) + a256(tiles * 8) + 6 * a256(slots * 4) + 4 * a256(cap * 4) + a256(cap * 2)
        assert size(n, spp_n, 3, cap, nl, hs) == want, (n, spp_n, cap, nl, hs)
    assert size(67, 2, 3, 804, 2, 2) == size(67, 2, 12, 804, 2, 2)  # (the slots per ray do not enter: the mask is 16 bits)
