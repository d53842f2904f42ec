"""CPU: the caller-traced rlDisney integrator in the companion library (rls_trace_disney_emit, librls_trace.so).

Both code objects carry its emit kernels, one family per lobe and lane-group width (EXACT <G, 0>, FAST <G, 1>); the product
library carries none of them; the Python bindings prototype the entry point.  tests/native/trace_disney_checks.cpp runs its
argument checks with dummy planes and no GPU, in both math modes: statuses, message texts, and that a passing argument set
reaches the launch (RLS_ERR_HIP).  Like tests/test_argument_checks.py it skips where torch sees a GPU."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "native" / "trace_disney_checks.cpp"
GROUPS = (1, 4, 16, 64)
FAMILIES = ("disney_diffuse_emit_kernel", "disney_specular_emit_kernel")


@pytest.fixture(scope="module")
def trace_lib():
    from rlshaders_amd import build
    return build.build_trace_library()


def test_both_code_objects_carry_every_disney_emit_kernel(trace_lib):
    from rlshaders_amd.codeid import DeviceCode, code_objects, fatbin
    objs = code_objects(fatbin(trace_lib))
    assert len(objs) == 2
    dc = DeviceCode(trace_lib)
    units = set()
    for fast in (0, 1):
        for fam in FAMILIES:
            for g in GROUPS:
                u = dc.unit_of_kernel(f"{fam}<{g}, {fast}>")
                assert u is not None, (fam, g, fast)
                units.add((fast, u))
    # the EXACT kernels in one code object, the FAST ones in the other
    assert len({u for f, u in units if f == 0}) == 1 and len({u for f, u in units if f == 1}) == 1
    assert {u for f, u in units if f == 0} != {u for f, u in units if f == 1}


def test_no_disney_emit_kernel_in_the_product_library(trace_lib):
    from rlshaders_amd import build
    from rlshaders_amd.codeid import code_objects, fatbin
    for elf in code_objects(fatbin(build.build_library())):
        for fam in FAMILIES:
            assert fam.encode() not in elf, fam
    syms = subprocess.run(["nm", "-D", "--defined-only", str(build.LIB)], capture_output=True, text=True, check=True).stdout
    assert "rls_trace_disney_emit" not in syms


def test_bindings_prototype_the_disney_emit(trace_lib):
    import ctypes as C
    from rlshaders_amd import _capi as capi, trace
    restype, argtypes = trace.PROTOTYPES["rls_trace_disney_emit"]
    assert restype is C.c_int
    assert argtypes[2] == C.POINTER(capi.DisneyClosure) and len(argtypes) == 9
    lib = trace.load()
    assert lib.rls_trace_disney_emit.argtypes == argtypes
    assert callable(trace.disney_rays)
    out = subprocess.run(["nm", "-D", "--defined-only", str(trace_lib)], capture_output=True, text=True, check=True).stdout
    assert " T rls_trace_disney_emit" in out


@pytest.fixture(scope="module")
def cases(tmp_path_factory, trace_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the driver hands dummy planes to the entry point")
    from rlshaders_amd import build
    exe = tmp_path_factory.mktemp("trace_disney_checks") / "trace_disney_checks"
    cmd = [build._hipcc(), "-std=c++17", "-O1", "-x", "hip", "--offload-host-only", "-Wall", "-DRLS_FAST=0", str(DRIVER),
           "-o", str(exe), f"-L{build.LIBDIR}", "-lrls_trace", "-lrlshaders_amd", f"-Wl,-rpath,{build.LIBDIR}"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    rows = []
    for line in p.stdout.splitlines():
        what, fast, status, want, text, message = line.split("\t")
        rows.append(dict(what=what, fast=int(fast), status=int(status), want=int(want), text=text, message=message))
    return rows


def test_argument_checks_in_both_modes(cases):
    for fast in (0, 1):
        mine = [c for c in cases if c["fast"] == fast]
        assert len(mine) >= 30
        assert {c["what"] for c in mine} >= {"valid, diffuse", "valid, glossy", "lobe 0", "spp_n 0", "spp_n 17", "n < 0",
                                            "queue NULL", "queue.offsets NULL", "queue.dir NULL", "queue.weight.g NULL",
                                            "closure NULL", "wo NULL", "queue.capacity short", "queue.scratch NULL",
                                            "queue.scratch short", "n == 0"}
    wrong = []
    for c in cases:
        ok = c["status"] == c["want"]
        if ok and c["want"] == 1:                           # RLS_ERR_INVALID_ARGUMENT: "emit: <text>"
            prefix, _, text = c["message"].partition(": ")
            ok = prefix == "emit" and text == c["text"]
        elif ok and c["want"] == 3:                         # RLS_ERR_HIP: every check passed, the launch found no device
            ok = c["message"].startswith("HIP error ")
        if not ok:
            wrong.append(f'{c["what"]} [fast={c["fast"]}]: status {c["status"]} "{c["message"]}", '
                         f'want {c["want"]} "{c["text"]}"')
    assert not wrong, "\n".join(wrong)
