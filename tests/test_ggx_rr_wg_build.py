"""CPU: the companion code object of BASELINE config 2 (rlshaders_amd/csrc_rr/ -> librls_ggx_rr.so) builds for gfx950 through
rlshaders_amd/build.py and through CMake, exports its launcher and nothing else, and is optional: the product library loads
and resolves every header symbol without it.  And the inputs of tests/test_gpu_ggx_rr_wg.py hold the request counts they
are named after, decided in float64 away from the thresholds and confirmed on the oracle's microfacet normals.
(That the product library's device code is still the frozen one: tests/test_profile_binding.py.)"""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rr_wg_util as U

ROOT = Path(__file__).resolve().parent.parent
LAUNCHER = "rls_ggx_rr_wg_launch"


def _functions(lib):
    """the functions a shared library defines and exports (beside them it holds two objects every HIP unit built from
    rls_internal.hpp holds: the unit's __hip_cuid_* byte and the thread-local of rlsh::pending_device_error)"""
    out = subprocess.run(["readelf", "--dyn-syms", "-W", str(lib)], capture_output=True, text=True, check=True).stdout
    rows = [l.split() for l in out.splitlines()]
    return sorted(r[7].split("@")[0] for r in rows if len(r) == 8 and r[3] in ("FUNC", "IFUNC") and r[6] != "UND")


@pytest.fixture(scope="module")
def built():
    from rlshaders_amd import build
    build.build_library()
    return build


def test_build_library_builds_the_companion(built):
    assert built.RR_LIB.exists() and built.RR_LIB.parent == built.LIB.parent
    assert _functions(built.RR_LIB) == [LAUNCHER]
    dyn = subprocess.run(["readelf", "-d", str(built.RR_LIB)], capture_output=True, text=True, check=True).stdout
    assert "librlshaders_amd.so" in dyn and "$ORIGIN" in dyn
    from rlshaders_amd.codeid import DeviceCode
    dc = DeviceCode(built.RR_LIB)
    assert len(dc.units) == 1 and dc.kernel_id("ggx_rr_wg_kernel") is not None        # one gfx950 code object, the kernel in it
    assert DeviceCode(built.LIB).kernel_id("ggx_rr_wg_kernel") is None                  # and not in the product library
    # the product library declares nothing new and imports the loader's calls it finds the companion with
    und = subprocess.run(["nm", "-D", "--undefined-only", str(built.LIB)], capture_output=True, text=True, check=True).stdout
    assert "dladdr" in und and "dlopen" in und
    assert LAUNCHER not in (ROOT / "include" / "rlshaders_amd.h").read_text()


def test_frozen_units_do_not_include_the_companions_header():
    for p in (ROOT / "rlshaders_amd" / "csrc").iterdir():
        assert "rls_rr_device.hpp" not in p.read_text(), p
    assert "vndf_microfacet_pair_wg" not in (ROOT / "rlshaders_amd" / "csrc" / "rls_device.hpp").read_text()


def test_product_library_stands_without_the_companion(built, tmp_path):
    """a copy of lib/ without librls_ggx_rr.so: the product library loads and every header symbol resolves"""
    from test_capi_symbols import declared_symbols
    lib = tmp_path / "lib"
    lib.mkdir()
    shutil.copy(built.LIB, lib / built.LIB.name)
    assert not (lib / built.RR_LIB.name).exists()
    h = C.CDLL(str(lib / built.LIB.name))
    names = declared_symbols()
    assert len(names) >= 40
    for nm in names:
        assert hasattr(h, nm), nm
    h.rls_version.restype = C.c_int
    assert h.rls_version() > 0


def test_cmake_builds_the_companion():
    """the tree tests/test_cmake_build.py builds (incremental): the companion beside the product, the same device code"""
    if shutil.which("cmake") is None:
        pytest.skip("cmake is not installed")
    import test_cmake_trace as T
    gen = ["-G", "Ninja"] if shutil.which("ninja") else []
    T._run(["cmake", "-S", str(ROOT), "-B", str(T.BUILD), *gen])
    T._run(["cmake", "--build", str(T.BUILD), "-j", "6"])
    lib = T.BUILD / "librls_ggx_rr.so"
    assert lib.exists() and (T.BUILD / "librlshaders_amd.so").exists()
    assert _functions(lib) == [LAUNCHER]
    assert "librlshaders_amd.so" in T._run(["readelf", "-d", str(lib)])
    from rlshaders_amd import build
    from rlshaders_amd.codeid import DeviceCode
    assert DeviceCode(lib).library_id == DeviceCode(build.RR_LIB).library_id             # the same device code as build.py's


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------
def _oracle_takes_the_fallback(oracle, c, x):
    """per sample: the oracle's microfacet normal IS the uniform fallback's (float64 restatement, 1e-5)"""
    from gpu_util_cpu import ggx_oracle
    og = ggx_oracle(oracle, c)
    out = []
    for rx, ry in ((x[0], x[1]), (x[2], x[3])):
        m = og.microfacet(rx, ry).astype(np.float64)
        out.append(np.linalg.norm(m - U.uniform_microfacet(c, rx, ry), axis=0) < 1e-5)
    return out


@pytest.mark.parametrize("layout", sorted(U.LAYOUTS))
@pytest.mark.parametrize("name", sorted(U.RECIPES))
def test_recipes_hold_the_request_counts_they_name(oracle, name, layout):
    c, x = U.recipe(name, layout)
    n, off = U.LAYOUTS[layout]
    n1, n2, _, _ = U.requests(c, x)
    want = np.zeros(n, bool)
    want[off + np.array(U.RECIPES[name], int)] = True
    assert np.array_equal(n1, want) and np.array_equal(n2, want)                       # a near-normal point: both samples
    assert U.margin(c, x) >= 2.0
    o1, o2 = _oracle_takes_the_fallback(oracle, c, x)
    assert np.array_equal(o1, want) and np.array_equal(o2, want)
    per_tile = U.per_tile_requests(c, x)
    assert per_tile.sum() == 2 * len(U.RECIPES[name])
    if layout == "tile":
        assert list(per_tile) == [{"none": 0, "one": 2, "n32": 64, "n33": 66, "all": 512, "first_wave": 128, "last_wave": 128}[name]]
        per_wave = (n1.astype(int) + n2).reshape(4, 64).sum(1)
        if name == "first_wave":
            assert list(per_wave) == [128, 0, 0, 0]
        if name == "last_wave":
            assert list(per_wave) == [0, 0, 0, 128]
    else:
        assert per_tile[0] > 0 or name in ("none", "one", "last_wave")
        if name in ("n32", "n33", "all"):
            assert per_tile[0] > 0 and per_tile[1] > 0                                  # the requests straddle the two tiles


@pytest.mark.parametrize("sample", [0, 1])
def test_rx_zero_requests_one_sample_only(oracle, sample):
    c, x = U.rx_zero(sample)
    n1, n2, flat, _ = U.requests(c, x)
    hit = np.zeros(x.shape[1], bool)
    hit[::3] = True
    assert not flat.any()
    assert np.array_equal(n2 if sample else n1, hit) and not (n1 if sample else n2).any()
    o = _oracle_takes_the_fallback(oracle, c, x)
    assert np.array_equal(o[sample], hit) and not o[1 - sample].any()


def test_mixed_batch_is_what_the_sizing_assumed():
    """the benchmark's inputs (cases.ggx_mixed): a few per cent of the points request, nearly every tile holds a request and
    none holds more than one pass serves"""
    c, x = U.mixed(1 << 16)
    per_tile = U.per_tile_requests(c, x)
    assert 20 <= per_tile.mean() <= 40 and per_tile.max() <= 64 and (per_tile > 0).mean() > 0.99


def test_rounds_batch_alternates_tiles_with_and_without_requests():
    n = 64 * U.TILE
    c, x = U.mixed(n, first=1 << 33)
    tile = np.arange(n) // U.TILE
    quiet = (tile % 3 == 1) | (tile % 8 == 6)
    U._quiet(c, x, quiet)
    per_tile = U.per_tile_requests(c, x)
    assert (per_tile[quiet[::U.TILE]] == 0).all() and (per_tile[~quiet[::U.TILE]] > 0).all()
