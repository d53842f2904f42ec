"""CPU: the CMake build carries the any-hit companion library (librls_nearest_any.so, include/rlshaders_amd_nearest_any.h): it
builds for gfx950 beside the other libraries, exports exactly the rls_nearest_any_* symbols its header declares, links the
product alone, installs with its header and the C++ mirror, and an outside project links rlshaders_amd::nearest_any.  After
tests/test_cmake_nearest_group.py: the same build tree, built incrementally; the four other nearest libraries keep their exports."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BUILD = ROOT / "rlshaders_amd" / "build" / "cmake"          # the tree tests/test_cmake_build.py builds (incremental)
PREFIX = ROOT / "rlshaders_amd" / "build" / "cmake_nearest_any_prefix"

CONSUMER = """cmake_minimum_required(VERSION 3.21)
project(rls_nearest_any_consumer LANGUAGES CXX)
find_package(rlshaders_amd REQUIRED)
add_executable(consumer ${RLS_EXAMPLE_SOURCE})
set_target_properties(consumer PROPERTIES CXX_STANDARD 14 CXX_STANDARD_REQUIRED ON)
target_link_libraries(consumer PRIVATE rlshaders_amd::nearest_any rlshaders_amd::shadow_walk)
"""


def _run(cmd, **kw):
    p = subprocess.run(cmd, capture_output=True, text=True, **kw)
    assert p.returncode == 0, f"{' '.join(map(str, cmd))}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    return p.stdout


@pytest.fixture(scope="module")
def built():
    if shutil.which("cmake") is None:
        pytest.skip("cmake is not installed")
    gen = ["-G", "Ninja"] if shutil.which("ninja") else []
    _run(["cmake", "-S", str(ROOT), "-B", str(BUILD), *gen])
    _run(["cmake", "--build", str(BUILD), "-j", str(min(6, os.cpu_count() or 2))])
    shutil.rmtree(PREFIX, ignore_errors=True)
    _run(["cmake", "--install", str(BUILD), "--prefix", str(PREFIX)])
    return BUILD


def test_companion_builds_and_exports_its_header(built):
    from nearest_abi_util import declared_symbols as nearest_declared, exported_symbols
    from nearest_rebuild_util import declared_symbols as rebuild_declared
    from nearest_refit_util import declared_symbols as refit_declared
    from test_nearest_any_abi import declared_symbols
    from test_nearest_group_abi import declared_symbols as group_declared
    lib = built / "librls_nearest_any.so"
    assert lib.exists()
    assert exported_symbols(lib) == declared_symbols() and len(declared_symbols()) == 3
    needed = _run(["readelf", "-d", str(lib)])
    assert "librlshaders_amd.so" in needed and "$ORIGIN" in needed
    for other in ("librls_trace", "librls_walk", "librls_shadow_walk", "librls_nearest.so", "librls_nearest_refit", "librls_nearest_rebuild",
                  "librls_nearest_group"):
        assert other not in needed, other
    assert exported_symbols(built / "librls_nearest.so") == nearest_declared()
    assert exported_symbols(built / "librls_nearest_refit.so") == refit_declared()
    assert exported_symbols(built / "librls_nearest_rebuild.so") == rebuild_declared()
    assert exported_symbols(built / "librls_nearest_group.so") == group_declared()
    assert (built / "example_nearest_any").exists()
    # the same device code as the Python-driven build: sources and flags alone decide it
    from rlshaders_amd import build
    from rlshaders_amd.codeid import DeviceCode
    assert DeviceCode(lib).library_id == DeviceCode(build.build_nearest_any_library()).library_id


def test_install_and_outside_consumer(built, tmp_path):
    for rel in ("include/rlshaders_amd_nearest_any.h", "include/rlshaders_amd_nearest.h", "include/rlshaders_amd_walk.h",
                "include/rls_nearest_any.hpp", "include/rls_nearest.hpp", "include/rls_trace.hpp",
                "lib/librls_nearest_any.so", "lib/librls_nearest.so", "lib/librls_shadow_walk.so", "lib/librlshaders_amd.so"):
        assert (PREFIX / rel).exists(), rel
    src = tmp_path / "src"
    src.mkdir()
    (src / "CMakeLists.txt").write_text(CONSUMER)
    gen = ["-G", "Ninja"] if shutil.which("ninja") else []
    _run(["cmake", "-S", str(src), "-B", str(tmp_path / "b"), *gen, f"-DCMAKE_PREFIX_PATH={PREFIX}",
          f"-DRLS_EXAMPLE_SOURCE={ROOT / 'rlshaders_amd' / 'host' / 'example_nearest_any.cpp'}"])
    _run(["cmake", "--build", str(tmp_path / "b")])
    exe = tmp_path / "b" / "consumer"
    assert exe.exists()
    needed = _run(["readelf", "-d", str(exe)])
    assert "librls_nearest_any.so" in needed and "librls_nearest.so" in needed and "librlshaders_amd.so" in needed
