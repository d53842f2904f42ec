"""Build driver: compiles the HIP translation units under ``csrc/`` for gfx950 and links them
into ``rlshaders_amd/lib/librlshaders_amd.so`` (in-tree, so the library travels with the repo
snapshot to the GPU box).  hipcc cross-compiles without a GPU present.

Parity build flags: ``-ffp-contract=off`` and no fast-math (FMA contraction alone moves ~5 % of
chained GGX values past 1e-5 relative).  fp32 divide / sqrt stay correctly
rounded (hipcc default ``-fhip-fp32-correctly-rounded-divide-sqrt``).

The companion libraries beside the product (``librls_*.so``) are described once each in COMPANIONS and built by one function;
tests/test_build_commands.py holds every command line of this file to a recording.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import NamedTuple

PKG = Path(__file__).resolve().parent
CSRC = PKG / "csrc"
HOST = PKG / "host"
INCLUDE = PKG.parent / "include"
LIBDIR = PKG / "lib"
OBJDIR = PKG / "build"
LIB = LIBDIR / "librlshaders_amd.so"
ARCH = "gfx950"

# the largest units first (the thread pool starts them first); integrate / lights / scatter / shade share csrc/rls_loops.hpp
SOURCES = ["shade.hip", "integrate.hip", "lights.hip", "scatter.hip", "skin.hip", "ggx.hip", "disney.hip", "sss.hip", "alternates.hip", "context.hip", "pipeline.hip",
           "libm_check.hip"]
FAST_UNITS = {"ggx.hip", "disney.hip", "sss.hip", "skin.hip", "integrate.hip", "lights.hip", "scatter.hip", "shade.hip", "alternates.hip"}
HEADERS = [CSRC / "rls_device.hpp", CSRC / "rls_libm.hpp", CSRC / "rls_libm_tables.inc", CSRC / "rls_libm_flavour_args.inc", CSRC / "rls_internal.hpp", CSRC / "rls_loops.hpp",
           INCLUDE / "rlshaders_amd.h", INCLUDE / "rlshaders_amd_diag.h"]
# a unit's flavours: EXACT (carries the C ABI), FAST (kernels behind a hidden symbol)
EXACT, FAST = ("", "RLS_FAST=0"), ("_fast", "RLS_FAST=1")

HIPCC_FLAGS = [
    f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC",
    "-ffp-contract=off", "-fno-fast-math",
    # gfx950 issues v_pk_{mul,add}_f32 at half the rate of the scalar forms, and pairing operands costs
    # moves and registers: with SLP packing off config 2 runs 4 % (EXACT) / 6 % (FAST) faster; measured again in round 3 on the
    # n^2-spp loops (tools/ab.sh, packing ON against this default): rlDisney 64 spp +16 %, rlSkin shader_evaluate +25 %,
    # rlGgx shader_evaluate +7 %, its light loop +8 %, integrateScatter +2.5 % slower
    "-fno-slp-vectorize",
    "-fno-gpu-rdc",
    "-Wall", "-Wno-unused-function",
]
HOST_CXX = ["g++", "-std=c++14", "-O2", "-Wall"]


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the rlshaders_amd HIP library cannot be built")
    return exe


def _stale(target: Path, deps) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(Path(d).stat().st_mtime > t for d in deps)


def _run(cmd, verbose: bool, what: str = "hipcc failed"):
    if verbose:
        print(" ".join(cmd), flush=True)
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"{what}:\n{' '.join(cmd)}\n{p.stdout}\n{p.stderr}")
    return p


def _compile_and_link(jobs, lib: Path, objs, link_deps, link_flags, force: bool, verbose: bool) -> Path:
    """the stale objects compiled (in parallel), then the library linked if anything was, or if it is older than a dependency"""
    if jobs:
        with ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            list(ex.map(lambda cmd: _run(cmd, verbose), jobs))
    if force or jobs or _stale(lib, link_deps):
        _run([_hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(lib), *map(str, objs), *link_flags], verbose)
    return lib


def sources():
    return [CSRC / s for s in SOURCES if (CSRC / s).exists()]


def build_library(force: bool = False, verbose: bool = False, variant: str = "", defines=(), extra=()) -> Path:
    """Compile every HIP TU for gfx950 and link the C-ABI shared library.  Returns its path.

    ``variant`` / ``defines`` build an experiment flavour next to the product library
    (``librlshaders_amd_<variant>.so``, selected at run time with RLSHADERS_AMD_LIB)."""
    hipcc = _hipcc()
    LIBDIR.mkdir(exist_ok=True)
    objdir = OBJDIR if not variant else PKG / f"build_{variant}"
    lib = LIB if not variant else LIBDIR / f"librlshaders_amd_{variant}.so"
    objdir.mkdir(exist_ok=True)
    jobs = []
    objs = []
    for src in sources():
        # every closure unit twice
        for suffix, flag in [EXACT] + ([FAST] if src.name in FAST_UNITS else []):
            obj = objdir / (src.stem + suffix + ".o")
            objs.append(obj)
            if force or _stale(obj, [src, *HEADERS, Path(__file__)]):
                # -cuid: clang names one symbol per unit `__hip_cuid_<hash>` and by default hashes the PATHS on its command line
                # into it -- the same sources in another checkout or object directory then differ in that symbol's length now
                # and again, which can move a code object's layout by a cache line (rlshaders_amd/codeid.py).  A fixed id per
                # unit makes the device code a function of sources and flags alone.
                jobs.append([hipcc, *HIPCC_FLAGS, *extra, f"-cuid=rlshaders_amd.{src.stem}{suffix}", f"-D{flag}",
                             *[f"-D{d}" for d in defines], "-c", str(src), "-o", str(obj)])
    _compile_and_link(jobs, lib, objs, objs, [], force, verbose)
    if not variant:
        build_rr_library(force=force, verbose=verbose)
    return lib


# ---- the companion libraries: librls_<name>.so beside the product, so that the product's device code -- frozen,
# tests/test_profile_binding.py -- and each other's pinned surfaces stay what they are.  All are built alike: the product's
# flags, a fixed -cuid per unit and flavour (rls_<name>.<unit>[_fast]), objects under build/<objdir>/, linked against
# librlshaders_amd.so alone (contexts, errors, graphs) and found next to it ($ORIGIN) -- a name no build_library(variant=...)
# output can take.  What differs is one Companion each:
#   headers: what its units include beyond HEADERS -- an object is stale against its source, these and this file;
#   flavours: EXACT alone (a mode-free library: IEEE arithmetic) or EXACT and FAST;
#   after_product: build_library() is its prerequisite.  Not so for rr, which build_library() itself builds right after the
#     product (the product looks for it next to itself, so every caller of build_library() has it): it links the product as
#     it finds it.
class Companion(NamedTuple):
    name: str
    objdir: str
    csrc: Path
    units: list
    headers: list
    flavours: tuple = (EXACT,)
    after_product: bool = True

    @property
    def lib(self) -> Path:
        return LIBDIR / f"librls_{self.name}.so"


RR_CSRC, TRACE_CSRC, WALK_CSRC = PKG / "csrc_rr", PKG / "csrc_trace", PKG / "csrc_walk"
SHADOW_WALK_CSRC, NEAREST_CSRC = PKG / "csrc_shadow_walk", PKG / "csrc_nearest"
RR_HEADERS = [RR_CSRC / "rls_rr_device.hpp"]
TRACE_HEADERS = [*sorted(TRACE_CSRC.glob("*.hpp")), INCLUDE / "rlshaders_amd_trace.h"]
WALK_HEADERS = [*sorted(WALK_CSRC.glob("*.hpp")), INCLUDE / "rlshaders_amd_walk.h"]
SHADOW_WALK_HEADERS = [*sorted(SHADOW_WALK_CSRC.glob("*.hpp")), INCLUDE / "rlshaders_amd_shadow_walk.h", INCLUDE / "rlshaders_amd_walk.h"]
NEAREST_HEADERS = [NEAREST_CSRC / "rls_nearest_device.hpp", NEAREST_CSRC / "rls_nearest_bvh.hpp", NEAREST_CSRC / "rls_nearest_scene.hpp",
                   INCLUDE / "rlshaders_amd_nearest.h", INCLUDE / "rlshaders_amd_walk.h", INCLUDE / "rlshaders_amd_trace.h"]
NEAREST_REFIT_HEADERS = [NEAREST_CSRC / "rls_nearest_refit.hpp", NEAREST_CSRC / "rls_nearest_update.hpp", INCLUDE / "rlshaders_amd_nearest_refit.h"]
NEAREST_REBUILD_HEADERS = [NEAREST_CSRC / "rls_nearest_refit.hpp", NEAREST_CSRC / "rls_nearest_update.hpp", NEAREST_CSRC / "rls_nearest_rebuild.hpp",
                           INCLUDE / "rlshaders_amd_nearest_rebuild.h"]
NEAREST_GROUP_HEADERS = [NEAREST_CSRC / "rls_nearest_refit.hpp", NEAREST_CSRC / "rls_nearest_group.hpp", INCLUDE / "rlshaders_amd_nearest_group.h"]
NEAREST_ANY_HEADERS = [NEAREST_CSRC / "rls_nearest_any.hpp", INCLUDE / "rlshaders_amd_nearest_any.h"]

COMPANIONS = {c.name: c for c in (
    # BASELINE config 2's kernel with one uniform-slope pass per workgroup, handed the streamed EXACT reflect+refract launches
    # by the product (csrc/ggx.hip, rr_wg_launcher); the kernel has no FAST flavour
    Companion("ggx_rr", "rr", RR_CSRC, ["ggx_rr.hip"], RR_HEADERS, after_product=False),
    # the caller-traced integrators (include/rlshaders_amd_trace.h): the two flavours of the product's closure units
    Companion("trace", "trace", TRACE_CSRC, ["trace.hip"], TRACE_HEADERS, flavours=(EXACT, FAST)),
    # rlSss's probe walk (include/rlshaders_amd_walk.h); it includes the trace library's scan kernels from csrc_trace/
    Companion("walk", "walk", WALK_CSRC, ["walk.hip"], TRACE_HEADERS + WALK_HEADERS),
    # the shadow rays' walk (include/rlshaders_amd_shadow_walk.h): the scan from csrc_trace/, the list machinery it shares
    # with the probe walk from csrc_walk/
    Companion("shadow_walk", "shadow_walk", SHADOW_WALK_CSRC, ["shadow_walk.hip"],
              TRACE_HEADERS + SHADOW_WALK_HEADERS + [WALK_CSRC / "rls_walk_list.hpp"]),
    # nearest-hit queries over a triangle mesh (include/rlshaders_amd_nearest.h): nothing of the other companions' sources; its
    # header includes the probe walk's for the type of the walks' lists
    Companion("nearest", "nearest", NEAREST_CSRC, ["nearest.hip"], NEAREST_HEADERS),
    # moving meshes (include/rlshaders_amd_nearest_refit.h): it reads a scene of librls_nearest.so through the private header
    # csrc_nearest/rls_nearest_scene.hpp and calls nothing of that library; its host layer is csrc_nearest/rls_nearest_update.hpp
    Companion("nearest_refit", "nearest_refit", NEAREST_CSRC, ["refit.hip"], NEAREST_HEADERS + NEAREST_REFIT_HEADERS),
    # rebuilding a scene's tree for a moved mesh (include/rlshaders_amd_nearest_rebuild.h): the scene through the same private
    # header, the records and boxes through the refit's kernel header, the same host layer; it calls nothing of either library
    Companion("nearest_rebuild", "nearest_rebuild", NEAREST_CSRC, ["rebuild.hip"], NEAREST_HEADERS + NEAREST_REBUILD_HEADERS),
    # instanced scenes (include/rlshaders_amd_nearest_group.h): many placed scenes under a top-level tree, both levels walked in
    # one launch; the scenes through the same private header, the query's functions from the nearest-hit library's kernel header
    # (without its kernel); it calls nothing of the other libraries
    Companion("nearest_group", "nearest_group", NEAREST_CSRC, ["group.hip"], NEAREST_HEADERS + NEAREST_GROUP_HEADERS),
    # any-hit shadow queries (include/rlshaders_amd_nearest_any.h): a one-mesh scene through the same private header, the slab and
    # triangle tests from the nearest-hit library's kernel header (without its kernel); it calls nothing of the other libraries
    Companion("nearest_any", "nearest_any", NEAREST_CSRC, ["any.hip"], NEAREST_HEADERS + NEAREST_ANY_HEADERS),
)}
RR_LIB, TRACE_LIB, WALK_LIB = COMPANIONS["ggx_rr"].lib, COMPANIONS["trace"].lib, COMPANIONS["walk"].lib
SHADOW_WALK_LIB, NEAREST_LIB, NEAREST_REFIT_LIB = COMPANIONS["shadow_walk"].lib, COMPANIONS["nearest"].lib, COMPANIONS["nearest_refit"].lib
NEAREST_REBUILD_LIB, NEAREST_GROUP_LIB = COMPANIONS["nearest_rebuild"].lib, COMPANIONS["nearest_group"].lib
NEAREST_ANY_LIB = COMPANIONS["nearest_any"].lib


def build_companion(name: str, force: bool = False, verbose: bool = False) -> Path:
    """Compile a companion's units for gfx950 and link librls_<name>.so against the product library.  Returns its path."""
    c = COMPANIONS[name]
    hipcc = _hipcc()
    main = build_library(verbose=verbose) if c.after_product else LIB
    objdir = OBJDIR / c.objdir
    objdir.mkdir(parents=True, exist_ok=True)
    jobs, objs = [], []
    for unit in c.units:
        src = c.csrc / unit
        for suffix, flag in c.flavours:
            obj = objdir / (src.stem + suffix + ".o")
            objs.append(obj)
            if force or _stale(obj, [src, *HEADERS, *c.headers, Path(__file__)]):
                jobs.append([hipcc, *HIPCC_FLAGS, f"-cuid=rls_{c.name}.{src.stem}{suffix}", f"-D{flag}", "-c", str(src), "-o", str(obj)])
    return _compile_and_link(jobs, c.lib, objs, [*objs, main], [f"-L{LIBDIR}", "-lrlshaders_amd", "-Wl,-rpath,$ORIGIN"], force, verbose)


def build_rr_library(force: bool = False, verbose: bool = False) -> Path:
    return build_companion("ggx_rr", force, verbose)


def build_trace_library(force: bool = False, verbose: bool = False) -> Path:
    return build_companion("trace", force, verbose)


def build_walk_library(force: bool = False, verbose: bool = False) -> Path:
    return build_companion("walk", force, verbose)


def build_shadow_walk_library(force: bool = False, verbose: bool = False) -> Path:
    return build_companion("shadow_walk", force, verbose)


def build_nearest_library(force: bool = False, verbose: bool = False) -> Path:
    return build_companion("nearest", force, verbose)


def build_nearest_refit_library(force: bool = False, verbose: bool = False) -> Path:
    return build_companion("nearest_refit", force, verbose)


def build_nearest_rebuild_library(force: bool = False, verbose: bool = False) -> Path:
    return build_companion("nearest_rebuild", force, verbose)


def build_nearest_group_library(force: bool = False, verbose: bool = False) -> Path:
    return build_companion("nearest_group", force, verbose)


def build_nearest_any_library(force: bool = False, verbose: bool = False) -> Path:
    return build_companion("nearest_any", force, verbose)


def _link_flags(libs) -> list:
    return [f"-L{LIBDIR}", *[f"-l{l}" for l in libs], "-lrlshaders_amd", f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]


def build_example(name: str, companions, verbose: bool = False) -> Path:
    """host/<name>.cpp against the product and the companions named, in link order (a library ahead of what it uses); each is
    built first, and the example is stale against them, their headers and their host mirrors host/rls_<companion>.hpp"""
    deps = [LIB, *HEADERS]
    for c in reversed(companions):
        deps += [build_companion(c, verbose=verbose), HOST / f"rls_{c}.hpp", *COMPANIONS[c].headers]
    src, out = HOST / f"{name}.cpp", OBJDIR / name
    if _stale(out, [src, *deps]):
        _run([*HOST_CXX, f"-I{INCLUDE}", f"-I{HOST}", str(src), "-o", str(out), *_link_flags(f"rls_{c}" for c in companions)], verbose,
             f"host example {name} failed to build")
    return out


def build_trace_example(verbose: bool = False, name: str = "example_trace") -> Path:
    """host/example_trace.cpp (or ``name``: example_trace_bounce, example_trace_skin_bounce, example_trace_shadow,
    example_trace_path): emit -> a host-side "tracer" -> resolve"""
    return build_example(name, ["trace"], verbose)


def build_walk_example(verbose: bool = False, name: str = "example_walk") -> Path:
    """probe emit -> walk over a host-side closest-hit function -> resolve"""
    return build_example(name, ["walk", "trace"], verbose)


def build_shadow_walk_example(verbose: bool = False, name: str = "example_shadow_walk") -> Path:
    """light-loop emit -> walk over a host-side closest-hit function -> resolve"""
    return build_example(name, ["shadow_walk", "trace"], verbose)


def build_nearest_example(verbose: bool = False, name: str = "example_nearest") -> Path:
    """emit -> walk over device nearest hits -> resolve: no host tracer"""
    return build_example(name, ["nearest", "shadow_walk", "walk", "trace"], verbose)


def build_nearest_refit_example(verbose: bool = False, name: str = "example_nearest_refit") -> Path:
    """a sphere squashed and moved over three frames, walked on the refit scene and on a fresh one"""
    return build_example(name, ["nearest_refit", "nearest", "shadow_walk", "walk", "trace"], verbose)


def build_nearest_rebuild_example(verbose: bool = False, name: str = "example_nearest_rebuild") -> Path:
    """a sphere twisted, its tree rebuilt on the device, walked on the rebuilt scene and on a fresh one"""
    return build_example(name, ["nearest_rebuild", "nearest", "shadow_walk", "walk", "trace"], verbose)


def build_nearest_group_example(verbose: bool = False, name: str = "example_nearest_group") -> Path:
    """three instances of one mesh under a group: a shadow walk and a routed glossy queue through them, one instance moved"""
    return build_example(name, ["nearest_group", "nearest", "shadow_walk", "walk", "trace"], verbose)


def build_nearest_any_example(verbose: bool = False, name: str = "example_nearest_any") -> Path:
    """a light loop's shadow queue under an opaque occluder in one launch, and under a mixed table through the two-phase route"""
    return build_example(name, ["nearest_any", "nearest", "shadow_walk", "walk", "trace"], verbose)


def build_nearest_stats(verbose: bool = False) -> Path:
    """csrc_nearest/nearest_stats.cpp: the traversal source compiled for the host (g++, -ffp-contract=off, no HIP), counting the
    nodes and triangles a ray visits (rlshaders_amd.nearest.host_stats)."""
    OBJDIR.mkdir(exist_ok=True)
    src, out = NEAREST_CSRC / "nearest_stats.cpp", OBJDIR / "nearest_stats"
    if _stale(out, [src, NEAREST_CSRC / "rls_nearest_device.hpp", NEAREST_CSRC / "rls_nearest_bvh.hpp"]):
        _run([*HOST_CXX, "-ffp-contract=off", str(src), "-o", str(out)], verbose, "nearest_stats failed to build")
    return out


# ---- the test-only device probe of rls_libm.hpp's primitives (tests/native/libm_device_probe.hip): the product's own flags
# and headers, one unit, a fixed -cuid, linked on its own (it calls nothing of the product) -- under tests/, so that no product
# library gains an entry point.
PROBE_SRC = PKG.parent / "tests" / "native" / "libm_device_probe.hip"
PROBE_LIB = PKG.parent / "tests" / "native" / "build" / "librls_libm_probe.so"


def build_libm_probe(force: bool = False, verbose: bool = False, include: Path = CSRC, out: Path = PROBE_LIB) -> Path:
    """Compile tests/native/libm_device_probe.hip for gfx950 into tests/native/build/librls_libm_probe.so; rebuilt only when
    the probe or a header is newer.  ``include`` / ``out`` build it against another copy of the headers (a mutated
    rls_libm.hpp, to see the tests fail) next to the real one."""
    hipcc = _hipcc()
    out.parent.mkdir(parents=True, exist_ok=True)
    headers = HEADERS if include == CSRC else sorted(Path(include).glob("*"))
    if force or _stale(out, [PROBE_SRC, *headers, Path(__file__)]):
        _run([hipcc, *HIPCC_FLAGS, "-cuid=rls_libm_probe.libm_device_probe", "-DRLS_FAST=0", f"-I{include}", "-shared",
              str(PROBE_SRC), "-o", str(out)], verbose)
    return out


def build_host_examples(verbose: bool = False) -> Path:
    """Compile-check the C++ host mirror (header-only) and its example against the C ABI."""
    OBJDIR.mkdir(exist_ok=True)
    first = OBJDIR / "example_arnold_stub"
    for name in ("example_arnold_stub", "example_multi_gpu", "example_host_pipeline", "test_arnold_stub"):
        src, out = HOST / f"{name}.cpp", OBJDIR / name
        if src.exists() and _stale(out, [src, HOST / "rls_batch.hpp", HOST / "rl_arnold_stub.hpp", LIB, *HEADERS]):
            _run([*HOST_CXX, "-pthread", f"-I{INCLUDE}", f"-I{HOST}", str(src), "-o", str(out), *_link_flags([])], verbose,
                 f"host example {name} failed to build")
    return first


if __name__ == "__main__":
    # python -m rlshaders_amd.build [--force] [--variant NAME -DFOO=1 -fsome-flag -mllvm -some-option ...]
    args = sys.argv[1:]
    variant = args[args.index("--variant") + 1] if "--variant" in args else ""
    defines = [a[2:] for a in args if a.startswith("-D")]
    extra = []
    for i, a in enumerate(args):
        if a.startswith(("-f", "-m", "-O")):
            extra.append(a)
            if a == "-mllvm":
                extra.append(args[i + 1])
    print(build_library(force="--force" in args, verbose=True, variant=variant, defines=defines, extra=extra))
