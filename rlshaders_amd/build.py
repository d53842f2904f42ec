"""Build driver: compiles the HIP translation units under ``csrc/`` for gfx950 and links them
into ``rlshaders_amd/lib/librlshaders_amd.so`` (in-tree, so the library travels with the repo
snapshot to the GPU box).  hipcc cross-compiles without a GPU present.

Parity build flags: ``-ffp-contract=off`` and no fast-math (FMA contraction alone moves ~5 % of
chained GGX values past 1e-5 relative).  fp32 divide / sqrt stay correctly
rounded (hipcc default ``-fhip-fp32-correctly-rounded-divide-sqrt``).
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG = Path(__file__).resolve().parent
CSRC = PKG / "csrc"
LIBDIR = PKG / "lib"
OBJDIR = PKG / "build"
LIB = LIBDIR / "librlshaders_amd.so"
ARCH = "gfx950"

# the largest units first (the thread pool starts them first); integrate / lights / scatter / shade share csrc/rls_loops.hpp
SOURCES = ["shade.hip", "integrate.hip", "lights.hip", "scatter.hip", "skin.hip", "ggx.hip", "disney.hip", "sss.hip", "alternates.hip", "context.hip", "pipeline.hip",
           "libm_check.hip"]
FAST_UNITS = {"ggx.hip", "disney.hip", "sss.hip", "skin.hip", "integrate.hip", "lights.hip", "scatter.hip", "shade.hip", "alternates.hip"}
HEADERS = [CSRC / "rls_device.hpp", CSRC / "rls_libm.hpp", CSRC / "rls_libm_tables.inc", CSRC / "rls_libm_flavour_args.inc", CSRC / "rls_internal.hpp", CSRC / "rls_loops.hpp",
           PKG.parent / "include" / "rlshaders_amd.h", PKG.parent / "include" / "rlshaders_amd_diag.h"]

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
    srcs = sources()
    jobs = []
    objs = []
    for src in srcs:
        # every closure unit twice: EXACT (carries the C ABI) and FAST (kernels behind a hidden symbol)
        flavours = [("", "RLS_FAST=0")] + ([("_fast", "RLS_FAST=1")] if src.name in FAST_UNITS else [])
        for suffix, flag in flavours:
            obj = objdir / (src.stem + suffix + ".o")
            objs.append(obj)
            if force or _stale(obj, [src, *HEADERS, Path(__file__)]):
                # -cuid: clang names one symbol per unit `__hip_cuid_<hash>` and by default hashes the PATHS on its command line
                # into it -- the same sources in another checkout or object directory then differ in that symbol's length now
                # and again, which can move a code object's layout by a cache line (rlshaders_amd/codeid.py).  A fixed id per
                # unit makes the device code a function of sources and flags alone.
                jobs.append([hipcc, *HIPCC_FLAGS, *extra, f"-cuid=rlshaders_amd.{src.stem}{suffix}", f"-D{flag}",
                             *[f"-D{d}" for d in defines], "-c", str(src), "-o", str(obj)])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{p.stdout}\n{p.stderr}")
        return p

    if jobs:
        with ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            list(ex.map(run, jobs))
    if force or jobs or _stale(lib, objs):
        run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(lib), *map(str, objs)])
    if not variant:
        build_rr_library(force=force, verbose=verbose)
    return lib


# BASELINE config 2's kernel with one uniform-slope pass per workgroup (csrc_rr/ggx_rr.hip): a second companion, for the same
# reason as the one below -- the product's device code stays the frozen one.  The product library looks for it next to itself
# and hands it the streamed EXACT reflect+refract launches (csrc/ggx.hip, rr_wg_launcher), so build_library() builds it
# right after the product and every caller of build_library() has it.  EXACT only (the kernel has no FAST flavour), the
# same flags, a fixed -cuid; linked against librlshaders_amd.so (contexts, errors) and found next to it ($ORIGIN).
RR_CSRC = PKG / "csrc_rr"
RR_SOURCES = ["ggx_rr.hip"]
RR_LIB = LIBDIR / "librls_ggx_rr.so"
RR_HEADERS = [RR_CSRC / "rls_rr_device.hpp"]


def build_rr_library(force: bool = False, verbose: bool = False) -> Path:
    """Compile csrc_rr/ for gfx950 and link librls_ggx_rr.so against the product library (which must exist).  Returns its path."""
    hipcc = _hipcc()
    objdir = OBJDIR / "rr"
    objdir.mkdir(parents=True, exist_ok=True)
    objs, built = [], False
    for name in RR_SOURCES:
        src = RR_CSRC / name
        obj = objdir / (src.stem + ".o")
        objs.append(obj)
        if force or _stale(obj, [src, *HEADERS, *RR_HEADERS, Path(__file__)]):
            cmd = [hipcc, *HIPCC_FLAGS, f"-cuid=rls_ggx_rr.{src.stem}", "-DRLS_FAST=0", "-c", str(src), "-o", str(obj)]
            if verbose:
                print(" ".join(cmd), flush=True)
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{p.stdout}\n{p.stderr}")
            built = True
    if force or built or _stale(RR_LIB, [*objs, LIB]):
        cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(RR_LIB), *map(str, objs),
               f"-L{LIBDIR}", "-lrlshaders_amd", "-Wl,-rpath,$ORIGIN"]
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{p.stdout}\n{p.stderr}")
    return RR_LIB


# The caller-traced integrators (include/rlshaders_amd_trace.h): a companion library beside the product, so that the product's
# device code -- frozen, tests/test_profile_binding.py -- stays what it is.  Same flags, the same two flavours per unit (EXACT
# with the C ABI, FAST behind hidden symbols), fixed -cuid per unit; linked against librlshaders_amd.so (context, errors) and
# found next to it ($ORIGIN).  A name no build_library(variant=...) output can take.
TRACE_CSRC = PKG / "csrc_trace"
TRACE_SOURCES = ["trace.hip"]
TRACE_LIB = LIBDIR / "librls_trace.so"
TRACE_HEADERS = [*sorted(TRACE_CSRC.glob("*.hpp")), PKG.parent / "include" / "rlshaders_amd_trace.h"]


def build_trace_library(force: bool = False, verbose: bool = False) -> Path:
    """Compile csrc_trace/ for gfx950 and link librls_trace.so against the product library.  Returns its path."""
    hipcc = _hipcc()
    main = build_library(verbose=verbose)
    objdir = OBJDIR / "trace"
    objdir.mkdir(parents=True, exist_ok=True)
    jobs, objs = [], []
    for name in TRACE_SOURCES:
        src = TRACE_CSRC / name
        for suffix, flag in (("", "RLS_FAST=0"), ("_fast", "RLS_FAST=1")):
            obj = objdir / (src.stem + suffix + ".o")
            objs.append(obj)
            if force or _stale(obj, [src, *HEADERS, *TRACE_HEADERS, Path(__file__)]):
                jobs.append([hipcc, *HIPCC_FLAGS, f"-cuid=rls_trace.{src.stem}{suffix}", f"-D{flag}", "-c", str(src),
                             "-o", str(obj)])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{p.stdout}\n{p.stderr}")

    if jobs:
        with ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            list(ex.map(run, jobs))
    if force or jobs or _stale(TRACE_LIB, [*objs, main]):
        run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(TRACE_LIB), *map(str, objs),
             f"-L{LIBDIR}", "-lrlshaders_amd", "-Wl,-rpath,$ORIGIN"])
    return TRACE_LIB


def build_trace_example(verbose: bool = False, name: str = "example_trace") -> Path:
    """host/example_trace.cpp (or ``name``: example_trace_bounce, example_trace_skin_bounce, example_trace_shadow, example_trace_path) against both libraries (emit -> a host-side \"tracer\" ->
    resolve)."""
    OBJDIR.mkdir(exist_ok=True)
    lib = build_trace_library(verbose=verbose)
    src, out = PKG / "host" / f"{name}.cpp", OBJDIR / name
    if _stale(out, [src, PKG / "host" / "rls_trace.hpp", lib, LIB, *HEADERS, *TRACE_HEADERS]):
        cmd = ["g++", "-std=c++14", "-O2", "-Wall", f"-I{PKG.parent / 'include'}", f"-I{PKG / 'host'}", str(src), "-o", str(out),
               f"-L{LIBDIR}", "-lrls_trace", "-lrlshaders_amd", f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"host example {name} failed to build:\n{p.stdout}\n{p.stderr}")
    return out


# rlSss's probe walk (include/rlshaders_amd_walk.h): a third companion, so that the trace library's surface -- pinned entry point
# by entry point, tests/test_trace_abi.py -- and the product stay what they are.  The walk is mode-free: ONE unit, compiled with
# RLS_FAST=0 (IEEE arithmetic), the same flags, a fixed -cuid.  It includes the trace library's scan kernels from csrc_trace/, so
# those headers are its dependencies too; linked against librlshaders_amd.so (contexts, errors, graphs), found by $ORIGIN.
WALK_CSRC = PKG / "csrc_walk"
WALK_SOURCES = ["walk.hip"]
WALK_LIB = LIBDIR / "librls_walk.so"
WALK_HEADERS = [*sorted(WALK_CSRC.glob("*.hpp")), PKG.parent / "include" / "rlshaders_amd_walk.h"]


def build_walk_library(force: bool = False, verbose: bool = False) -> Path:
    """Compile csrc_walk/ for gfx950 and link librls_walk.so against the product library.  Returns its path."""
    hipcc = _hipcc()
    main = build_library(verbose=verbose)
    objdir = OBJDIR / "walk"
    objdir.mkdir(parents=True, exist_ok=True)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{p.stdout}\n{p.stderr}")

    objs, built = [], False
    for name in WALK_SOURCES:
        src = WALK_CSRC / name
        obj = objdir / (src.stem + ".o")
        objs.append(obj)
        if force or _stale(obj, [src, *HEADERS, *TRACE_HEADERS, *WALK_HEADERS, Path(__file__)]):
            run([hipcc, *HIPCC_FLAGS, f"-cuid=rls_walk.{src.stem}", "-DRLS_FAST=0", "-c", str(src), "-o", str(obj)])
            built = True
    if force or built or _stale(WALK_LIB, [*objs, main]):
        run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(WALK_LIB), *map(str, objs),
             f"-L{LIBDIR}", "-lrlshaders_amd", "-Wl,-rpath,$ORIGIN"])
    return WALK_LIB


def build_walk_example(verbose: bool = False, name: str = "example_walk") -> Path:
    """host/example_walk.cpp against the three libraries (probe emit -> walk over a host-side closest-hit function -> resolve)."""
    OBJDIR.mkdir(exist_ok=True)
    trace, lib = build_trace_library(verbose=verbose), build_walk_library(verbose=verbose)
    src, out = PKG / "host" / f"{name}.cpp", OBJDIR / name
    if _stale(out, [src, PKG / "host" / "rls_walk.hpp", PKG / "host" / "rls_trace.hpp", lib, trace, LIB, *HEADERS, *TRACE_HEADERS,
                    *WALK_HEADERS]):
        cmd = ["g++", "-std=c++14", "-O2", "-Wall", f"-I{PKG.parent / 'include'}", f"-I{PKG / 'host'}", str(src), "-o", str(out),
               f"-L{LIBDIR}", "-lrls_walk", "-lrls_trace", "-lrlshaders_amd", f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib",
               "-Wl,-rpath,/opt/rocm/lib"]
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"host example {name} failed to build:\n{p.stdout}\n{p.stderr}")
    return out


# ---- the shadow rays' walk (include/rlshaders_amd_shadow_walk.h): a fourth companion, built like the probe walk's -- one
# mode-free unit with RLS_FAST=0, the same flags, a fixed -cuid, the trace library's scan kernels included from csrc_trace/ --
# and linked against librlshaders_amd.so alone, found by $ORIGIN.
SHADOW_WALK_CSRC = PKG / "csrc_shadow_walk"
SHADOW_WALK_SOURCES = ["shadow_walk.hip"]
SHADOW_WALK_LIB = LIBDIR / "librls_shadow_walk.so"
SHADOW_WALK_HEADERS = [*sorted(SHADOW_WALK_CSRC.glob("*.hpp")), PKG.parent / "include" / "rlshaders_amd_shadow_walk.h",
                       PKG.parent / "include" / "rlshaders_amd_walk.h"]


def build_shadow_walk_library(force: bool = False, verbose: bool = False) -> Path:
    """Compile csrc_shadow_walk/ for gfx950 and link librls_shadow_walk.so against the product library.  Returns its path."""
    hipcc = _hipcc()
    main = build_library(verbose=verbose)
    objdir = OBJDIR / "shadow_walk"
    objdir.mkdir(parents=True, exist_ok=True)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{p.stdout}\n{p.stderr}")

    objs, built = [], False
    for name in SHADOW_WALK_SOURCES:
        src = SHADOW_WALK_CSRC / name
        obj = objdir / (src.stem + ".o")
        objs.append(obj)
        if force or _stale(obj, [src, *HEADERS, *TRACE_HEADERS, *SHADOW_WALK_HEADERS, Path(__file__)]):
            run([hipcc, *HIPCC_FLAGS, f"-cuid=rls_shadow_walk.{src.stem}", "-DRLS_FAST=0", "-c", str(src), "-o", str(obj)])
            built = True
    if force or built or _stale(SHADOW_WALK_LIB, [*objs, main]):
        run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(SHADOW_WALK_LIB), *map(str, objs),
             f"-L{LIBDIR}", "-lrlshaders_amd", "-Wl,-rpath,$ORIGIN"])
    return SHADOW_WALK_LIB


def build_shadow_walk_example(verbose: bool = False, name: str = "example_shadow_walk") -> Path:
    """host/example_shadow_walk.cpp against the product, the trace library and the shadow walk (light-loop emit -> walk over a
    host-side closest-hit function -> resolve)."""
    OBJDIR.mkdir(exist_ok=True)
    trace, lib = build_trace_library(verbose=verbose), build_shadow_walk_library(verbose=verbose)
    src, out = PKG / "host" / f"{name}.cpp", OBJDIR / name
    if _stale(out, [src, PKG / "host" / "rls_shadow_walk.hpp", PKG / "host" / "rls_trace.hpp", lib, trace, LIB, *HEADERS,
                    *TRACE_HEADERS, *SHADOW_WALK_HEADERS]):
        cmd = ["g++", "-std=c++14", "-O2", "-Wall", f"-I{PKG.parent / 'include'}", f"-I{PKG / 'host'}", str(src), "-o", str(out),
               f"-L{LIBDIR}", "-lrls_shadow_walk", "-lrls_trace", "-lrlshaders_amd", f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib",
               "-Wl,-rpath,/opt/rocm/lib"]
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"host example {name} failed to build:\n{p.stdout}\n{p.stderr}")
    return out


# ---- nearest-hit queries over a triangle mesh (include/rlshaders_amd_nearest.h): a fifth companion -- one mode-free unit with
# RLS_FAST=0, the same flags, a fixed -cuid -- linked against librlshaders_amd.so alone, found by $ORIGIN.  It includes nothing
# of the other companions' sources; its header includes the probe walk's for the type of the walks' lists.
NEAREST_CSRC = PKG / "csrc_nearest"
NEAREST_SOURCES = ["nearest.hip"]
NEAREST_LIB = LIBDIR / "librls_nearest.so"
NEAREST_HEADERS = [NEAREST_CSRC / "rls_nearest_device.hpp", NEAREST_CSRC / "rls_nearest_bvh.hpp", NEAREST_CSRC / "rls_nearest_scene.hpp",
                   PKG.parent / "include" / "rlshaders_amd_nearest.h", PKG.parent / "include" / "rlshaders_amd_walk.h",
                   PKG.parent / "include" / "rlshaders_amd_trace.h"]


def build_nearest_library(force: bool = False, verbose: bool = False) -> Path:
    """Compile csrc_nearest/ for gfx950 and link librls_nearest.so against the product library.  Returns its path."""
    hipcc = _hipcc()
    main = build_library(verbose=verbose)
    objdir = OBJDIR / "nearest"
    objdir.mkdir(parents=True, exist_ok=True)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{p.stdout}\n{p.stderr}")

    objs, built = [], False
    for name in NEAREST_SOURCES:
        src = NEAREST_CSRC / name
        obj = objdir / (src.stem + ".o")
        objs.append(obj)
        if force or _stale(obj, [src, *HEADERS, *NEAREST_HEADERS, Path(__file__)]):
            run([hipcc, *HIPCC_FLAGS, f"-cuid=rls_nearest.{src.stem}", "-DRLS_FAST=0", "-c", str(src), "-o", str(obj)])
            built = True
    if force or built or _stale(NEAREST_LIB, [*objs, main]):
        run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(NEAREST_LIB), *map(str, objs),
             f"-L{LIBDIR}", "-lrlshaders_amd", "-Wl,-rpath,$ORIGIN"])
    return NEAREST_LIB


def build_nearest_example(verbose: bool = False, name: str = "example_nearest") -> Path:
    """host/example_nearest.cpp against the product, the trace library, both walks and the nearest-hit library (emit -> walk over
    device nearest hits -> resolve: no host tracer)."""
    OBJDIR.mkdir(exist_ok=True)
    trace, walk, shadow = build_trace_library(verbose=verbose), build_walk_library(verbose=verbose), build_shadow_walk_library(verbose=verbose)
    lib = build_nearest_library(verbose=verbose)
    host = PKG / "host"
    src, out = host / f"{name}.cpp", OBJDIR / name
    if _stale(out, [src, host / "rls_nearest.hpp", host / "rls_shadow_walk.hpp", host / "rls_walk.hpp", host / "rls_trace.hpp", lib, trace,
                    walk, shadow, LIB, *HEADERS, *TRACE_HEADERS, *WALK_HEADERS, *SHADOW_WALK_HEADERS, *NEAREST_HEADERS]):
        cmd = ["g++", "-std=c++14", "-O2", "-Wall", f"-I{PKG.parent / 'include'}", f"-I{host}", str(src), "-o", str(out),
               f"-L{LIBDIR}", "-lrls_nearest", "-lrls_shadow_walk", "-lrls_walk", "-lrls_trace", "-lrlshaders_amd",
               f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"host example {name} failed to build:\n{p.stdout}\n{p.stderr}")
    return out


def build_nearest_stats(verbose: bool = False) -> Path:
    """csrc_nearest/nearest_stats.cpp: the traversal source compiled for the host (g++, -ffp-contract=off, no HIP), counting the
    nodes and triangles a ray visits (rlshaders_amd.nearest.host_stats)."""
    OBJDIR.mkdir(exist_ok=True)
    src, out = NEAREST_CSRC / "nearest_stats.cpp", OBJDIR / "nearest_stats"
    if _stale(out, [src, NEAREST_CSRC / "rls_nearest_device.hpp", NEAREST_CSRC / "rls_nearest_bvh.hpp"]):
        cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", str(src), "-o", str(out)]
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"nearest_stats failed to build:\n{p.stdout}\n{p.stderr}")
    return out


# ---- moving meshes (include/rlshaders_amd_nearest_refit.h): a sixth companion, librls_nearest_refit.so -- csrc_nearest/refit.hip,
# one mode-free unit with RLS_FAST=0, the same flags, a fixed -cuid -- linked against librlshaders_amd.so alone, found by
# $ORIGIN.  It reads a scene of librls_nearest.so through the private header csrc_nearest/rls_nearest_scene.hpp and calls
# nothing of that library.
NEAREST_REFIT_SOURCES = ["refit.hip"]
NEAREST_REFIT_LIB = LIBDIR / "librls_nearest_refit.so"
NEAREST_REFIT_HEADERS = [NEAREST_CSRC / "rls_nearest_refit.hpp", PKG.parent / "include" / "rlshaders_amd_nearest_refit.h"]


def build_nearest_refit_library(force: bool = False, verbose: bool = False) -> Path:
    """Compile csrc_nearest/refit.hip for gfx950 and link librls_nearest_refit.so against the product library.  Returns its path."""
    hipcc = _hipcc()
    main = build_library(verbose=verbose)
    objdir = OBJDIR / "nearest_refit"
    objdir.mkdir(parents=True, exist_ok=True)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{p.stdout}\n{p.stderr}")

    objs, built = [], False
    for name in NEAREST_REFIT_SOURCES:
        src = NEAREST_CSRC / name
        obj = objdir / (src.stem + ".o")
        objs.append(obj)
        if force or _stale(obj, [src, *HEADERS, *NEAREST_HEADERS, *NEAREST_REFIT_HEADERS, Path(__file__)]):
            run([hipcc, *HIPCC_FLAGS, f"-cuid=rls_nearest_refit.{src.stem}", "-DRLS_FAST=0", "-c", str(src), "-o", str(obj)])
            built = True
    if force or built or _stale(NEAREST_REFIT_LIB, [*objs, main]):
        run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(NEAREST_REFIT_LIB), *map(str, objs),
             f"-L{LIBDIR}", "-lrlshaders_amd", "-Wl,-rpath,$ORIGIN"])
    return NEAREST_REFIT_LIB


def build_nearest_refit_example(verbose: bool = False, name: str = "example_nearest_refit") -> Path:
    """host/example_nearest_refit.cpp against the product, the trace library, both walks, the nearest-hit library and its
    refit (a sphere squashed and moved over three frames, walked on the refit scene and on a fresh one)."""
    OBJDIR.mkdir(exist_ok=True)
    trace, walk, shadow = build_trace_library(verbose=verbose), build_walk_library(verbose=verbose), build_shadow_walk_library(verbose=verbose)
    near, lib = build_nearest_library(verbose=verbose), build_nearest_refit_library(verbose=verbose)
    host = PKG / "host"
    src, out = host / f"{name}.cpp", OBJDIR / name
    if _stale(out, [src, host / "rls_nearest_refit.hpp", host / "rls_nearest.hpp", host / "rls_shadow_walk.hpp", host / "rls_walk.hpp",
                    host / "rls_trace.hpp", lib, near, trace, walk, shadow, LIB, *HEADERS, *TRACE_HEADERS, *WALK_HEADERS,
                    *SHADOW_WALK_HEADERS, *NEAREST_HEADERS, *NEAREST_REFIT_HEADERS]):
        cmd = ["g++", "-std=c++14", "-O2", "-Wall", f"-I{PKG.parent / 'include'}", f"-I{host}", str(src), "-o", str(out),
               f"-L{LIBDIR}", "-lrls_nearest_refit", "-lrls_nearest", "-lrls_shadow_walk", "-lrls_walk", "-lrls_trace", "-lrlshaders_amd",
               f"-Wl,-rpath,{LIBDIR}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"host example {name} failed to build:\n{p.stdout}\n{p.stderr}")
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
        cmd = [hipcc, *HIPCC_FLAGS, "-cuid=rls_libm_probe.libm_device_probe", "-DRLS_FAST=0", f"-I{include}", "-shared",
               str(PROBE_SRC), "-o", str(out)]
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{' '.join(cmd)}\n{p.stdout}\n{p.stderr}")
    return out


def build_host_examples(verbose: bool = False) -> Path:
    """Compile-check the C++ host mirror (header-only) and its example against the C ABI."""
    OBJDIR.mkdir(exist_ok=True)
    first = OBJDIR / "example_arnold_stub"
    for name in ("example_arnold_stub", "example_multi_gpu", "example_host_pipeline", "test_arnold_stub"):
        src = PKG / "host" / f"{name}.cpp"
        out = OBJDIR / name
        if not src.exists():
            continue
        if _stale(out, [src, PKG / "host" / "rls_batch.hpp", PKG / "host" / "rl_arnold_stub.hpp", LIB, *HEADERS]):
            cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-pthread", f"-I{PKG.parent / 'include'}", f"-I{PKG / 'host'}",
                   str(src), "-o", str(out), f"-L{LIBDIR}", "-lrlshaders_amd", f"-Wl,-rpath,{LIBDIR}",
                   "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
            if verbose:
                print(" ".join(cmd), flush=True)
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                raise RuntimeError(f"host example {name} failed to build:\n{p.stdout}\n{p.stderr}")
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
