"""CPU: the ABI of the companion library of the caller-traced integrators (include/rlshaders_amd_trace.h, librls_trace.so,
rlshaders_amd/trace.py): the whole surface, from the table tests/trace_abi_tables.py.

The header declares, the library exports and trace.PROTOTYPES binds the same entry points with the same arity; every
ctypes.Structure of trace.py mirrors one struct of the header in member order, array lengths, sizeof and every offsetof, and the
constants carry the header's values (both from one compiled probe); the header is C99 / C++14 clean in every use the families
document; the library holds exactly two gfx950 code objects, every per-mode kernel in the unit of its math mode and every
mode-free kernel in the EXACT unit alone; the product library -- frozen, tests/test_profile_binding.py -- is as recorded and
holds none of this.  The argument checks that need no device: of the node, bounce and opacity calls in
tests/test_trace_{shade,bounce,skin,opacity}_abi.py, of the routes in tests/test_trace_route_checks.py; here the scratch sizes,
and the standalone integrators' (rlSss probe / scatter, rlDisney emit) through tests/native/trace_sss_checks.cpp and
trace_disney_checks.cpp in both math modes, which like tests/test_argument_checks.py skip where torch sees a GPU."""
import ctypes as C
import inspect
import json
import re
import subprocess

import pytest

from trace_abi_tables import FAMILIES, every
from trace_abi_util import (HEADER, INVALID, ROOT, check_absent_from_product, check_bound, check_callables, check_members,
                            check_placement, code_text, declarations, declared_symbols, declared_trace_symbols, dynamic_symbols,
                            exported_trace_symbols, header_structs, mirrors, run_probe, struct_body, struct_members,
                            syntax_check, trace_lib)  # noqa: F401

# (entry point, parameter) -> the struct it points to, or takes by value
POINTERS = {("rls_trace_disney_emit", 2): "capi.DisneyClosure",
            ("rls_trace_sss_probe_emit", 2): "capi.SssClosure", ("rls_trace_sss_probe_emit", 7): "trace.ProbeQueue_",
            ("rls_trace_sss_scatter_resolve", 5): "trace.ProbeQueue_", ("rls_trace_sss_scatter_resolve", 6): "trace.ProbeHits_",
            ("rls_trace_sss_hits_emit", 2): "capi.SssClosure", ("rls_trace_sss_hits_emit", 5): "trace.ProbeQueue_",
            ("rls_trace_sss_hits_emit", 6): "trace.ProbeHits_", ("rls_trace_sss_hits_emit", 15): "trace.HitQueues_",
            ("rls_trace_sss_hits_resolve", 1): "trace.ProbeHits_", ("rls_trace_sss_hits_resolve", 6): "trace.HitQueues_",
            ("rls_trace_ggx_direct_emit", 3): "capi.GgxShader", ("rls_trace_ggx_direct_emit", 10): "trace.ShadowQueue_",
            ("rls_trace_disney_direct_emit", 9): "trace.ShadowQueue_", ("rls_trace_ggx_direct_resolve", 7): "trace.ShadowQueue_",
            ("rls_trace_disney_direct_resolve", 5): "trace.ShadowQueue_"}
BY_VALUE = {("rls_trace_sss_hits_emit", 7): "capi.CVec3"}
METHODS = dict(HitQueues=("resolve",), HitRoutes=("sizes", "index", "gather", "scatter", "fill_misses", "gather_state"))

# the constants trace.py restates, and the values the header's users pin as literals
CONSTANTS = ("RLS_RAY_TRANSMITTED", "RLS_RAY_TIR_MIRROR", "RLS_MAX_PROBE_HITS", "RLS_SHADOW_LIGHT_MASK", "RLS_SHADOW_BSDF",
             "RLS_SHADOW_SPECULAR", "RLS_SHADOW_DIFFUSE", "RLS_RT_CAMERA", "RLS_RT_SHADOW", "RLS_RT_REFLECTED", "RLS_RT_REFRACTED",
             "RLS_RT_DIFFUSE", "RLS_RT_GLOSSY", "RLS_SKIN_DIFFUSE_SEED", "RLS_ROUTE_MAX_BINS", "RLS_ROUTE_MAX_W32", "RLS_ROUTE_MAX_U8")
LITERALS = dict(RLS_RAY_TIR_MIRROR=1, RLS_ROUTE_MAX_BINS=16, RLS_ROUTE_MAX_W32=24, RLS_ROUTE_MAX_U8=8)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """what the C compiler says: sizeof of every struct of the header, offsetof of every member, the value of every constant"""
    lines = [f'  printf("{name} %lld\\n", (long long)({name}));' for name in CONSTANTS + ("RLS_MAX_LIGHTS",)]
    for c_name in header_structs():
        lines.append(f'  printf("sizeof {c_name} %zu\\n", sizeof({c_name}));')
        lines += [f'  printf("{c_name}.{m} %zu\\n", offsetof({c_name}, {m}));' for m, _ in struct_members(c_name)]
    out = run_probe(tmp_path_factory.mktemp("probe"), lines)
    assert len(out) == len(lines)
    return {k: int(v) for k, v in (l.rsplit(" ", 1) for l in out)}


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_exports_exactly_the_header_and_the_bindings(trace_lib):
    from rlshaders_amd import trace
    declared, arity = declared_trace_symbols(), every("arity")
    assert declared and all(s.startswith("rls_trace_") for s in declared), declared
    assert exported_trace_symbols(trace_lib) == declared
    assert sorted(trace.PROTOTYPES) == declared and sorted(declarations()) == declared and sorted(arity) == declared
    assert sum(len(f["arity"]) for f in FAMILIES.values()) == len(arity)        # no entry point in two families
    check_bound(trace_lib, arity)          # binds every prototype (no device needed)


def test_the_python_surface():
    from rlshaders_amd import _capi as capi, trace
    modules = dict(capi=capi, trace=trace)
    resolve = lambda spec: getattr(modules[spec.split(".")[0]], spec.split(".")[1])
    for (name, at), spec in POINTERS.items():
        assert trace.PROTOTYPES[name][1][at] == C.POINTER(resolve(spec)), (name, at)
    for (name, at), spec in BY_VALUE.items():
        assert trace.PROTOTYPES[name][1][at] is resolve(spec), (name, at)
    check_callables(every("callables"))
    for cls, methods in METHODS.items():
        assert all(callable(getattr(getattr(trace, cls), m)) for m in methods), cls
    assert issubclass(trace.SkinNodeQueues, trace._NodeQueues) and issubclass(trace.SkinBounceQueues, trace.SkinNodeQueues)
    # ggx_shader carries KtColor and Kt, and its first callers are unchanged
    sig = inspect.signature(trace.ggx_shader)
    assert list(sig.parameters)[:5] == ["sampler", "KdColor", "Kd", "diffuseRoughness", "Ks"]
    assert sig.parameters["KtColor"].default == (1.0, 1.0, 1.0) and sig.parameters["Kt"].default == 0.0


def test_not_in_the_drop_in_surface():
    """the 82-entry drop-in header and its ctypes prototypes are left alone"""
    from rlshaders_amd import _capi
    drop_in = declared_symbols(ROOT / "include" / "rlshaders_amd.h", ROOT / "include" / "rlshaders_amd_diag.h")
    assert drop_in and not [s for s in drop_in if s.startswith("rls_trace_")]
    assert not [s for s in _capi.PROTOTYPES if s.startswith("rls_trace_")]
    assert "rlshaders_amd_trace.h" not in (ROOT / "include" / "rlshaders_amd.h").read_text()


# ---- structs and constants: trace.py against the compiler ----------------------------------------------------------------------
def test_every_struct_mirror_has_the_headers_layout(probe):
    from rlshaders_amd import trace
    assert sorted(mirrors()) == sorted(header_structs()) == sorted(every("structs")) and len(mirrors()) == 21
    check_members(header_structs())
    for c_name, cls in mirrors().items():
        assert C.sizeof(cls) == probe[f"sizeof {c_name}"], c_name
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == probe[f"{c_name}.{f}"], (c_name, f)
    assert [m for m, _ in struct_members("rls_hit_queues")] == ["hit_capacity", "hit_count", "hit_element", "shadow", "diffuse",
                                                                "scratch", "scratch_bytes"]
    body = struct_body("rls_hit_queues")                         # the two queues by value
    assert "rls_shadow_queue shadow" in body and "rls_ray_queue diffuse" in body
    assert dict(trace.HitQueues_._fields_)["shadow"] is trace.ShadowQueue_ and dict(trace.HitQueues_._fields_)["diffuse"] is trace.RayQueue_
    # the rlSkin node's structs are embedded whole, first: a bounce struct's address is its node struct's
    assert probe["rls_skin_bounce_queues.node"] == 0 and probe["rls_skin_bounce_traced.node"] == 0
    assert trace.SkinBounceQueues_.node.offset == 0 and trace.SkinBounceQueues_._fields_[0][1] is trace.SkinNodeQueues_
    assert trace.SkinBounceTraced_.node.offset == 0 and trace.SkinBounceTraced_._fields_[0][1] is trace.SkinNodeTraced_
    assert C.sizeof(trace.SkinBounceQueues_) == C.sizeof(trace.SkinNodeQueues_) + C.sizeof(C.c_void_p)
    assert C.sizeof(trace.SkinBounceTraced_) == C.sizeof(trace.SkinNodeTraced_) + 3 * C.sizeof(C.c_void_p)


def test_the_constants_are_the_headers(probe):
    from rlshaders_amd import trace
    for name in CONSTANTS:
        assert getattr(trace, name) == probe[name], name
    for name, value in LITERALS.items():
        assert probe[name] == value, name
    assert set(re.findall(r"\bRLS_RT_[A-Z]+\b", code_text())) == {"RLS_RT_CAMERA", "RLS_RT_SHADOW", "RLS_RT_REFLECTED", "RLS_RT_REFRACTED",
                                                                  "RLS_RT_DIFFUSE", "RLS_RT_GLOSSY"}
    assert set(re.findall(r"\bRLS_ROUTE_MAX_[A-Z0-9]+\b", code_text())) == {"RLS_ROUTE_MAX_BINS", "RLS_ROUTE_MAX_W32", "RLS_ROUTE_MAX_U8"}
    assert probe["RLS_SHADOW_LIGHT_MASK"] == probe["RLS_MAX_LIGHTS"] - 1
    assert probe["RLS_SHADOW_LIGHT_MASK"] | probe["RLS_SHADOW_BSDF"] | probe["RLS_SHADOW_SPECULAR"] | probe["RLS_SHADOW_DIFFUSE"] == 0x3F


# ---- the header ----------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_cxx(tmp_path):
    """one translation unit with every family's snippet, a function each"""
    snippets = [f["snippet"] for f in FAMILIES.values() if f["snippet"]]
    functions = [f"int family_{i}(void);\nint family_{i}(void){{ {body} }}\n" for i, body in enumerate(snippets)]
    syntax_check(tmp_path, "".join(functions) + "int main(void){ return " + " + ".join(f"family_{i}()" for i in range(len(snippets))) + "; }\n")
    # the header no longer lists rlSkin as not covered, and says what stays a per-call flag
    assert "Not covered: rlSkin" not in HEADER.read_text()
    assert "trace_diffuse" in HEADER.read_text().split("Not covered:")[1].split("*/")[0]


# ---- the device code -----------------------------------------------------------------------------------------------------------
def test_code_objects_are_gfx950(trace_lib):
    """two gfx950 code objects; every per-mode kernel in its mode's unit at every width; every mode-free kernel once, in the EXACT
    unit, the FAST image without a trace of it"""
    check_placement(trace_lib, every("width"), every("mode"), every("free"))


def test_links_the_product_library_by_origin(trace_lib):
    d = subprocess.run(["readelf", "-d", str(trace_lib)], capture_output=True, text=True, check=True).stdout
    assert "[librlshaders_amd.so]" in d and "$ORIGIN" in d


def test_product_library_is_unchanged(trace_lib):
    """building the companion leaves the product's device code as recorded, and none of its kernels or symbols is in there"""
    from rlshaders_amd import build
    from rlshaders_amd.codeid import DeviceCode, code_objects, fatbin
    main = build.build_library()
    recorded = json.loads((ROOT / "profiles" / "r06_library_id.json").read_text())
    assert DeviceCode(main).library_id == recorded["library_id"]
    assert len(code_objects(fatbin(build.LIB))) >= 12
    check_absent_from_product(every("width") + every("mode") + every("free"))
    assert "rls_trace_" not in dynamic_symbols(build.LIB)


# ---- the scratch sizes: no device needed ---------------------------------------------------------------------------------------
def test_scratch_sizes_and_their_argument_checks(trace_lib):
    from rlshaders_amd import _capi as capi, trace
    lib = trace.load()
    b = C.c_size_t()
    up = lambda x: (x + 255) // 256 * 256                        # every part is rounded up to 256 bytes
    tile = 2048
    # the light loops: 10 float planes and a 32-bit tag per slot, n_lights * 3 * spp_n^2 slots a point, plus the scan's tile sums
    for n, nl, spp_n in ((1, 1, 1), (1000, 2, 4), (5, 8, 16), (0, 3, 2)):
        assert lib.rls_trace_shadow_scratch_bytes(n, nl, spp_n, C.byref(b)) == 0
        slots = n * nl * 3 * spp_n * spp_n
        assert 11 * 4 * slots <= b.value <= 11 * 4 * slots + 12 * 256 + 8 * (n // tile + 1)
        assert trace.shadow_scratch_bytes(n, nl, spp_n) == b.value
    for args in ((-1, 1, 1), (1, 0, 1), (1, 9, 1), (1, 1, 0), (1, 1, 17)):
        assert lib.rls_trace_shadow_scratch_bytes(*args, C.byref(b)) == INVALID, args
    assert lib.rls_trace_shadow_scratch_bytes(1, 1, 1, None) == INVALID
    # (the light loops' entry points refuse a NULL context before anything else)
    q = trace.ShadowQueue_()
    assert lib.rls_trace_disney_direct_emit(None, 1, None, capi.CVec3(), None, 1, 1, 0, 0, C.byref(q)) == INVALID
    assert lib.rls_trace_ggx_direct_resolve(None, 1, None, None, None, 1, 1, C.byref(q), capi.CRgb(), capi.Rgb(), capi.Rgb()) == INVALID
    # the hits: the staging grows with hit_capacity x n_lights x 2 x hit_spp_n^2 slots of five float planes and a 32-bit tag
    sb = lib.rls_trace_sss_hits_scratch_bytes
    assert sb(67, 2, 3, 804, 2, 2, None) == INVALID
    for args in ((-1, 2, 3, 8, 2, 2), (67, 0, 3, 8, 2, 2), (67, 17, 3, 8, 2, 2), (67, 2, 0, 8, 2, 2), (67, 2, 13, 8, 2, 2),
                 (67, 2, 3, -1, 2, 2), (67, 2, 3, 8, -1, 2), (67, 2, 3, 8, 9, 2), (67, 2, 3, 8, 2, 0), (67, 2, 3, 8, 2, 17)):
        assert sb(*args, C.byref(b)) == INVALID, args
    size = trace.sss_hits_scratch_bytes
    for n, spp_n, cap, nl, hs in ((67, 2, 804, 2, 2), (0, 1, 0, 0, 1), (5000, 1, 100, 8, 4), (67, 2, 803, 0, 1)):
        rays, slots = n * spp_n * spp_n, cap * nl * 2 * hs * hs
        tiles = max((rays + tile - 1) // tile, (cap + tile - 1) // tile, 1)
        want = up(rays * 2) + up((rays + 1) * 8) + up(tiles * 8) + 6 * up(slots * 4) + 4 * up(cap * 4) + up(cap * 2)
        assert size(n, spp_n, 3, cap, nl, hs) == want, (n, spp_n, cap, nl, hs)
    assert size(67, 2, 3, 804, 2, 2) == size(67, 2, 12, 804, 2, 2)  # (the slots per ray do not enter: the mask is 16 bits)
    # the routes: (bins + 1) x tiles counts and the grand total, then the scan's tile sums
    for rays, bins in ((0, 1), (1, 1), (tile, 3), (tile + 1, 3), (1 << 24, 16), ((1 << 32) - 1, 16)):
        cells = (bins + 1) * ((rays + tile - 1) // tile)
        assert trace.route_scratch_bytes(rays, bins) == up(8 * (cells + 1)) + up(8 * max((cells + tile - 1) // tile, 1)), (rays, bins)


# ---- the native drivers: the standalone integrators' argument checks in both math modes ----------------------------------------
def _driver_rows(tmp_path_factory, name, columns):
    """build tests/native/<name>.cpp against both libraries, run it, and read its tab-separated rows"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the driver hands dummy planes to the entry points")
    from rlshaders_amd import build
    exe = tmp_path_factory.mktemp(name) / name
    cmd = [build._hipcc(), "-std=c++17", "-O1", "-x", "hip", "--offload-host-only", "-Wall", "-DRLS_FAST=0",
           str(ROOT / "tests" / "native" / f"{name}.cpp"), "-o", str(exe), f"-L{build.LIBDIR}", "-lrls_trace", "-lrlshaders_amd",
           f"-Wl,-rpath,{build.LIBDIR}"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    rows = []
    for line in p.stdout.splitlines():
        fields = line.split("\t")
        assert len(fields) == len(columns), line
        r = dict(zip(columns, fields))
        r.update(fast=int(r["fast"]), status=int(r["status"]), want=int(r["want"]))
        rows.append(r)
    return rows


def _driver_mismatches(cases, entry_of):
    wrong = []
    for c in cases:
        ok = c["status"] == c["want"]
        if ok and c["want"] == 1:                           # RLS_ERR_INVALID_ARGUMENT: "<name>: <text>"
            prefix, _, text = c["message"].partition(": ")
            ok = prefix == entry_of(c) and text == c["text"]
        elif ok and c["want"] == 3:                         # RLS_ERR_HIP: every check passed, the launch found no device
            ok = c["message"].startswith("HIP error ")
        if not ok:
            wrong.append(f'{c.get("verb", "")} {c["what"]} [fast={c["fast"]}]: status {c["status"]} "{c["message"]}", '
                         f'want {c["want"]} "{c["text"]}"')
    return wrong


@pytest.fixture(scope="module")
def sss_cases(tmp_path_factory, trace_lib):
    return _driver_rows(tmp_path_factory, "trace_sss_checks", ("verb", "what", "fast", "status", "want", "text", "message"))


@pytest.fixture(scope="module")
def disney_cases(tmp_path_factory, trace_lib):
    return _driver_rows(tmp_path_factory, "trace_disney_checks", ("what", "fast", "status", "want", "text", "message"))


def test_sss_argument_checks_in_both_modes(sss_cases):
    for fast in (0, 1):
        emits = {c["what"] for c in sss_cases if c["fast"] == fast and c["verb"] == "emit"}
        resolves = {c["what"] for c in sss_cases if c["fast"] == fast and c["verb"] == "resolve"}
        assert emits >= {"valid", "spp_n 0", "spp_n 17", "queue NULL", "queue.origin NULL", "queue.maxdist NULL",
                         "queue.capacity short", "closure NULL", "N NULL", "P NULL", "n == 0"}
        assert resolves >= {"valid", "spp_n 0", "spp_n 17", "max_hits 0", "max_hits 13", "hits NULL", "hits.stride short",
                            "hits.count NULL", "hits.irradiance NULL", "queue.capacity short", "result NULL", "n == 0"}
    wrong = _driver_mismatches(sss_cases, lambda c: "rls_trace_sss_probe_emit" if c["verb"] == "emit" else "rls_trace_sss_scatter_resolve")
    assert not wrong, "\n".join(wrong)


def test_disney_argument_checks_in_both_modes(disney_cases):
    for fast in (0, 1):
        mine = [c for c in disney_cases if c["fast"] == fast]
        assert len(mine) >= 30
        assert {c["what"] for c in mine} >= {"valid, diffuse", "valid, glossy", "lobe 0", "spp_n 0", "spp_n 17", "n < 0",
                                            "queue NULL", "queue.offsets NULL", "queue.dir NULL", "queue.weight.g NULL",
                                            "closure NULL", "wo NULL", "queue.capacity short", "queue.scratch NULL",
                                            "queue.scratch short", "n == 0"}
    wrong = _driver_mismatches(disney_cases, lambda c: "emit")
    assert not wrong, "\n".join(wrong)
