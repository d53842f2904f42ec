"""CPU: the routing calls of the companion library (rls_trace_route_scratch_bytes, rls_trace_route_hits, rls_trace_route_gather,
rls_trace_route_scatter, rls_trace_route_fill; include/rlshaders_amd_trace.h, librls_trace.so).

The five symbols are declared, exported and bound with matching arity; the two structs' members match the header in order, the
plane arrays in length; the header compiles as C99 and C++14; the library still holds two code objects, the five mode-free
kernels in the EXACT one alone and none in the product library, whose library_id is the recorded one; the scratch size is what
the header's layout gives."""
import ctypes as C
import json
import re
import subprocess

from test_trace_shade_abi import HEADER, ROOT, _declarations, trace_lib  # noqa: F401

ARITY = dict(rls_trace_route_scratch_bytes=3, rls_trace_route_hits=4, rls_trace_route_gather=4, rls_trace_route_scatter=4,
             rls_trace_route_fill=6)
KERNELS = ("route_count_kernel", "route_place_kernel", "route_gather_kernel", "route_scatter_kernel", "route_fill_kernel")
STRUCTS = (("HitRoutes_", "rls_hit_routes"), ("RoutePlanes_", "rls_route_planes"))
CAPS = dict(RLS_ROUTE_MAX_BINS=16, RLS_ROUTE_MAX_W32=24, RLS_ROUTE_MAX_U8=8)


def test_declared_exported_and_bound_with_matching_arity(trace_lib):
    from rlshaders_amd import trace
    decl = _declarations()
    out = subprocess.run(["nm", "-D", "--defined-only", str(trace_lib)], capture_output=True, text=True, check=True).stdout
    lib = trace.load()
    for name, arity in ARITY.items():
        assert name in decl, name
        assert len(decl[name].split(",")) == arity, (name, decl[name])
        assert f" T {name}\n" in out, name
        restype, argtypes = trace.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == arity, name
        assert getattr(lib, name).argtypes == argtypes
    assert all(callable(getattr(trace, f)) for f in ("route_hits", "HitRoutes", "route_gather", "route_scatter", "route_fill",
                                                     "route_scratch_bytes"))
    for method in ("sizes", "index", "gather", "scatter", "fill_misses", "gather_state"):
        assert callable(getattr(trace.HitRoutes, method)), method


def test_the_structs_have_the_headers_members():
    from rlshaders_amd import trace
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    caps = re.search(r"enum \{([^}]*RLS_ROUTE_MAX_BINS[^}]*)\}", text).group(1)
    assert {k.strip(): int(v) for k, v in (part.split("=") for part in caps.split(","))} == CAPS
    for name, value in CAPS.items():
        assert getattr(trace, name) == value
    for cls, c_name in STRUCTS:
        body = re.search(r"typedef struct %s\s*\{(.*?)\} %s;" % (c_name, c_name), text, flags=re.S).group(1)
        members = []                                             # (name, array length or None), a declarator at a time
        for d in body.split(";"):
            for part in d.split(",") if d.strip() else []:
                m = re.search(r"(\w+)\s*(?:\[(\w+)\])?\s*$", part.strip())
                members.append((m.group(1), CAPS[m.group(2)] if m.group(2) else None))
        fields = [(f[0], f[1]._length_ if issubclass(f[1], C.Array) else None) for f in getattr(trace, cls)._fields_]
        assert members == fields, (c_name, members, fields)


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_trace.h"\n'
                   'int main(void){ rls_hit_routes r = {2, 0, 0, 0, 0, 0}; rls_route_planes p = {0, 0, {0}, {0}, {0}, {0}};\n'
                   '  size_t b = 0; float v[3] = {0.0f, 0.0f, 0.0f}; float *d[3] = {0, 0, 0};\n'
                   '  return rls_trace_route_scratch_bytes(1, 2, &b) + rls_trace_route_hits(0, 0, 0, &r) +\n'
                   '         rls_trace_route_gather(0, 0, 0, &p) + rls_trace_route_scatter(0, 0, 0, &p) +\n'
                   '         rls_trace_route_fill(0, 0, 0, 3, d, v) + (RLS_ROUTE_MAX_BINS == 16 ? 0 : 1); }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{ROOT / 'include'}",
                            "-x", "c" if cc == "gcc" else "c++", str(src)], capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)


def test_still_two_code_objects_with_the_five_kernels_in_the_exact_one(trace_lib):
    from rlshaders_amd import build
    from rlshaders_amd.codeid import DeviceCode, code_objects, fatbin
    objs = code_objects(fatbin(trace_lib))
    assert len(objs) == 2                                        # still the EXACT and the FAST unit
    dc = DeviceCode(trace_lib)
    exact = dc.unit_of_kernel("state_advance_kernel")
    assert exact is not None and exact == dc.unit_of_kernel("ggx_direct_emit_kernel<4, 0>")
    for k in KERNELS:                                            # mode-free: one copy, in the EXACT unit
        assert dc.unit_of_kernel(k) == exact, k
        assert sum(k.encode() in elf for elf in objs) == 1, k
    main = build.build_library()
    for elf in code_objects(fatbin(main)):
        for k in KERNELS:
            assert k.encode() not in elf, k
    recorded = json.loads((ROOT / "profiles" / "r06_library_id.json").read_text())
    assert DeviceCode(main).library_id == recorded["library_id"]


def test_the_scratch_size(trace_lib):
    """(bins + 1) x tiles counts and the grand total, then the scan's tile sums, each part rounded up to 256 bytes"""
    from rlshaders_amd import trace
    tile = 2048
    up = lambda b: (b + 255) // 256 * 256
    for rays, bins in ((0, 1), (1, 1), (tile, 3), (tile + 1, 3), (1 << 24, 16), ((1 << 32) - 1, 16)):
        tiles = (rays + tile - 1) // tile
        cells = (bins + 1) * tiles
        assert trace.route_scratch_bytes(rays, bins) == up(8 * (cells + 1)) + up(8 * max((cells + tile - 1) // tile, 1)), (rays, bins)
