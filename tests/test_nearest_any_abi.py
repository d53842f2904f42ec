"""CPU: the ABI of the any-hit companion library (include/rlshaders_amd_nearest_any.h, librls_nearest_any.so,
rlshaders_amd/nearest_any.py).

The header declares, the library exports and nearest_any.PROTOTYPES binds the same entry points with the same arity; the
ctypes.Structure of nearest_any.py mirrors the header's struct in member order, sizeof and every offsetof (from a compiled probe),
and the module's constants are the header's; the header is C99 / C++14 clean, includes the nearest-hit header alone and restates
neither rls_nearest_rays nor rls_walk_rays; the library holds ONE gfx950 code object of its own two kernels, which use no scratch
memory and spill no register, the query kernel with 24 KiB of LDS; it links the product library by $ORIGIN and no other
companion; no other library, header or module knows an rls_nearest_any_ name, and the four other nearest libraries keep their
device code; every argument check refuses with "<entry>: <text>" over dummy memory (no device needed), the layout tag of a scene
included, and each message is written once."""
import ctypes as C
import inspect
import re
import subprocess

import pytest

from nearest_abi_util import NearestWorld, compiled_layout, exported_symbols, header_abi, scene_layout_tag
from trace_abi_util import ROOT, code_text, dynamic_symbols, put, refusals

HEADER = ROOT / "include" / "rlshaders_amd_nearest_any.h"
CSRC = ROOT / "rlshaders_amd" / "csrc_nearest"
HIP = CSRC / "any.hip"
ARITY = dict(rls_nearest_any_hits=4, rls_nearest_any_walk_hits=5, rls_nearest_any_opaque=4)
STRUCTS = ["rls_nearest_any_found"]
CONSTANTS = dict(RLS_NEAREST_ANY_CLEAR=0, RLS_NEAREST_ANY_BLOCKED=1, RLS_NEAREST_ANY_VEILED=2)
# the device code of the four other nearest libraries, as it was before this library came (rlshaders_amd/codeid.py)
OTHERS_DEVICE_CODE = dict(nearest="73baa46bb6e900d2", nearest_refit="6e73042cb8ac0f11", nearest_rebuild="f9976b180359b396",
                          nearest_group="c3e4471a22bd3a12")
LAYOUT = "scene is not a scene of this build's layout (librls_nearest.so and librls_nearest_any.so must be of one build)"

declared_symbols, declarations, structs, struct_members = header_abi(HEADER, "rls_nearest_any_")


@pytest.fixture(scope="module")
def any_lib():
    from rlshaders_amd import build
    return build.build_nearest_any_library()


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_exports_exactly_the_header_and_the_bindings(any_lib):
    from rlshaders_amd import nearest_any
    declared, decl = declared_symbols(), declarations()
    assert declared and all(s.startswith("rls_nearest_any_") for s in declared), declared
    assert exported_symbols(any_lib) == declared
    assert sorted(nearest_any.PROTOTYPES) == declared == sorted(decl) == sorted(ARITY)
    lib, out = nearest_any.load(), dynamic_symbols(any_lib)
    for name, n in ARITY.items():
        assert len(decl[name].split(",")) == n, (name, decl[name])
        assert f" T {name}\n" in out, name
        restype, argtypes = nearest_any.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == n and getattr(lib, name).argtypes == argtypes, name
    assert list(inspect.signature(nearest_any.shadow).parameters)[:7] == ["queue", "O", "scene", "opacity_table", "max_steps", "base", "last"]
    assert list(inspect.signature(nearest_any.opaque_flags).parameters)[:2] == ["ctx", "table"]
    assert callable(nearest_any.hits) and callable(nearest_any.load)
    for name, value in CONSTANTS.items():
        assert getattr(nearest_any, name) == value, name
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, code_text(HEADER)).group(1)) == value, name


def test_no_other_library_header_or_module_knows_the_query(any_lib):
    from rlshaders_amd import _capi, build, nearest, nearest_group, nearest_rebuild, nearest_refit, shadow_walk, trace, walk
    from rlshaders_amd.codeid import DeviceCode
    libs = dict(nearest=build.build_nearest_library(), nearest_refit=build.build_nearest_refit_library(),
                nearest_rebuild=build.build_nearest_rebuild_library(), nearest_group=build.build_nearest_group_library())
    build.build_trace_library(), build.build_walk_library(), build.build_shadow_walk_library()
    for lib in (build.LIB, build.TRACE_LIB, build.WALK_LIB, build.SHADOW_WALK_LIB, build.RR_LIB, *libs.values()):
        assert "rls_nearest_any_" not in dynamic_symbols(lib), lib
        assert b"rls_nearest_any" not in lib.read_bytes(), lib
    assert not [s for m in (_capi, trace, walk, shadow_walk, nearest, nearest_refit, nearest_rebuild, nearest_group) for s in m.PROTOTYPES
                if s.startswith("rls_nearest_any_")]
    for h in sorted((ROOT / "include").glob("*.h")):
        if h != HEADER:
            assert "nearest_any" not in h.read_text(), h
    for m in sorted((ROOT / "rlshaders_amd").glob("*.py")):
        if m.name not in ("nearest_any.py", "build.py"):
            assert "nearest_any" not in m.read_text(), m
    # the four other nearest libraries keep their device code: nothing they compile was edited
    for name, lib in libs.items():
        assert DeviceCode(lib).library_id == OTHERS_DEVICE_CODE[name], name
    # it reads a scene through the private header alone, takes the slab and triangle tests from the nearest-hit library's kernel
    # header without its kernel, and includes no other library's unit
    text = re.sub(r"//[^\n]*", "", HIP.read_text() + (CSRC / "rls_nearest_any.hpp").read_text())
    assert '#include "rls_nearest_scene.hpp"' in text and '#include "rls_nearest_device.hpp"' in text
    assert "#define RLS_NEAREST_DEVICE_NO_KERNEL 1" in text
    for unit in ("nearest.hip", "refit.hip", "rebuild.hip", "group.hip", "rls_nearest_update.hpp", "rls_nearest_group.hpp"):
        assert unit not in text, unit
    for own in ("nearest_triangle", "nearest_slab", "nearest_candidate", "nearest_traverse"):
        assert not re.search(r"\b(void|bool|NearestBest)\s+" + own + r"\s*\(", text), own            # used or left alone, not written again
    assert "nearest_slab(" in text and "nearest_triangle(" in text
    assert "visits < node_count" in text and "sp < kNearestStack" in text


# ---- the struct: nearest_any.py against the compiler ---------------------------------------------------------------------------------
def test_the_struct_mirror_has_the_headers_layout(tmp_path):
    from rlshaders_amd import nearest_any
    probe = compiled_layout(tmp_path, HEADER, structs, struct_members)
    assert structs() == STRUCTS
    cls = nearest_any.NearestAnyFound_
    assert cls.__doc__ == "rls_nearest_any_found"
    assert [f[0] for f in cls._fields_] == struct_members("rls_nearest_any_found") == \
        ["state", "opaque", "opaque_count", "base", "visibility", "reach", "last"]
    assert C.sizeof(cls) == probe["sizeof rls_nearest_any_found"]
    for f, _ in cls._fields_:
        assert getattr(cls, f).offset == probe[f"rls_nearest_any_found.{f}"], f
    assert re.findall(r'#include\s+"([^"]+)"', HEADER.read_text()) == ["rlshaders_amd_nearest.h"]
    for other in ("rls_nearest_rays", "rls_walk_rays"):                                               # reused, not restated
        assert not re.search(r"typedef struct %s\b" % other, code_text(HEADER)), other


# ---- the header ----------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_cxx(tmp_path):
    body = ("rls_nearest_any_found f = {0}; rls_nearest_rays r = {0}; rls_walk_rays l = {0}; rls_crgb o = {0}; rls_nearest_scene *s = 0; "
            "return (int)rls_nearest_any_hits(0, s, &r, &f) + (int)rls_nearest_any_walk_hits(0, s, &l, -1, &f) + "
            "(int)rls_nearest_any_opaque(0, &o, 0, 0) + RLS_NEAREST_ANY_CLEAR + RLS_NEAREST_ANY_BLOCKED + RLS_NEAREST_ANY_VEILED;")
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_nearest_any.h"\nint main(void){ ' + body + ' }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-Wno-missing-field-initializers", "-Wno-missing-braces",
                            "-fsyntax-only", f"-I{ROOT / 'include'}", "-x", "c" if cc == "gcc" else "c++", str(src)],
                           capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)


# ---- the device code -----------------------------------------------------------------------------------------------------------
def test_one_gfx950_code_object_no_scratch_no_spill(any_lib, tmp_path):
    from rlshaders_amd.codeid import code_objects, fatbin, kernel_digests
    objs = code_objects(fatbin(any_lib))
    assert len(objs) == 1 and b"gfx950" in objs[0]
    kernels = list(kernel_digests(objs[0]))
    want = ("any_kernel", "any_flags_kernel")
    assert len(kernels) == len(want) and all(any(k in name for name in kernels) for k in want), kernels     # no other library's
    d = subprocess.run(["readelf", "-d", str(any_lib)], capture_output=True, text=True, check=True).stdout
    assert "[librlshaders_amd.so]" in d and "$ORIGIN" in d
    for other in ("librls_trace", "librls_walk", "librls_shadow_walk", "librls_nearest", "librls_ggx_rr"):
        assert other not in d.replace("librls_nearest_any", ""), other
    (tmp_path / "any.co").write_bytes(objs[0])
    note = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(tmp_path / "any.co")], capture_output=True,
                          text=True, check=True).stdout
    private = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", note)
    vspills = re.findall(r"\.vgpr_spill_count:\s*(\d+)", note)
    sspills = re.findall(r"\.sgpr_spill_count:\s*(\d+)", note)
    assert len(private) == len(vspills) == len(sspills) == len(kernels), note[-3000:]
    # no scratch memory, and no register spilled anywhere, scalar ones included
    assert set(private) == {"0"} and set(vspills) == {"0"} and set(sspills) == {"0"}, note[-3000:]
    # the stacks of 256 lanes in LDS, 24 words a lane; the flag kernel has none
    assert sorted(re.findall(r"\.group_segment_fixed_size:\s*(\d+)", note)) == sorted(["0", str(24 * 256 * 4)]), note[-3000:]
    print("resources:", {k: re.findall(r"\.%s:\s*(\d+)" % k, note) for k in ("sgpr_count", "vgpr_count", "group_segment_fixed_size")},
          re.findall(r"\.name:\s*(\S+)", note))


# ---- the refusals: no device needed ------------------------------------------------------------------------------------------------
class AnyWorld(NearestWorld):
    """NearestWorld's rays and list, a scene of 4 KiB that starts with this build's layout tag and device 0 (the dummy context's)
    -- the struct leads with just these members, so every check is reached; a refused call reads nothing else -- and every
    found plane set over dummy memory."""

    def __init__(self):
        super().__init__()
        from rlshaders_amd import nearest_any
        capi = self.capi
        self.mod, self.alib = nearest_any, nearest_any.load()
        self.scene_mem = C.create_string_buffer(4096)
        C.c_uint64.from_buffer(self.scene_mem, 0).value = scene_layout_tag()
        self.scenep = C.addressof(self.scene_mem)
        p = self.p
        self.af = nearest_any.NearestAnyFound_(p, p, 4, self.v3(capi.CRgb), self.v3(capi.Rgb), p, p)
        self.afp = C.byref(self.af)
        self.opacity = self.v3(capi.CRgb)
        self.opacityp, self.surfaces, self.flagsp = C.byref(self.opacity), 4, p

    def hits(self):
        return self.alib.rls_nearest_any_hits(self.ctxp, self.scenep, self.rp, self.afp)

    def walk_hits(self):
        return self.alib.rls_nearest_any_walk_hits(self.ctxp, self.scenep, self.listp, self.bound, self.afp)

    def opaque(self):
        return self.alib.rls_nearest_any_opaque(self.ctxp, self.opacityp, self.surfaces, self.flagsp)


def _tables():
    ctx = ("ctx NULL", lambda w: put(w, "ctxp", None), "ctx is NULL")
    scene = ("scene NULL", lambda w: put(w, "scenep", None), "scene is NULL")
    found = [
        ("found NULL", lambda w: put(w, "afp", None), "found is NULL"),
        ("state NULL", lambda w: put(w.af, "state", None), "found.state plane is NULL"),
        ("opaque with count 0", lambda w: put(w.af, "opaque_count", 0), "found.opaque is set with found.opaque_count == 0"),
        ("base partly", lambda w: put(w.af, "base", w.half3(w.capi.CRgb)), "found.base or found.visibility is partly NULL: all three planes or none"),
        ("visibility partly", lambda w: put(w.af, "visibility", w.half3(w.capi.Rgb)),
         "found.base or found.visibility is partly NULL: all three planes or none"),
        ("a zeroed scene", lambda w: put(w, "scenep", w.p), LAYOUT),
        ("another layout", lambda w: C.c_uint64.from_buffer(w.scene_mem, 0).__setattr__("value", scene_layout_tag() - 1), LAYOUT),
        ("another device", lambda w: C.c_int.from_buffer(w.scene_mem, 8).__setattr__("value", 1), "the scene lives on another device than ctx"),
    ]
    return dict(
        hits=[
            ctx, scene,
            ("rays NULL", lambda w: put(w, "rp", None), "rays is NULL"),
            ("rays < 0", lambda w: put(w.r, "rays", -1), "rays < 0"),
            ("rays past 2^32", lambda w: put(w.r, "rays", 1 << 32), "rays > 2^32 - 1 (a ray id is 32-bit)"),
            ("origin NULL", lambda w: put(w.r, "origin", w.none3(w.capi.CVec3)), "rays.origin or rays.dir plane is NULL"),
            ("dir partly", lambda w: put(w.r, "dir", w.half3(w.capi.CVec3)), "rays.origin or rays.dir plane is NULL"),
            *found,
        ],
        walk_hits=[
            ctx, scene,
            ("list NULL", lambda w: put(w, "listp", None), "list is NULL"),
            ("count NULL", lambda w: put(w.list, "count", None), "list.count is NULL"),
            ("capacity < 0", lambda w: put(w.list, "capacity", -1), "list.capacity < 0"),
            ("ray NULL", lambda w: put(w.list, "ray", None), "list.ray or list.maxdist plane is NULL"),
            ("maxdist NULL", lambda w: put(w.list, "maxdist", None), "list.ray or list.maxdist plane is NULL"),
            *found,
        ],
        opaque=[
            ctx,
            ("opacity NULL", lambda w: put(w, "opacityp", None), "opacity or one of its planes is NULL"),
            ("opacity partly", lambda w: put(w, "opacityp", C.byref(w.half3(w.capi.CRgb))), "opacity or one of its planes is NULL"),
            ("flags NULL", lambda w: put(w, "flagsp", None), "flags is NULL"),
        ])


TABLES = _tables()


@pytest.mark.parametrize("verb", list(TABLES))
def test_every_argument_check_refuses_by_name(any_lib, verb):
    wrong = refusals(AnyWorld, getattr(AnyWorld, verb), "rls_nearest_any_" + verb, TABLES[verb])
    assert not wrong, "\n".join(wrong)


def test_empty_queries_are_accepted_without_planes(any_lib):
    w = AnyWorld()
    w.r.rays = 0                                                     # no rays: accepted, nothing launched, the planes not asked for
    w.af.state = None
    assert w.hits() == 0
    w.surfaces, w.opacityp, w.flagsp = 0, None, None
    assert w.opaque() == 0
    w = AnyWorld()
    w.af.opaque, w.af.opaque_count = None, 0                         # no table: a count of 0 is what it is
    w.r.rays = 0
    assert w.hits() == 0


def test_the_checks_are_written_once():
    """every message of any.hip's argument checks appears once in it, but for the entry points' own first lines, and every message
    the tables above ask for is one of them"""
    text = HIP.read_text()
    messages = re.findall(r'RLS_REQUIRE(?:_IN)?\([^;]*?"([^"]+)"\s*\)\s*;', text, flags=re.S)
    assert len(messages) >= 15, len(messages)
    twice = sorted(m for m in set(messages) if messages.count(m) > 1)
    assert twice == ["ctx is NULL", "scene is NULL"], twice
    for _, _, want in sum(TABLES.values(), []):
        assert text.count(f'"{want}"') >= 1 or want == LAYOUT, want
    assert text.count("scene is not a scene of this build's layout") == 1
