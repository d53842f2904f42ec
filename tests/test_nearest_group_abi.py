"""CPU: the ABI of the instanced-scene companion library (include/rlshaders_amd_nearest_group.h, librls_nearest_group.so,
rlshaders_amd/nearest_group.py).

The header declares, the library exports and nearest_group.PROTOTYPES binds the same entry points with the same arity; every
ctypes.Structure of nearest_group.py mirrors one struct of the header in member order, array lengths, sizeof and every offsetof
(from a compiled probe), and the module's constants are the header's; the header is C99 / C++14 clean and includes the
nearest-hit header alone; the library holds ONE gfx950 code object of its own kernels (no other library's), which use no scratch
memory and spill no vector register, the query kernel with 40 KiB of LDS; it links the product library by $ORIGIN and no other companion;
no other library, header or module knows an rls_nearest_group_ name, and the three other nearest libraries keep their device
code; every argument check refuses with "<entry>: <text>" over dummy memory (no device needed), the layout tag of a scene
included, and each message is written once."""
import ctypes as C
import inspect
import re
import subprocess

import pytest

from nearest_abi_util import NearestWorld, compiled_layout, exported_symbols, scene_layout_tag
from trace_abi_util import ROOT, code_text, dynamic_symbols, put, refusals

HEADER = ROOT / "include" / "rlshaders_amd_nearest_group.h"
CSRC = ROOT / "rlshaders_amd" / "csrc_nearest"
HIP = CSRC / "group.hip"
ARITY = dict(rls_nearest_group_create=5, rls_nearest_group_destroy=1, rls_nearest_group_get_info=2, rls_nearest_group_update=3,
             rls_nearest_group_hits=4, rls_nearest_group_walk_hits=5, rls_nearest_group_read_tree=7)
STRUCTS = ["rls_nearest_group_found", "rls_nearest_group_info", "rls_nearest_group_moves", "rls_nearest_instance"]
CONSTANTS = dict(RLS_NEAREST_GROUP_STACK=16, RLS_NEAREST_GROUP_MAX_INSTANCES=1 << 16, RLS_NEAREST_GROUP_MAX_LEAF=4,
                 RLS_NEAREST_GROUP_DEFAULT_LEAF=2, RLS_NEAREST_NO_INSTANCE=0xFFFFFFFF)
# the device code of the three other nearest libraries, as it was before this library came (rlshaders_amd/codeid.py)
OTHERS_DEVICE_CODE = dict(nearest="73baa46bb6e900d2", nearest_refit="6e73042cb8ac0f11", nearest_rebuild="f9976b180359b396")
LAYOUT = "an instance's scene is not a scene of this build's layout (librls_nearest.so and librls_nearest_group.so must be of one build)"


@pytest.fixture(scope="module")
def group_lib():
    from rlshaders_amd import build
    return build.build_nearest_group_library()


def declared_symbols():
    return sorted(set(re.findall(r"\b(rls_[a-z0-9_]+)\s*\(", code_text(HEADER))))


def declarations():
    return {m.group(1): m.group(2)
            for m in re.finditer(r"rls_status\s+(rls_nearest_group_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code_text(HEADER), flags=re.S)}


def structs():
    return re.findall(r"typedef struct (\w+)\s*\{", code_text(HEADER))


def struct_members(c_name):
    """[(member, array length or None)] in the header's order"""
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (c_name, c_name), code_text(HEADER), flags=re.S).group(1)
    out = []
    for d in body.split(";"):
        for part in d.split(",") if d.strip() else []:
            m = re.search(r"(\w+)\s*(?:\[(\d+)\])?\s*$", part.strip())
            out.append((m.group(1), int(m.group(2)) if m.group(2) else None))
    return out


def mirrors():
    from rlshaders_amd import nearest_group
    classes = [c for _, c in inspect.getmembers(nearest_group, inspect.isclass)
               if issubclass(c, C.Structure) and c.__module__ == nearest_group.__name__]
    assert len({c.__doc__ for c in classes}) == len(classes)
    return {c.__doc__: c for c in classes}


# ---- the surface ---------------------------------------------------------------------------------------------------------------
def test_exports_exactly_the_header_and_the_bindings(group_lib):
    from rlshaders_amd import nearest_group
    declared, decl = declared_symbols(), declarations()
    assert declared and all(s.startswith("rls_nearest_group_") for s in declared), declared
    assert exported_symbols(group_lib) == declared
    assert sorted(nearest_group.PROTOTYPES) == declared == sorted(decl) == sorted(ARITY)
    lib, out = nearest_group.load(), dynamic_symbols(group_lib)
    for name, n in ARITY.items():
        assert len(decl[name].split(",")) == n, (name, decl[name])
        assert f" T {name}\n" in out, name
        restype, argtypes = nearest_group.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == n and getattr(lib, name).argtypes == argtypes, name
    assert all(callable(getattr(nearest_group.Group, m)) for m in ("hits", "update", "read_tree", "info", "close"))
    assert list(inspect.signature(nearest_group.Group.__init__).parameters) == ["self", "ctx", "instances", "leaf_size"]
    assert list(inspect.signature(nearest_group.Group.update).parameters)[:4] == ["self", "to_object", "to_world", "parked"]
    assert list(inspect.signature(nearest_group.Instance.__init__).parameters) == ["self", "scene", "to_world", "surface_base", "to_object"]
    assert all(callable(getattr(nearest_group.Found, m)) for m in ("walk_found", "shadow_found", "bins", "gatherable"))
    for name, value in CONSTANTS.items():
        assert getattr(nearest_group, name) == value, name
        spelled = re.search(r"#define\s+%s\s+(.+)" % name, code_text(HEADER)).group(1).strip()
        assert eval(re.sub(r"\(int64_t\)|u\b", "", spelled)) == value, (name, spelled)


def test_no_other_library_header_or_module_knows_the_group(group_lib):
    from rlshaders_amd import _capi, build, nearest, nearest_rebuild, nearest_refit, shadow_walk, trace, walk
    from rlshaders_amd.codeid import DeviceCode
    libs = dict(nearest=build.build_nearest_library(), nearest_refit=build.build_nearest_refit_library(),
                nearest_rebuild=build.build_nearest_rebuild_library())
    build.build_trace_library(), build.build_walk_library(), build.build_shadow_walk_library()
    for lib in (build.LIB, build.TRACE_LIB, build.WALK_LIB, build.SHADOW_WALK_LIB, build.RR_LIB, *libs.values()):
        assert "rls_nearest_group_" not in dynamic_symbols(lib), lib
        assert b"rls_nearest_group" not in lib.read_bytes(), lib
    assert not [s for m in (_capi, trace, walk, shadow_walk, nearest, nearest_refit, nearest_rebuild) for s in m.PROTOTYPES
                if s.startswith("rls_nearest_group_")]
    for h in sorted((ROOT / "include").glob("*.h")):
        if h != HEADER:
            assert "nearest_group" not in h.read_text(), h
    for m in sorted((ROOT / "rlshaders_amd").glob("*.py")):
        if m.name not in ("nearest_group.py", "build.py"):
            assert "nearest_group" not in m.read_text(), m
    # the slab routine has a variant of its own here, and the shared headers gained two preprocessor guards: the three other
    # nearest libraries keep their device code
    for name, lib in libs.items():
        assert DeviceCode(lib).library_id == OTHERS_DEVICE_CODE[name], name
    # it reads a scene through the private header alone and includes no other library's unit
    text = re.sub(r"//[^\n]*", "", HIP.read_text() + (CSRC / "rls_nearest_group.hpp").read_text())
    assert '#include "rls_nearest_scene.hpp"' in text and '#include "rls_nearest_device.hpp"' in text
    for unit in ("nearest.hip", "refit.hip", "rebuild.hip", "rls_nearest_update.hpp", "rls_nearest_rebuild.hpp"):
        assert unit not in text, unit
    for own in ("nearest_triangle", "nearest_slab", "nearest_normalize", "refit_union", "refit_levels"):
        assert not re.search(r"\b(void|bool)\s+" + own + r"\s*\(", text), own                # used, not written again


# ---- structs: nearest_group.py against the compiler --------------------------------------------------------------------------------
def test_every_struct_mirror_has_the_headers_layout(tmp_path):
    probe = compiled_layout(tmp_path, HEADER, structs, lambda c: [m for m, _ in struct_members(c)])
    assert sorted(mirrors()) == sorted(structs()) == STRUCTS
    for c_name, cls in mirrors().items():
        fields = [(f[0], f[1]._length_ if issubclass(f[1], C.Array) else None) for f in cls._fields_]
        assert fields == struct_members(c_name), c_name
        assert C.sizeof(cls) == probe[f"sizeof {c_name}"], c_name
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == probe[f"{c_name}.{f}"], (c_name, f)
    assert struct_members("rls_nearest_instance") == [("scene", None), ("to_object", 12), ("to_world", 12), ("surface_base", None)]
    assert [m for m, _ in struct_members("rls_nearest_group_info")] == ["instances", "scenes", "top_nodes", "top_depth", "leaf_size",
                                                                        "device_bytes", "updates"]
    assert [m for m, _ in struct_members("rls_nearest_group_moves")] == ["to_object", "to_world", "parked"]
    assert [m for m, _ in struct_members("rls_nearest_group_found")] == ["found", "instance", "last_instance"]
    assert re.findall(r'#include\s+"([^"]+)"', HEADER.read_text()) == ["rlshaders_amd_nearest.h"]


# ---- the header ----------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c_and_cxx(tmp_path):
    body = ("rls_nearest_instance i = {0}; rls_nearest_group_info n = {0}; rls_nearest_group_moves m = {0}; rls_nearest_group_found f = {0}; "
            "rls_nearest_rays r = {0}; rls_walk_rays l = {0}; rls_nearest_group *g = 0; "
            "return (int)rls_nearest_group_create(0, &i, 1, 0, &g) + (int)rls_nearest_group_update(0, g, &m) + "
            "(int)rls_nearest_group_get_info(g, &n) + (int)rls_nearest_group_hits(0, g, &r, &f) + "
            "(int)rls_nearest_group_walk_hits(0, g, &l, -1, &f) + (int)rls_nearest_group_read_tree(0, g, 0, 0, 0, 0, 0) + "
            "(int)rls_nearest_group_destroy(g) + (int)(RLS_NEAREST_GROUP_MAX_INSTANCES >> RLS_NEAREST_GROUP_STACK) + "
            "(int)(RLS_NEAREST_NO_INSTANCE & RLS_NEAREST_GROUP_MAX_LEAF & RLS_NEAREST_GROUP_DEFAULT_LEAF);")
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_nearest_group.h"\nint main(void){ ' + body + ' }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-Wno-missing-field-initializers", "-Wno-missing-braces",
                            "-fsyntax-only", f"-I{ROOT / 'include'}", "-x", "c" if cc == "gcc" else "c++", str(src)],
                           capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)
    text = HEADER.read_text()
    for must in ("THE STATEMENT", "PARKED", "MIRRORING", "BORROWS", "never inverts", "2^-21", "last_instance", "no float atomics", "tn_top <= tnW_j"):
        assert must in text, must


# ---- the device code -----------------------------------------------------------------------------------------------------------
def test_one_gfx950_code_object_no_scratch_no_spill(group_lib, tmp_path):
    from rlshaders_amd.codeid import code_objects, fatbin, kernel_digests
    objs = code_objects(fatbin(group_lib))
    assert len(objs) == 1 and b"gfx950" in objs[0]
    kernels = list(kernel_digests(objs[0]))
    want = ("group_kernel", "group_records_kernel", "group_level_kernel", "group_top_kernel")
    assert len(kernels) == len(want) and all(any(k in name for name in kernels) for k in want), kernels     # no other library's
    d = subprocess.run(["readelf", "-d", str(group_lib)], capture_output=True, text=True, check=True).stdout
    assert "[librlshaders_amd.so]" in d and "$ORIGIN" in d
    for other in ("librls_trace", "librls_walk", "librls_shadow_walk", "librls_nearest", "librls_ggx_rr"):
        assert other not in d.replace("librls_nearest_group", ""), other
    (tmp_path / "group.co").write_bytes(objs[0])
    note = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", str(tmp_path / "group.co")], capture_output=True,
                          text=True, check=True).stdout
    private = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", note)
    vspills = re.findall(r"\.vgpr_spill_count:\s*(\d+)", note)
    sspills = re.findall(r"\.sgpr_spill_count:\s*(\d+)", note)
    assert len(private) == len(vspills) == len(sspills) == len(kernels), note[-3000:]
    # no scratch memory and no vector register spilled anywhere.  The query kernel holds some forty plane pointers of its
    # argument beside two levels of traversal state and parks scalar registers in vector LANES (94 of them; no memory is touched);
    # the three update kernels park none
    assert set(private) == {"0"} and set(vspills) == {"0"} and sorted(sspills).count("0") == 3, note[-3000:]
    # both stacks of 256 lanes in LDS: (16 + 24) words a lane
    assert str((16 + 24) * 256 * 4) in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", note), note[-3000:]


# ---- the refusals: no device needed ------------------------------------------------------------------------------------------------
class GroupWorld(NearestWorld):
    """NearestWorld's rays, list and found planes, one instance whose scene is 4 KiB that start with this build's layout tag and
    device 0 (the dummy context's), and a group handle of 4 KiB that starts with a public info struct and device 0 -- the two
    structs lead with just these members, so every check is reached; a refused call reads nothing else."""

    def __init__(self):
        super().__init__()
        from rlshaders_amd import nearest_group
        self.mod, self.glib = nearest_group, nearest_group.load()
        self.scene = C.create_string_buffer(4096)
        C.c_uint64.from_buffer(self.scene, 0).value = scene_layout_tag()
        self.instances = (nearest_group.NearestInstance_ * 2)()
        for i in self.instances:
            i.scene = C.addressof(self.scene)
        self.count, self.leaf = 2, 0
        self.instancesp = C.cast(self.instances, C.c_void_p)
        self.handle = C.create_string_buffer(4096)
        self.handle_info = nearest_group.NearestGroupInfo_.from_buffer(self.handle, 0)
        self.handle_info.instances = 2
        self.handlep = C.addressof(self.handle)
        self.out = C.c_void_p()
        self.outp = C.byref(self.out)
        self.moves = nearest_group.NearestGroupMoves_(self.p, self.p, self.p)
        self.movesp = C.byref(self.moves)
        self.gf = nearest_group.NearestGroupFound_(self.f, self.p, self.p)
        self.gfp = C.byref(self.gf)
        self.ginfo = nearest_group.NearestGroupInfo_()
        self.ginfop = C.byref(self.ginfo)

    def handle_device(self, device):
        C.c_int.from_buffer(self.handle, C.sizeof(self.ginfo)).value = device

    def create(self):
        return self.glib.rls_nearest_group_create(self.ctxp, C.cast(self.instancesp, C.POINTER(self.mod.NearestInstance_)), self.count,
                                                  self.leaf, self.outp)

    def update(self):
        return self.glib.rls_nearest_group_update(self.ctxp, self.handlep, self.movesp)

    def hits(self):
        return self.glib.rls_nearest_group_hits(self.ctxp, self.handlep, self.rp, self.gfp)

    def walk_hits(self):
        return self.glib.rls_nearest_group_walk_hits(self.ctxp, self.handlep, self.listp, self.bound, self.gfp)

    def get_info(self):
        return self.glib.rls_nearest_group_get_info(self.handlep, self.ginfop)

    def read_tree(self):
        return self.glib.rls_nearest_group_read_tree(self.ctxp, self.handlep, self.p, self.p, self.p, self.p, self.p)


def _tables():
    ctx = ("ctx NULL", lambda w: put(w, "ctxp", None), "ctx is NULL")
    group = ("group NULL", lambda w: put(w, "handlep", None), "group is NULL")
    device = ("another device", lambda w: w.handle_device(1), "the group lives on another device than ctx")
    found = [
        ("found NULL", lambda w: put(w, "gfp", None), "found is NULL"),
        ("hit NULL", lambda w: put(w.gf.found, "hit", None), "found.hit or found.t plane is NULL"),
        ("t NULL", lambda w: put(w.gf.found, "t", None), "found.hit or found.t plane is NULL"),
        ("N partly", lambda w: put(w.gf.found, "N", w.half3(w.capi.Vec3)), "found.P, N, Ns, T or wo is partly NULL: all three planes or none"),
        ("bin without a table", lambda w: put(w.gf.found, "bin_of_surface", None),
         "found.bin is set with found.bin_of_surface NULL or found.bin_count == 0"),
        ("bin_count 0", lambda w: put(w.gf.found, "bin_count", 0), "found.bin is set with found.bin_of_surface NULL or found.bin_count == 0"),
        ("last alone", lambda w: put(w.gf, "last_instance", None), "found.last and last_instance are a pair: both or neither"),
        ("last_instance alone", lambda w: put(w.gf.found, "last", None), "found.last and last_instance are a pair: both or neither"),
        device,
    ]
    return dict(
        create=[
            ctx,
            ("out NULL", lambda w: put(w, "outp", None), "out is NULL"),
            ("count < 0", lambda w: put(w, "count", -1), "count < 0"),
            ("count past the limit", lambda w: put(w, "count", (1 << 16) + 1), "count > 2^16: the top stack of 16 entries bounds the top tree's depth"),
            ("leaf 5", lambda w: put(w, "leaf", 5), "leaf_size must be in [1, 4], or 0 for the default"),
            ("leaf -1", lambda w: put(w, "leaf", -1), "leaf_size must be in [1, 4], or 0 for the default"),
            ("instances NULL", lambda w: put(w, "instancesp", C.c_void_p(None)), "instances is NULL"),
            ("scene NULL", lambda w: put(w.instances[1], "scene", None), "an instance's scene is NULL"),
            ("a zeroed scene", lambda w: put(w.instances[1], "scene", w.p), LAYOUT),
            ("another layout", lambda w: C.c_uint64.from_buffer(w.scene, 0).__setattr__("value", scene_layout_tag() - 1), LAYOUT),
            ("another device", lambda w: C.c_int.from_buffer(w.scene, 8).__setattr__("value", 1), "an instance's scene lives on another device than ctx"),
        ],
        update=[
            ctx, group,
            ("moves NULL", lambda w: put(w, "movesp", None), "moves is NULL"),
            ("to_world alone", lambda w: put(w.moves, "to_object", None), "moves.to_object and moves.to_world: both planes or neither"),
            ("to_object alone", lambda w: put(w.moves, "to_world", None), "moves.to_object and moves.to_world: both planes or neither"),
            device,
        ],
        hits=[
            ctx, group,
            ("rays NULL", lambda w: put(w, "rp", None), "rays is NULL"),
            ("rays < 0", lambda w: put(w.r, "rays", -1), "rays < 0"),
            ("rays past 2^32", lambda w: put(w.r, "rays", 1 << 32), "rays > 2^32 - 1 (a ray id is 32-bit)"),
            ("origin NULL", lambda w: put(w.r, "origin", w.none3(w.capi.CVec3)), "rays.origin or rays.dir plane is NULL"),
            ("dir partly", lambda w: put(w.r, "dir", w.half3(w.capi.CVec3)), "rays.origin or rays.dir plane is NULL"),
            *found,
        ],
        walk_hits=[
            ctx, group,
            ("list NULL", lambda w: put(w, "listp", None), "list is NULL"),
            ("count NULL", lambda w: put(w.list, "count", None), "list.count is NULL"),
            ("capacity < 0", lambda w: put(w.list, "capacity", -1), "list.capacity < 0"),
            ("ray NULL", lambda w: put(w.list, "ray", None), "list.ray or list.maxdist plane is NULL"),
            ("maxdist NULL", lambda w: put(w.list, "maxdist", None), "list.ray or list.maxdist plane is NULL"),
            *found,
        ],
        get_info=[group, ("info NULL", lambda w: put(w, "ginfop", None), "info is NULL")],
        read_tree=[ctx, group, device])


TABLES = _tables()


@pytest.mark.parametrize("verb", list(TABLES))
def test_every_argument_check_refuses_by_name(group_lib, verb):
    wrong = refusals(GroupWorld, getattr(GroupWorld, verb), "rls_nearest_group_" + verb, TABLES[verb])
    assert not wrong, "\n".join(wrong)


def test_info_of_dummy_memory_destroy_of_null_and_empty_queries(group_lib):
    w = GroupWorld()
    assert w.get_info() == 0 and (w.ginfo.instances, w.ginfo.updates) == (2, 0)
    assert w.glib.rls_nearest_group_destroy(None) == 0
    assert w.out.value is None
    w.r.rays = 0                                                     # no rays: accepted, nothing launched, the planes not asked for
    assert w.hits() == 0


def test_the_checks_are_written_once():
    """every message of group.hip's argument checks appears once in it, but for the entry points' own first lines, and every message
    the tables above ask for is one of them"""
    text = HIP.read_text()
    messages = re.findall(r'RLS_REQUIRE(?:_IN)?\([^;]*?"([^"]+)"\s*\)\s*;', text, flags=re.S)
    assert len(messages) >= 30, len(messages)
    twice = sorted(m for m in set(messages) if messages.count(m) > 1)
    assert twice == ["ctx is NULL", "group is NULL", "the group lives on another device than ctx"], twice
    for _, _, want in sum(TABLES.values(), []):
        assert text.count(f'"{want}"') >= 1 or want == LAYOUT, want
    assert text.count("an instance's scene is not a scene of this build's layout") == 1
