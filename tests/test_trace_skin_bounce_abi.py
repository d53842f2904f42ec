"""CPU: the secondary-ray calls of the caller-traced rlSkin node (rls_trace_skin_bounce_emit / rls_trace_skin_bounce_resolve;
include/rlshaders_amd_trace.h, librls_trace.so).

Both symbols are declared, exported and bound with matching arity (12 and 14); the two new structs have the header's members in
its order and embed the node's structs unchanged; the header compiles as C99 and C++14; the library still holds two code objects,
each with the state-aware kernels beside their parents; and every refusal -- the node calls' table (tests/test_trace_skin_abi.py),
the state's (tests/test_trace_bounce_abi.py) and the sixth queue's -- returns RLS_ERR_INVALID_ARGUMENT with the entry point's
name in the message.  The checks run through ctypes with dummy planes and a dummy context: a refused call returns before the
context is read."""
import ctypes as C
import re
import subprocess

import pytest

from test_trace_bounce_abi import PLANES
from test_trace_skin_abi import BOTH, EMIT_ONLY, HEADER, INVALID, RESOLVE_ONLY, ROOT, World, trace_lib  # noqa: F401

ARITY = dict(rls_trace_skin_bounce_emit=12, rls_trace_skin_bounce_resolve=14)
EMIT_FAMILIES = ("skin_bounce_shadow_emit_kernel", "skin_bounce_sheen_glossy_emit_kernel", "skin_bounce_specular_glossy_emit_kernel",
                 "skin_diffuse_emit_kernel")
OTHER_KERNELS = ("skin_bounce_probe_emit_kernel", "skin_bounce_resolve_kernel")


def _members(c_name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), HEADER.read_text(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.findall(r"\w+", part)[-1] for d in body.split(";") if d.strip() for part in d.split(",")]


def test_declared_exported_and_bound_with_matching_arity(trace_lib):
    from rlshaders_amd import trace
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"rls_status\s+(rls_trace_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}
    out = subprocess.run(["nm", "-D", "--defined-only", str(trace_lib)], capture_output=True, text=True, check=True).stdout
    lib = trace.load()
    for name, arity in ARITY.items():
        assert name in decl, name
        assert len(decl[name].split(",")) == arity, (name, decl[name])
        assert f" T {name}\n" in out, name
        restype, argtypes = trace.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == arity, name
        assert getattr(lib, name).argtypes == argtypes
    assert callable(trace.skin_bounce_rays) and issubclass(trace.SkinBounceQueues, trace.SkinNodeQueues)
    for cls, c_name in ((trace.SkinBounceQueues_, "rls_skin_bounce_queues"), (trace.SkinBounceTraced_, "rls_skin_bounce_traced")):
        assert _members(c_name) == [f[0] for f in cls._fields_], c_name
    # the node's structs are embedded whole, first: a bounce struct's address is its node struct's
    assert trace.SkinBounceQueues_.node.offset == 0 and trace.SkinBounceQueues_._fields_[0][1] is trace.SkinNodeQueues_
    assert trace.SkinBounceTraced_.node.offset == 0 and trace.SkinBounceTraced_._fields_[0][1] is trace.SkinNodeTraced_
    assert C.sizeof(trace.SkinBounceQueues_) == C.sizeof(trace.SkinNodeQueues_) + C.sizeof(C.c_void_p)
    assert C.sizeof(trace.SkinBounceTraced_) == C.sizeof(trace.SkinNodeTraced_) + 3 * C.sizeof(C.c_void_p)
    # the derived seed's constant is the header's
    value = re.search(r"#define RLS_SKIN_DIFFUSE_SEED (0x[0-9A-Fa-f]+)u", HEADER.read_text()).group(1)
    assert trace.RLS_SKIN_DIFFUSE_SEED == int(value, 16)
    # the header no longer lists rlSkin as not covered, and says what stays a per-call flag
    assert "Not covered: rlSkin" not in HEADER.read_text()
    assert "trace_diffuse" in HEADER.read_text().split("Not covered:")[1].split("*/")[0]


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_trace.h"\n'
                   'int main(void){ rls_skin_bounce_queues q; rls_skin_bounce_traced t; rls_skin_integrate_out o; rls_ray_state s;\n'
                   '  rls_gi_depths g = { 8, 2, 2, 4 }; rls_cvec3 P = { 0, 0, 0 }; unsigned seed = 7u ^ RLS_SKIN_DIFFUSE_SEED;\n'
                   '  q.diffuse_shadow = 0; q.node.probes = 0; t.node.hits = 0; t.diffuse_visibility.r = 0; s.Rr = 0; (void)o;\n'
                   '  return rls_trace_skin_bounce_emit(0, 0, 0, P, 0, 0, 1, seed, 0, &s, &g, &q) +\n'
                   '         rls_trace_skin_bounce_resolve(0, 0, 0, P, 0, 0, 0, 0, 1, &s, &g, &q, &t, &o); }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{ROOT / 'include'}",
                            "-x", "c" if cc == "gcc" else "c++", str(src)], capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)


def test_still_two_code_objects_with_the_skin_bounce_kernels(trace_lib):
    from rlshaders_amd.codeid import DeviceCode, code_objects, fatbin
    assert len(code_objects(fatbin(trace_lib))) == 2             # still the EXACT and the FAST unit
    dc = DeviceCode(trace_lib)
    units = {0: set(), 1: set()}
    for fast in (0, 1):
        for fam in EMIT_FAMILIES:
            for g in (1, 4, 16, 64):
                u = dc.unit_of_kernel(f"{fam}<{g}, {fast}>")
                assert u is not None, (fam, g, fast)
                units[fast].add(u)
        for k in OTHER_KERNELS:                                  # per math mode, like their parents
            u = dc.unit_of_kernel(f"{k}<{fast}>")
            assert u is not None, (k, fast)
            units[fast].add(u)
    assert len(units[0]) == 1 and len(units[1]) == 1 and units[0] != units[1]
    # the parents keep their names beside them, and the sixth queue is compacted by the hit list's kernel
    for k in ("skin_shadow_emit_kernel<4, 0>", "skin_sheen_glossy_emit_kernel<1, 1>", "skin_specular_glossy_emit_kernel<64, 0>",
              "skin_probe_emit_kernel<0>", "skin_node_resolve_kernel<1>", "sss_hits_emit_kernel<16, 0>", "hits_compact_kernel"):
        assert dc.unit_of_kernel(k) is not None, k


def test_no_skin_bounce_kernel_in_the_product_library(trace_lib):
    from rlshaders_amd import build
    from rlshaders_amd.codeid import code_objects, fatbin
    for elf in code_objects(fatbin(build.build_library())):
        for fam in EMIT_FAMILIES + OTHER_KERNELS:
            assert fam.encode() not in elf, fam


class BounceWorld(World):
    """World with the state planes, the depths, the sixth queue and its visibility"""

    def __init__(self):
        super().__init__()
        capi, trace = self.capi, self.trace
        p = C.addressof(self.mem)
        self.state = trace.RayState_(p, p, p, p, p)
        self.depths = trace.GiDepths_(8, 2, 2, 4)
        self.sp, self.dp = C.byref(self.state), C.byref(self.depths)
        d = trace.ShadowQueue_()
        d.capacity, d.offsets, d.dir, d.maxdist = self.n * self.nl * 2 * 4, p, capi.Vec3(p, p, p), p
        d.weight_diffuse, d.kind = capi.Rgb(p, None, None), p    # (weight_specular stays NULL)
        d.scratch, d.scratch_bytes = p, self.shadows[0].scratch_bytes
        self.diffuse = d
        self.node_q = self.q
        self.q = trace.SkinBounceQueues_()
        self.sync()
        self.q.diffuse_shadow = C.pointer(d)
        self.node_t = self.t
        self.t = trace.SkinBounceTraced_()
        self.t.diffuse_visibility = capi.CRgb(p, p, p)
        self.qp, self.tp = C.byref(self.q), C.byref(self.t)

    def sync(self):
        """the node structs the tables edit, copied into the bounce structs"""
        for name, _ in self.trace.SkinNodeQueues_._fields_:
            setattr(self.q.node, name, getattr(self.node_q, name))
        if isinstance(self.t, self.trace.SkinBounceTraced_):
            for name, _ in self.trace.SkinNodeTraced_._fields_:
                setattr(self.t.node, name, getattr(self.node_t, name))

    def emit(self):
        self.sync()
        return self.lib.rls_trace_skin_bounce_emit(self.ctxp, self.n, self._c(), self.P, self.lights, self.nl, self.spp_n, 7, 0,
                                                   self.sp, self.dp, self.qp)

    def resolve(self):
        self.sync()
        return self.lib.rls_trace_skin_bounce_resolve(self.ctxp, self.n, self._c(), self.P, self.lights, self.nl, 0, 0, self.spp_n,
                                                      self.sp, self.dp, self.qp, self.tp, self.op)


class _Edit:
    """the node tables' edits address w.q / w.t: here the node structs"""

    def __init__(self, w):
        object.__setattr__(self, "_w", w)

    def __getattr__(self, name):
        w = self._w
        return w.node_q if name == "q" else w.node_t if name == "t" else getattr(w, name)

    def __setattr__(self, name, value):
        setattr(self._w, name, value)


STATE = [("state NULL", lambda w: setattr(w, "sp", None), "state is NULL"),
         ("depths NULL", lambda w: setattr(w, "dp", None), "depths is NULL")] + \
        [(f"state.{name} NULL", (lambda name: lambda w: setattr(w.state, name, None))(name), PLANES)
         for name in ("ray_type", "Rr", "Rr_diff", "Rr_gloss", "Rr_refr")]
SIXTH = [
    ("diffuse_shadow NULL with lights", lambda w: setattr(w._w.q, "diffuse_shadow", None),
     "queues.diffuse_shadow is NULL but n_lights > 0"),
    ("diffuse_shadow offsets NULL", lambda w: setattr(w.diffuse, "offsets", None), "queue.offsets is NULL"),
    ("diffuse_shadow dir NULL", lambda w: setattr(w.diffuse, "dir", w.capi.Vec3(None, None, None)),
     "queue.dir or queue.maxdist plane is NULL"),
    ("diffuse_shadow weight NULL", lambda w: setattr(w.diffuse, "weight_diffuse", w.capi.Rgb(None, None, None)),
     "queue.weight_specular or queue.weight_diffuse plane is NULL"),
    ("diffuse_shadow kind NULL", lambda w: setattr(w.diffuse, "kind", None), "queue.kind is NULL"),
    ("diffuse_shadow capacity short", lambda w: setattr(w.diffuse, "capacity", w.diffuse.capacity - 1),
     "queue.capacity < n * n_lights * 2 * spp_n^2"),
]
SIXTH_EMIT = [
    ("diffuse_shadow scratch short", lambda w: setattr(w.diffuse, "scratch_bytes", 16),
     "queue.scratch is NULL or smaller than rls_trace_shadow_scratch_bytes"),
    ("diffuse_shadow scratch NULL", lambda w: setattr(w.diffuse, "scratch", None),
     "queue.scratch is NULL or smaller than rls_trace_shadow_scratch_bytes"),
]
SIXTH_RESOLVE = [
    ("diffuse_visibility NULL", lambda w: setattr(w._w.t, "diffuse_visibility", w.capi.CRgb(None, None, None)),
     "visibility plane is NULL"),
]


def _no_lights_but_sixth(w):
    w.nl = 0
    w.node_q.sheen_shadow = None
    w.node_q.specular_shadow = None


@pytest.mark.parametrize("verb", ["emit", "resolve"])
def test_every_refusal_names_the_entry_point_before_the_context_is_read(trace_lib, verb):
    from rlshaders_amd import _capi as capi
    entry = f"rls_trace_skin_bounce_{verb}"
    table = BOTH + STATE + SIXTH + (EMIT_ONLY + SIXTH_EMIT if verb == "emit" else RESOLVE_ONLY + SIXTH_RESOLVE)
    table = table + [("diffuse_shadow set without lights", lambda w: _no_lights_but_sixth(w._w),
                      "queues.diffuse_shadow is set but n_lights is 0")]
    wrong = []
    for what, breakit, text in table:
        w = BounceWorld()
        breakit(_Edit(w))
        st = getattr(w, verb)()
        msg = capi.load().rls_last_error().decode()
        if not (st == INVALID and msg == f"{entry}: {text}"):
            wrong.append(f'{entry} / {what}: status {st} "{msg}", want "{text}"')
    assert not wrong, "\n".join(wrong)


def test_a_resolve_of_nothing_succeeds_without_a_device(trace_lib):
    w = BounceWorld()
    w.n = 0
    w.state = type(w.state)()                                    # an empty batch reads no plane
    w.sp = C.byref(w.state)
    assert w.resolve() == 0
    w.sp = None
    assert w.resolve() == INVALID


def test_an_emit_refused_at_the_sixth_queue_launches_nothing(trace_lib):
    """valid but for the last-checked argument of the queue that is filled last: every check runs ahead of the first launch"""
    from rlshaders_amd import _capi as capi
    w = BounceWorld()
    w.diffuse.scratch_bytes = 16
    assert w.emit() == INVALID
    assert capi.load().rls_last_error().decode() == \
        "rls_trace_skin_bounce_emit: queue.scratch is NULL or smaller than rls_trace_shadow_scratch_bytes"
