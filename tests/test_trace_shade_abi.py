"""CPU: the caller-traced whole nodes in the companion library (rls_trace_ggx_shade_emit / _resolve,
rls_trace_disney_shade_emit / _resolve; include/rlshaders_amd_trace.h, librls_trace.so).

The four symbols are declared, exported and bound with matching arity; the header with the node structs compiles as C99 and
C++14; the library still holds two code objects, each with the node's emit kernels at every lane-group width, the EXACT one
with the two node resolve kernels; and every argument check returns RLS_ERR_INVALID_ARGUMENT with the entry point's name in
the message.  The checks run through ctypes with dummy planes and a dummy context: a refused call returns before the context
is read or anything is launched, so no device is needed."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "rlshaders_amd_trace.h"
NODE_SYMBOLS = ("rls_trace_ggx_shade_emit", "rls_trace_ggx_shade_resolve", "rls_trace_disney_shade_emit",
                "rls_trace_disney_shade_resolve")
ARITY = dict(rls_trace_ggx_shade_emit=12, rls_trace_ggx_shade_resolve=11, rls_trace_disney_shade_emit=10,
             rls_trace_disney_shade_resolve=8)
EMIT_FAMILIES = ("ggx_node_glossy_emit_kernel", "ggx_node_refract_emit_kernel", "ggx_node_diffuse_emit_kernel",
                 "disney_node_diffuse_emit_kernel", "disney_node_specular_emit_kernel")
INVALID = 1


@pytest.fixture(scope="module")
def trace_lib():
    from rlshaders_amd import build
    return build.build_trace_library()


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"rls_status\s+(rls_trace_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_declared_exported_and_bound_with_matching_arity(trace_lib):
    from rlshaders_amd import trace
    decl = _declarations()
    out = subprocess.run(["nm", "-D", "--defined-only", str(trace_lib)], capture_output=True, text=True, check=True).stdout
    lib = trace.load()
    for name in NODE_SYMBOLS:
        assert name in decl, name
        assert len(decl[name].split(",")) == ARITY[name], (name, decl[name])
        assert f" T {name}\n" in out, name
        restype, argtypes = trace.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == ARITY[name], name
        assert getattr(lib, name).argtypes == argtypes
    assert callable(trace.ggx_node_rays) and callable(trace.disney_node_rays)
    # the binding structs have the header's members, in its order
    text = HEADER.read_text()
    for cls, c_name in ((trace.GgxNodeQueues_, "rls_ggx_node_queues"), (trace.GgxNodeTraced_, "rls_ggx_node_traced"),
                        (trace.DisneyNodeQueues_, "rls_disney_node_queues"), (trace.DisneyNodeTraced_, "rls_disney_node_traced")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = [re.findall(r"\w+", part)[-1] for d in body.split(";") if d.strip() for part in d.split(",")]
        assert members == [f[0] for f in cls._fields_], (c_name, members)
    # ggx_shader carries KtColor and Kt, and today's callers are unchanged
    import inspect
    sig = inspect.signature(trace.ggx_shader)
    assert list(sig.parameters)[:5] == ["sampler", "KdColor", "Kd", "diffuseRoughness", "Ks"]
    assert sig.parameters["KtColor"].default == (1.0, 1.0, 1.0) and sig.parameters["Kt"].default == 0.0


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_trace.h"\n'
                   'int main(void){ rls_ggx_node_queues q = {0}; rls_ggx_node_traced t; rls_disney_node_queues d = {0};\n'
                   '  rls_disney_node_traced u; rls_ggx_shade_out o; rls_disney_shade_out p; (void)t; (void)u; (void)o; (void)p;\n'
                   '  return rls_trace_ggx_shade_resolve(0, 0, 0, 0, 0, 0, 1, 1, &q, 0, 0) +\n'
                   '         rls_trace_disney_shade_resolve(0, 0, 0, 0, 1, &d, 0, 0); }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{ROOT / 'include'}",
                            "-x", "c" if cc == "gcc" else "c++", str(src)], capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)


def test_two_code_objects_with_the_node_kernels(trace_lib):
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
    assert len(units[0]) == 1 and len(units[1]) == 1 and units[0] != units[1]
    # the resolves are mode-free (+ and x only): in the EXACT unit, like trace_resolve_kernel and shadow_resolve_kernel
    for k in ("ggx_node_resolve_kernel", "disney_node_resolve_kernel"):
        assert dc.unit_of_kernel(k) in units[0], k
    # the kernels the node verbs reuse keep their names
    for k in ("ggx_glossy_emit_kernel<1, 0>", "disney_specular_emit_kernel<64, 1>", "ggx_direct_emit_kernel<4, 0>",
              "trace_resolve_kernel<3>", "trace_resolve_kernel<1>", "shadow_resolve_kernel<1>", "shadow_resolve_kernel<3>"):
        assert dc.unit_of_kernel(k) is not None, k


def test_no_node_kernel_in_the_product_library(trace_lib):
    from rlshaders_amd import build
    from rlshaders_amd.codeid import code_objects, fatbin
    for elf in code_objects(fatbin(build.build_library())):
        for fam in EMIT_FAMILIES + ("ggx_node_resolve_kernel", "disney_node_resolve_kernel"):
            assert fam.encode() not in elf, fam


# ---- argument checks, no device ------------------------------------------------------------------------------------------------
class World:
    """a valid argument set over dummy planes (never read: every case below is refused before a launch)"""

    def __init__(self, node):
        from rlshaders_amd import _capi as capi, trace
        self.node, self.capi, self.trace = node, capi, trace
        self.lib = trace.load()
        self.ctx = C.create_string_buffer(4096)                  # non-NULL; a refused call does not read it
        self.mem = C.create_string_buffer(1 << 16)
        p = C.addressof(self.mem)
        self.n, self.spp_n, self.nl = 8, 2, 2
        v3 = lambda cls: cls(p, p, p)
        if node == "ggx":
            self.c = capi.GgxClosure()
            self.sh = capi.GgxShader()
        else:
            self.c = capi.DisneyClosure()
        self.c.wo, self.c.N, self.c.T = v3(capi.CVec3), v3(capi.CVec3), v3(capi.CVec3)
        self.P = v3(capi.CVec3)
        self.lights = (capi.SphereLight * 2)()
        for l in self.lights:
            l.radius = 1.0
        sb, rb = C.c_size_t(), C.c_size_t()
        assert self.lib.rls_trace_shadow_scratch_bytes(self.n, self.nl, self.spp_n, C.byref(sb)) == 0
        assert self.lib.rls_trace_scratch_bytes(self.n, self.spp_n, C.byref(rb)) == 0
        s = trace.ShadowQueue_()
        s.capacity, s.offsets, s.dir, s.maxdist = self.n * self.nl * 3 * 4, p, v3(capi.Vec3), p
        s.weight_specular, s.weight_diffuse, s.kind = v3(capi.Rgb), v3(capi.Rgb), p
        s.scratch, s.scratch_bytes = p, sb.value
        self.shadow = s
        self.rays = []
        for _ in range(3 if node == "ggx" else 2):
            q = trace.RayQueue_()
            q.capacity, q.offsets, q.dir, q.weight = self.n * 4, p, v3(capi.Vec3), v3(capi.Rgb)
            q.scratch, q.scratch_bytes = p, rb.value
            self.rays.append(q)
        self.q = (trace.GgxNodeQueues_ if node == "ggx" else trace.DisneyNodeQueues_)()
        self.q.shadow = C.pointer(self.shadow)
        for (name, _), r in zip(self.q._fields_[1:], self.rays):
            setattr(self.q, name, C.pointer(r))
        self.t = (trace.GgxNodeTraced_ if node == "ggx" else trace.DisneyNodeTraced_)()
        for name, _ in self.t._fields_:
            setattr(self.t, name, v3(capi.CRgb))
        self.out = (capi.GgxShadeOut if node == "ggx" else capi.DisneyShadeOut)()
        for name, _ in self.out._fields_:
            setattr(self.out, name, v3(capi.Rgb))
        self.qp, self.tp, self.op, self.ctxp = C.byref(self.q), C.byref(self.t), C.byref(self.out), C.addressof(self.ctx)

    def _c(self):
        return C.byref(self.c) if self.c is not None else None

    def emit(self):
        if self.node == "ggx":
            return self.lib.rls_trace_ggx_shade_emit(self.ctxp, self.n, self._c(), C.byref(self.sh), self.P, self.lights,
                                                     self.nl, 1, self.spp_n, 7, 0, self.qp)
        return self.lib.rls_trace_disney_shade_emit(self.ctxp, self.n, self._c(), self.P, self.lights, self.nl, self.spp_n,
                                                    7, 0, self.qp)

    def resolve(self):
        if self.node == "ggx":
            return self.lib.rls_trace_ggx_shade_resolve(self.ctxp, self.n, self._c(), C.byref(self.sh), self.lights, self.nl,
                                                        1, self.spp_n, self.qp, self.tp, self.op)
        return self.lib.rls_trace_disney_shade_resolve(self.ctxp, self.n, self.lights, self.nl, self.spp_n, self.qp, self.tp,
                                                       self.op)


def _null_shadow(w):
    w.q.shadow = None


def _no_lights(w):
    w.nl = 0


def _last_ray(w):
    return w.rays[-1]


BOTH = [
    ("ctx NULL", lambda w: setattr(w, "ctxp", None), "ctx is NULL"),
    ("n < 0", lambda w: setattr(w, "n", -1), "n < 0"),
    ("spp_n 0", lambda w: setattr(w, "spp_n", 0), "spp_n must be in [1, 16]"),
    ("spp_n 17", lambda w: setattr(w, "spp_n", 17), "spp_n must be in [1, 16]"),
    ("queues NULL", lambda w: setattr(w, "qp", None), "queues is NULL"),
    ("n_lights 9", lambda w: setattr(w, "nl", 9), "n_lights out of range (RLS_MAX_LIGHTS)"),
    ("n_lights -1", lambda w: setattr(w, "nl", -1), "n_lights out of range (RLS_MAX_LIGHTS)"),
    ("shadow NULL with lights", _null_shadow, "queues.shadow is NULL but n_lights > 0"),
    ("shadow set without lights", _no_lights, "queues.shadow is set but n_lights is 0"),
    ("a ray queue NULL", lambda w: setattr(w.q, w.q._fields_[-1][0], None), None),
    ("shadow capacity short", lambda w: setattr(w.shadow, "capacity", w.shadow.capacity - 1),
     "queue.capacity < n * n_lights * 3 * spp_n^2"),
    ("ray capacity short", lambda w: setattr(_last_ray(w), "capacity", _last_ray(w).capacity - 1), "queue.capacity < n * spp_n^2"),
    ("lights NULL", lambda w: setattr(w, "lights", None), None),
]
EMIT_ONLY = [
    ("ray scratch short", lambda w: setattr(_last_ray(w), "scratch_bytes", _last_ray(w).scratch_bytes - 1),
     "queue.scratch is NULL or smaller than rls_trace_scratch_bytes"),
    ("ray scratch NULL", lambda w: setattr(_last_ray(w), "scratch", None),
     "queue.scratch is NULL or smaller than rls_trace_scratch_bytes"),
    ("shadow scratch short", lambda w: setattr(w.shadow, "scratch_bytes", w.shadow.scratch_bytes - 1),
     "queue.scratch is NULL or smaller than rls_trace_shadow_scratch_bytes"),
    ("ray offsets NULL", lambda w: setattr(w.rays[0], "offsets", None), "queue.offsets is NULL"),
    ("ray dir NULL", lambda w: setattr(w.rays[0], "dir", w.capi.Vec3(None, None, None)), "queue.dir plane is NULL"),
    ("P NULL", lambda w: setattr(w, "P", w.capi.CVec3(None, None, None)), "wo/N/T/P plane is NULL"),
]
RESOLVE_ONLY = [
    ("traced NULL", lambda w: setattr(w, "tp", None), "traced or out is NULL"),
    ("out NULL", lambda w: setattr(w, "op", None), "traced or out is NULL"),
    ("an AOV plane NULL", lambda w: setattr(w.out, "indirect_specular", w.capi.Rgb(None, None, None)), "NULL AOV plane"),
    ("out.out partly set", lambda w: setattr(w.out, "out", w.capi.Rgb(C.addressof(w.mem), None, None)),
     "out planes must be all set or all NULL"),
    ("visibility NULL", lambda w: setattr(w.t, "visibility", w.capi.CRgb(None, None, None)), "visibility plane is NULL"),
    ("radiance NULL", lambda w: setattr(w.t, w.t._fields_[-1][0], w.capi.CRgb(None, None, None)), "radiance plane is NULL"),
    ("ray weight NULL", lambda w: setattr(w.rays[0], "weight", w.capi.Rgb(None, None, None)), "queue.weight plane is NULL"),
]


@pytest.mark.parametrize("verb", ["emit", "resolve"])
@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_argument_checks_name_the_entry_point(trace_lib, node, verb):
    from rlshaders_amd import _capi as capi
    entry = f"rls_trace_{node}_shade_{verb}"
    table = BOTH + (EMIT_ONLY if verb == "emit" else RESOLVE_ONLY)
    if node == "ggx":
        table = table + [("closure NULL", lambda w: setattr(w, "c", None), "closure or shader is NULL")]
    elif verb == "emit":
        table = table + [("closure NULL", lambda w: setattr(w, "c", None), "closure is NULL")]
    wrong = []
    for what, breakit, text in table:
        w = World(node)
        breakit(w)
        st = getattr(w, verb)()
        msg = capi.load().rls_last_error().decode()
        ok = st == INVALID and msg.startswith(entry + ": ") and (text is None or msg == f"{entry}: {text}")
        if what == "lights NULL":                                # copy_lights names itself, as in every light-loop verb
            ok = st == INVALID and msg.endswith("lights is NULL")
        if not ok:
            wrong.append(f'{entry} / {what}: status {st} "{msg}", want "{text}"')
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_a_resolve_of_nothing_succeeds_without_a_device(trace_lib, node):
    """n == 0: the resolve has nothing to write and launches nothing (the emit of n == 0 writes offsets[0] = 0 on the device:
    tests/test_gpu_trace_shade.py)"""
    w = World(node)
    w.n = 0
    assert w.resolve() == 0
    w.spp_n = 17
    assert w.resolve() == INVALID


@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_an_emit_refused_at_its_last_ray_queue_launches_nothing(trace_lib, node):
    """A valid call but for the last-checked argument of the last ray queue, its scratch one byte short: every check of a
    node emit runs ahead of its first launch, so the call is refused with the entry point's name before the (dummy) context
    is read -- the light loop's emit, first in stream order, included."""
    from rlshaders_amd import _capi as capi
    w = World(node)
    _last_ray(w).scratch_bytes -= 1
    assert w.emit() == INVALID
    assert capi.load().rls_last_error().decode() == \
        f"rls_trace_{node}_shade_emit: queue.scratch is NULL or smaller than rls_trace_scratch_bytes"
