"""CPU: the caller-traced rlSkin node in the companion library (rls_trace_skin_emit / rls_trace_skin_resolve;
include/rlshaders_amd_trace.h, librls_trace.so).

Both symbols are declared, exported and bound with matching arity (10 and 12) and the binding structs have the header's members
in its order; the header compiles as C99 and C++14; the library still holds two code objects, each with the node's emit kernels
at every lane-group width, the FAST one with no copy of a mode-free kernel; no new kernel name appears in the product
library; and every argument check returns
RLS_ERR_INVALID_ARGUMENT with the entry point's name in the message.  The checks run through ctypes with dummy planes and a dummy
context: a refused call returns before the context is read or anything is launched, so no device is needed."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "rlshaders_amd_trace.h"
ARITY = dict(rls_trace_skin_emit=10, rls_trace_skin_resolve=12)
EMIT_FAMILIES = ("skin_shadow_emit_kernel", "skin_sheen_glossy_emit_kernel", "skin_specular_glossy_emit_kernel")
OTHER_KERNELS = ("skin_probe_emit_kernel", "skin_node_resolve_kernel")
INVALID = 1


@pytest.fixture(scope="module")
def trace_lib():
    from rlshaders_amd import build
    return build.build_trace_library()


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
    assert callable(trace.skin_node_rays) and issubclass(trace.SkinNodeQueues, trace._NodeQueues)
    for cls, c_name in ((trace.SkinNodeQueues_, "rls_skin_node_queues"), (trace.SkinNodeTraced_, "rls_skin_node_traced")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), HEADER.read_text(), flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        members = [re.findall(r"\w+", part)[-1] for d in body.split(";") if d.strip() for part in d.split(",")]
        assert members == [f[0] for f in cls._fields_], (c_name, members)


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_trace.h"\n'
                   'int main(void){ rls_skin_node_queues q = {0}; rls_skin_node_traced t; rls_skin_integrate_out o; rls_cvec3 P = {0};\n'
                   '  (void)t; (void)o;\n'
                   '  return rls_trace_skin_emit(0, 0, 0, P, 0, 0, 1, 7u, 0, &q) +\n'
                   '         rls_trace_skin_resolve(0, 0, 0, P, 0, 0, 0, 0, 1, &q, 0, 0); }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{ROOT / 'include'}",
                            "-x", "c" if cc == "gcc" else "c++", str(src)], capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)


def test_two_code_objects_with_the_skin_kernels(trace_lib):
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
        # the probe emit and the one resolve follow the context's math mode (the scatter walk's profile and MIS arithmetic)
        for k in OTHER_KERNELS:
            u = dc.unit_of_kernel(f"{k}<{fast}>")
            assert u is not None, (k, fast)
            units[fast].add(u)
    assert len(units[0]) == 1 and len(units[1]) == 1 and units[0] != units[1]
    # the kernels the node reuses keep their names; the lobes' shadow queues are compacted without diffuse planes
    for k in ("sss_probe_emit_kernel<0>", "sss_scatter_resolve_kernel<1>", "shadow_compact_kernel<0>", "shadow_compact_kernel<1>",
              "shadow_compact_kernel<3>", "trace_compact_kernel<3>", "ggx_node_resolve_kernel"):
        assert dc.unit_of_kernel(k) is not None, k


def test_the_fast_unit_holds_no_copy_of_a_mode_free_kernel(trace_lib):
    """the scan, compaction and resolve kernels are templates (or guarded) and are launched from the EXACT unit's host code
    alone: the FAST code object must not instantiate any of them"""
    from rlshaders_amd.codeid import code_objects, fatbin
    fast = [elf for elf in code_objects(fatbin(trace_lib)) if b"skin_shadow_emit_kernelILi1ELi1EE" in elf]
    assert len(fast) == 1
    for name in (b"trace_scan_block_kernel", b"trace_scan_totals_kernel", b"trace_scan_add_kernel", b"trace_compact_kernel",
                 b"shadow_compact_kernel", b"trace_resolve_kernel", b"shadow_resolve_kernel", b"ggx_node_resolve_kernel",
                 b"disney_node_resolve_kernel", b"ggx_node_compose_kernel", b"disney_node_compose_kernel"):
        assert name not in fast[0], name


def test_no_skin_node_kernel_in_the_product_library(trace_lib):
    from rlshaders_amd import build
    from rlshaders_amd.codeid import code_objects, fatbin
    for elf in code_objects(fatbin(build.build_library())):
        for fam in EMIT_FAMILIES + OTHER_KERNELS:
            assert fam.encode() not in elf, fam


# ---- argument checks, no device ------------------------------------------------------------------------------------------------
class World:
    """a valid argument set over dummy planes (never read: every case below is refused before a launch)"""

    def __init__(self):
        from rlshaders_amd import _capi as capi, trace
        self.capi, self.trace = capi, trace
        self.lib = trace.load()
        self.ctx = C.create_string_buffer(4096)                  # non-NULL; a refused call does not read it
        self.mem = C.create_string_buffer(1 << 16)
        p = C.addressof(self.mem)
        self.n, self.spp_n, self.nl = 8, 2, 2
        v3 = lambda cls: cls(p, p, p)
        self.c = capi.SkinClosure()
        self.c.wo, self.c.N, self.c.T = v3(capi.CVec3), v3(capi.CVec3), v3(capi.CVec3)
        self.P = v3(capi.CVec3)
        self.lights = (capi.SphereLight * 2)()
        for l in self.lights:
            l.radius = 1.0
        sb, rb = C.c_size_t(), C.c_size_t()
        assert self.lib.rls_trace_shadow_scratch_bytes(self.n, self.nl, self.spp_n, C.byref(sb)) == 0
        assert self.lib.rls_trace_scratch_bytes(self.n, self.spp_n, C.byref(rb)) == 0
        self.shadows, self.rays = [], []
        for _ in range(2):
            s = trace.ShadowQueue_()
            s.capacity, s.offsets, s.dir, s.maxdist = self.n * self.nl * 2 * 4, p, v3(capi.Vec3), p
            s.weight_specular, s.kind = v3(capi.Rgb), p        # (weight_diffuse stays NULL)
            s.scratch, s.scratch_bytes = p, sb.value
            self.shadows.append(s)
            q = trace.RayQueue_()
            q.capacity, q.offsets, q.dir, q.weight = self.n * 4, p, v3(capi.Vec3), v3(capi.Rgb)
            q.scratch, q.scratch_bytes = p, rb.value
            self.rays.append(q)
        pq = trace.ProbeQueue_()
        pq.capacity, pq.offsets, pq.origin, pq.dir, pq.maxdist = self.n * 4, p, v3(capi.Vec3), v3(capi.Vec3), p
        self.probes = pq
        q = trace.SkinNodeQueues_()
        q.sheen_shadow, q.specular_shadow = C.pointer(self.shadows[0]), C.pointer(self.shadows[1])
        q.sheen_glossy, q.specular_glossy = C.pointer(self.rays[0]), C.pointer(self.rays[1])
        q.probes = C.pointer(pq)
        q.sheenFresnel = q.specularFresnel = q.sssWeight = p
        self.q = q
        h = trace.ProbeHits_()
        h.max_hits, h.stride, h.count, h.P, h.N, h.irradiance = 2, self.n * 4, p, v3(capi.CVec3), v3(capi.CVec3), v3(capi.CRgb)
        self.hits = h
        t = trace.SkinNodeTraced_()
        for name in ("sheen_visibility", "specular_visibility", "sheen_glossy", "specular_glossy"):
            setattr(t, name, v3(capi.CRgb))
        t.hits = C.pointer(h)
        self.t = t
        self.out = capi.SkinIntegrateOut()
        for name in ("sheen", "specular", "sss", "out"):
            setattr(self.out, name, v3(capi.Rgb))
        self.qp, self.tp, self.op, self.ctxp = C.byref(self.q), C.byref(self.t), C.byref(self.out), C.addressof(self.ctx)

    def _c(self):
        return C.byref(self.c) if self.c is not None else None

    def emit(self):
        return self.lib.rls_trace_skin_emit(self.ctxp, self.n, self._c(), self.P, self.lights, self.nl, self.spp_n, 7, 0, self.qp)

    def resolve(self):
        return self.lib.rls_trace_skin_resolve(self.ctxp, self.n, self._c(), self.P, self.lights, self.nl, 0, 0, self.spp_n, self.qp,
                                               self.tp, self.op)


def _no_lights(w):
    w.nl = 0


BOTH = [
    ("ctx NULL", lambda w: setattr(w, "ctxp", None), "ctx is NULL"),
    ("n < 0", lambda w: setattr(w, "n", -1), "n < 0"),
    ("spp_n 0", lambda w: setattr(w, "spp_n", 0), "spp_n must be in [1, 16]"),
    ("spp_n 17", lambda w: setattr(w, "spp_n", 17), "spp_n must be in [1, 16]"),
    ("queues NULL", lambda w: setattr(w, "qp", None), "queues is NULL"),
    ("n_lights 9", lambda w: setattr(w, "nl", 9), "n_lights out of range (RLS_MAX_LIGHTS)"),
    ("n_lights -1", lambda w: setattr(w, "nl", -1), "n_lights out of range (RLS_MAX_LIGHTS)"),
    ("lights NULL", lambda w: setattr(w, "lights", None), "lights is NULL"),
    ("one shadow NULL with lights", lambda w: setattr(w.q, "specular_shadow", None),
     "queues.sheen_shadow or queues.specular_shadow is NULL but n_lights > 0"),
    ("shadows set without lights", _no_lights, "queues.sheen_shadow or queues.specular_shadow is set but n_lights is 0"),
    ("a glossy queue NULL", lambda w: setattr(w.q, "specular_glossy", None),
     "queues.sheen_glossy, queues.specular_glossy or queues.probes is NULL"),
    ("probes NULL", lambda w: setattr(w.q, "probes", None), "queues.sheen_glossy, queues.specular_glossy or queues.probes is NULL"),
    ("a scalar plane NULL", lambda w: setattr(w.q, "sssWeight", None),
     "queues.sheenFresnel, queues.specularFresnel or queues.sssWeight is NULL"),
    ("offsets NULL", lambda w: setattr(w.rays[0], "offsets", None), "queue.offsets is NULL"),
    ("closure NULL", lambda w: setattr(w, "c", None), "closure is NULL"),
    ("P NULL", lambda w: setattr(w, "P", w.capi.CVec3(None, None, None)), "wo/N/T/P plane is NULL"),
    ("shadow capacity short", lambda w: setattr(w.shadows[1], "capacity", w.shadows[1].capacity - 1),
     "queue.capacity < n * n_lights * 2 * spp_n^2"),
    ("shadow weight NULL", lambda w: setattr(w.shadows[0], "weight_specular", w.capi.Rgb(None, None, None)),
     "queue.weight_specular plane is NULL"),
    ("ray capacity short", lambda w: setattr(w.rays[1], "capacity", w.rays[1].capacity - 1), "queue.capacity < n * spp_n^2"),
    ("probe capacity short", lambda w: setattr(w.probes, "capacity", w.probes.capacity - 1), "queue.capacity < n * spp_n^2"),
]
EMIT_ONLY = [
    ("ray scratch short", lambda w: setattr(w.rays[1], "scratch_bytes", 16), "queue.scratch is NULL or smaller than rls_trace_scratch_bytes"),
    ("ray scratch NULL", lambda w: setattr(w.rays[0], "scratch", None), "queue.scratch is NULL or smaller than rls_trace_scratch_bytes"),
    ("shadow scratch short", lambda w: setattr(w.shadows[0], "scratch_bytes", 16),
     "queue.scratch is NULL or smaller than rls_trace_shadow_scratch_bytes"),
    ("shadow scratch NULL", lambda w: setattr(w.shadows[1], "scratch", None),
     "queue.scratch is NULL or smaller than rls_trace_shadow_scratch_bytes"),
    ("ray dir NULL", lambda w: setattr(w.rays[0], "dir", w.capi.Vec3(None, None, None)), "queue.dir plane is NULL"),
    ("probe maxdist NULL", lambda w: setattr(w.probes, "maxdist", None), "queue.origin, queue.dir or queue.maxdist plane is NULL"),
]
RESOLVE_ONLY = [
    ("traced NULL", lambda w: setattr(w, "tp", None), "traced or out is NULL"),
    ("out NULL", lambda w: setattr(w, "op", None), "traced or out is NULL"),
    ("hits NULL", lambda w: setattr(w.t, "hits", None), "traced.hits is NULL"),
    ("max_hits 0", lambda w: setattr(w.hits, "max_hits", 0), "hits.max_hits must be in [1, 12]"),
    ("max_hits 13", lambda w: setattr(w.hits, "max_hits", 13), "hits.max_hits must be in [1, 12]"),
    ("stride short", lambda w: setattr(w.hits, "stride", w.n * 4 - 1), "hits.stride < n * spp_n^2"),
    ("a hit plane NULL", lambda w: setattr(w.hits, "count", None), "hits.count, hits.P, hits.N or hits.irradiance plane is NULL"),
    ("an AOV plane NULL", lambda w: setattr(w.out, "sss", w.capi.Rgb(None, None, None)), "NULL AOV plane"),
    ("out.out partly set", lambda w: setattr(w.out, "out", w.capi.Rgb(C.addressof(w.mem), None, None)),
     "out planes must be all set or all NULL"),
    ("visibility NULL", lambda w: setattr(w.t, "specular_visibility", w.capi.CRgb(None, None, None)), "visibility plane is NULL"),
    ("radiance NULL", lambda w: setattr(w.t, "sheen_glossy", w.capi.CRgb(None, None, None)), "radiance plane is NULL"),
    ("ray weight NULL", lambda w: setattr(w.rays[0], "weight", w.capi.Rgb(None, None, None)), "queue.weight plane is NULL"),
]


@pytest.mark.parametrize("verb", ["emit", "resolve"])
def test_argument_checks_name_the_entry_point(trace_lib, verb):
    from rlshaders_amd import _capi as capi
    entry = f"rls_trace_skin_{verb}"
    wrong = []
    for what, breakit, text in BOTH + (EMIT_ONLY if verb == "emit" else RESOLVE_ONLY):
        w = World()
        breakit(w)
        st = getattr(w, verb)()
        msg = capi.load().rls_last_error().decode()
        if not (st == INVALID and msg == f"{entry}: {text}"):
            wrong.append(f'{entry} / {what}: status {st} "{msg}", want "{text}"')
    assert not wrong, "\n".join(wrong)


def test_a_resolve_of_nothing_succeeds_without_a_device(trace_lib):
    w = World()
    w.n = 0
    assert w.resolve() == 0
    w.spp_n = 17
    assert w.resolve() == INVALID


@pytest.mark.parametrize("node", ["skin"])
def test_an_emit_refused_at_its_last_shadow_queue_launches_nothing(trace_lib, node):
    """A valid call but for the last-checked argument of the last queue, the second lobe's shadow scratch too small (World
    sizes it with rls_trace_shadow_scratch_bytes, more than a lobe's two-segment loop needs: hence 16 bytes, not one byte less):
    every check of the node emit runs ahead of its first launch, so the call is refused with the entry point's name before the
    (dummy) context is read -- the first lobe's emits, earlier in stream order, included."""
    from rlshaders_amd import _capi as capi
    w = World()
    w.shadows[1].scratch_bytes = 16
    assert w.emit() == INVALID
    assert capi.load().rls_last_error().decode() == \
        f"rls_trace_{node}_emit: queue.scratch is NULL or smaller than rls_trace_shadow_scratch_bytes"
