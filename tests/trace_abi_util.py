"""helpers of the companion library's CPU tests (test_trace_abi.py, test_trace_{shade,bounce,skin,opacity}_abi.py,
test_cmake_trace.py): what the header include/rlshaders_amd_trace.h declares, what librls_trace.so exports and holds, the two
compiler stanzas, the checks of a set of table rows (tests/trace_abi_tables.py), the refusal runner and the dummy arguments a
refused call is handed.  Each is written here once; pytest does not collect this module."""
import ctypes as C
import re
import subprocess
from functools import lru_cache
from pathlib import Path
from types import SimpleNamespace

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "rlshaders_amd_trace.h"
INVALID = 1                                                      # RLS_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def trace_lib():
    from rlshaders_amd import build
    return build.build_trace_library()


# ---- the header ----------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _without_comments(header):
    return re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)


def code_text(header=HEADER):
    """a header without its comments (read once a session)"""
    return _without_comments(Path(header))


def declared_symbols(*headers):
    return sorted({s for h in headers for s in re.findall(r"\b(rls_[a-z0-9_]+)\s*\(", code_text(h))})


def declared_trace_symbols():
    return declared_symbols(HEADER)


@lru_cache(maxsize=None)
def declarations():
    """entry point -> its parameter list"""
    return {m.group(1): m.group(2)
            for m in re.finditer(r"rls_status\s+(rls_trace_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code_text(), flags=re.S)}


@lru_cache(maxsize=None)
def dynamic_symbols(lib):
    """`nm -D --defined-only`: one "address type name" line per export"""
    return subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout


def exported_trace_symbols(lib):
    return sorted(l.split()[-1] for l in dynamic_symbols(lib).splitlines() if l.split() and l.split()[-1].startswith("rls_"))


def header_structs():
    return re.findall(r"typedef struct (\w+)\s*\{", code_text())


def struct_body(c_name):
    return re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (c_name, c_name), code_text(), flags=re.S).group(1)


def struct_members(c_name):
    """[(member, array length or None)] in the header's order, a declarator at a time; a length spelled as one of the header's
    enum constants is resolved through it"""
    enums = {k: int(v, 0) for k, v in re.findall(r"\b(RLS_[A-Z0-9_]+)\s*=\s*(0x[0-9a-fA-F]+|\d+)", code_text())}
    members = []
    for d in struct_body(c_name).split(";"):
        for part in d.split(",") if d.strip() else []:
            m = re.search(r"(\w+)\s*(?:\[(\w+)\])?\s*$", part.strip())
            length = m.group(2)
            members.append((m.group(1), None if length is None else int(length) if length.isdigit() else enums[length]))
    return members


# ---- the compilers -------------------------------------------------------------------------------------------------------------
def syntax_check(tmp_path, source):
    """one translation unit including the header, as strict C99 and as strict C++14"""
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_trace.h"\n' + source)
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{ROOT / 'include'}",
                            "-x", "c" if cc == "gcc" else "c++", str(src)], capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)


def run_probe(tmp_path, lines):
    """compile main() { lines } as C99 against the header and run it -> its output lines"""
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(['#include <stddef.h>', '#include <stdio.h>', '#include "rlshaders_amd_trace.h"', 'int main(void) {',
                              *lines, '  return 0; }']) + "\n")
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return [l for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if l]


# ---- the device code -----------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def units(trace_lib):
    """the companion's DeviceCode, its ELF images by unit id, and the units of the two math modes (told apart by the first emit
    kernel: EXACT <G, 0>, FAST <G, 1>)"""
    from rlshaders_amd.codeid import DeviceCode, code_objects, fatbin, unit_digest
    dc = DeviceCode(trace_lib)
    objs = code_objects(fatbin(trace_lib))
    return SimpleNamespace(dc=dc, objs=objs, images={unit_digest(e)[0]: e for e in objs},
                           exact=dc.unit_of_kernel("ggx_glossy_emit_kernel<1, 0>"), fast=dc.unit_of_kernel("ggx_glossy_emit_kernel<1, 1>"))


def check_placement(trace_lib, width, mode, free):
    """two gfx950 code objects; every `width` family <G, fast> and `mode` kernel <fast> in its mode's unit; every `free` instance
    in the EXACT unit, its name in one image only and nowhere in the FAST image"""
    u = units(trace_lib)
    assert len(u.objs) == 2 and all(b"gfx950" in elf for elf in u.objs)
    assert u.exact is not None and u.fast is not None and u.exact != u.fast and set(u.images) == {u.exact, u.fast}
    for fast, unit in ((0, u.exact), (1, u.fast)):
        for k in [f"{fam}<{g}, {fast}>" for fam in width for g in (1, 4, 16, 64)] + [f"{k}<{fast}>" for k in mode]:
            assert u.dc.unit_of_kernel(k) == unit, k
    for k in free:
        name = k.split("<")[0].encode()
        assert u.dc.unit_of_kernel(k) == u.exact, k
        assert sum(name in elf for elf in u.objs) == 1 and name not in u.images[u.fast], k


@lru_cache(maxsize=None)
def product_code_objects():
    from rlshaders_amd import build
    from rlshaders_amd.codeid import code_objects, fatbin
    return code_objects(fatbin(build.build_library()))


def check_absent_from_product(kernels):
    """no kernel of these names (template arguments dropped) in any code object of the product library"""
    names = sorted({k.split("<")[0] for k in kernels})
    for elf in product_code_objects():
        for k in names:
            assert k.encode() not in elf, k


# ---- the bindings --------------------------------------------------------------------------------------------------------------
def check_bound(trace_lib, arity):
    """every entry point of `arity` is declared with that many parameters, exported as a ` T ` symbol, and bound in
    trace.PROTOTYPES with as many argtypes, which the loaded function carries, returning int"""
    from rlshaders_amd import trace
    decl, out, lib = declarations(), dynamic_symbols(trace_lib), trace.load()
    for name, n in arity.items():
        assert name in decl, name
        assert len(decl[name].split(",")) == n, (name, decl[name])
        assert f" T {name}\n" in out, name
        restype, argtypes = trace.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == n, name
        assert getattr(lib, name).argtypes == argtypes


@lru_cache(maxsize=None)
def mirrors():
    """the ctypes.Structure classes trace.py defines, by the header struct their docstring names"""
    import inspect
    from rlshaders_amd import trace
    classes = [c for _, c in inspect.getmembers(trace, inspect.isclass) if issubclass(c, C.Structure) and c.__module__ == trace.__name__]
    assert len({c.__doc__ for c in classes}) == len(classes)
    return {c.__doc__: c for c in classes}


def check_members(c_names):
    """the mirror of each struct has the header's members in its order, arrays in length"""
    for c_name in c_names:
        cls = mirrors()[c_name]
        fields = [(f[0], f[1]._length_ if issubclass(f[1], C.Array) else None) for f in cls._fields_]
        assert struct_members(c_name) == fields, (c_name, struct_members(c_name), fields)


def check_callables(names):
    from rlshaders_amd import trace
    assert all(callable(getattr(trace, f)) for f in names), names


# ---- refused calls -------------------------------------------------------------------------------------------------------------
def last_error():
    from rlshaders_amd import _capi as capi
    return capi.load().rls_last_error().decode()


def refusals(make_world, call, entry, table):
    """Every row (what, edit, text) on a fresh world: edit(world), call(world) must return RLS_ERR_INVALID_ARGUMENT and leave
    "<entry>: <text>" in rls_last_error(); a text of None asks for the "<entry>: " prefix alone.  Returns the rows that differ."""
    wrong = []
    for what, edit, text in table:
        w = make_world()
        edit(w)
        st, msg = call(w), last_error()
        ok = st == INVALID and msg.startswith(entry + ": ") and (text is None or msg == f"{entry}: {text}")
        if what == "lights NULL" and text is None:               # copy_lights names itself, as in every light-loop verb
            ok = st == INVALID and msg.endswith("lights is NULL")
        if not ok:
            wrong.append(f'{entry} / {what}: status {st} "{msg}", want "{text}"')
    return wrong


class Dummies:
    """Valid arguments over dummy memory, for calls that return before a launch: a 4 KiB context and a 64 KiB block every plane
    points into (neither is read), n = 8 points at spp_n = 2 under 2 lights, and builders of the queue and state structs, each
    scratch sized by the library's own *_scratch_bytes call."""

    def __init__(self):
        from rlshaders_amd import _capi as capi, trace
        self.capi, self.trace, self.lib = capi, trace, trace.load()
        self.ctx = C.create_string_buffer(4096)                  # non-NULL; a refused call does not read it
        self.mem = C.create_string_buffer(1 << 16)
        self.p, self.ctxp = C.addressof(self.mem), C.addressof(self.ctx)
        self.n, self.spp_n, self.nl = 8, 2, 2

    def v3(self, cls):
        return cls(self.p, self.p, self.p)

    def none3(self, cls):
        return cls(None, None, None)

    def half3(self, cls):
        return cls(self.p, None, self.p)

    def _scratch(self, fn, *args):
        b = C.c_size_t()
        assert fn(*args, C.byref(b)) == 0
        return b.value

    def ray_queue(self):
        q = self.trace.RayQueue_()
        q.capacity, q.offsets, q.dir, q.weight = self.n * 4, self.p, self.v3(self.capi.Vec3), self.v3(self.capi.Rgb)
        q.scratch, q.scratch_bytes = self.p, self._scratch(self.lib.rls_trace_scratch_bytes, self.n, self.spp_n)
        return q

    def shadow_queue(self, segments, specular=True, diffuse=True):
        """a light loop's queue of `segments` (3: a node's, 2: an rlSkin lobe's) rays a sample, with the weight planes named"""
        s = self.trace.ShadowQueue_()
        s.capacity, s.offsets, s.dir, s.maxdist = self.n * self.nl * segments * 4, self.p, self.v3(self.capi.Vec3), self.p
        if specular:
            s.weight_specular = self.v3(self.capi.Rgb)
        if diffuse:
            s.weight_diffuse = self.v3(self.capi.Rgb)
        s.kind, s.scratch = self.p, self.p
        s.scratch_bytes = self._scratch(self.lib.rls_trace_shadow_scratch_bytes, self.n, self.nl, self.spp_n)
        return s

    def probe_queue(self):
        q = self.trace.ProbeQueue_()
        q.capacity, q.offsets, q.origin, q.dir, q.maxdist = self.n * 4, self.p, self.v3(self.capi.Vec3), self.v3(self.capi.Vec3), self.p
        return q

    def probe_hits(self):
        h = self.trace.ProbeHits_()
        h.max_hits, h.stride, h.count = 2, self.n * 4, self.p
        h.P, h.N, h.irradiance = self.v3(self.capi.CVec3), self.v3(self.capi.CVec3), self.v3(self.capi.CRgb)
        return h

    def ray_state(self):
        return self.trace.RayState_(self.p, self.p, self.p, self.p, self.p)

    def add_closure(self, closure):
        """the closure with its wo / N / T planes, the points and the two lights of a node call"""
        self.c = closure
        self.c.wo, self.c.N, self.c.T = (self.v3(self.capi.CVec3) for _ in range(3))
        self.P = self.v3(self.capi.CVec3)
        self.lights = (self.capi.SphereLight * 2)()
        for l in self.lights:
            l.radius = 1.0

    def add_state(self):
        """the state planes and the depths of a bounce call"""
        self.state, self.depths = self.ray_state(), self.trace.GiDepths_(8, 2, 2, 4)
        self.sp, self.dp = C.byref(self.state), C.byref(self.depths)

    def cp(self):
        return C.byref(self.c) if self.c is not None else None


# ---- what the refusal tests of more than one family share ----------------------------------------------------------------------
SCRATCH = "queue.scratch is NULL or smaller than rls_trace_scratch_bytes"
SHADOW_SCRATCH = "queue.scratch is NULL or smaller than rls_trace_shadow_scratch_bytes"


def put(obj, name, value):
    """setattr as an expression, for the tables' edits"""
    setattr(obj, name, value)


class NodeWorld(Dummies):
    """rlGgx's or rlDisney's whole node (shade_emit / _resolve), with `bounce` the state-aware calls (bounce_emit / _resolve).
    One shape for the four: rlDisney carries an unused rls_ggx_shader and the shade calls an unused state, so that the tables
    edit the same attributes whichever call they run against."""

    def __init__(self, node, bounce=False):
        super().__init__()
        capi, trace = self.capi, self.trace
        self.node, self.bounce = node, bounce
        self.add_closure(capi.GgxClosure() if node == "ggx" else capi.DisneyClosure())
        self.sh = capi.GgxShader()
        self.shadow = self.shadow_queue(3)
        self.rays = [self.ray_queue() for _ in range(3 if node == "ggx" else 2)]
        self.q = (trace.GgxNodeQueues_ if node == "ggx" else trace.DisneyNodeQueues_)()
        self.q.shadow = C.pointer(self.shadow)
        for (name, _), r in zip(self.q._fields_[1:], self.rays):
            setattr(self.q, name, C.pointer(r))
        self.t = (trace.GgxNodeTraced_ if node == "ggx" else trace.DisneyNodeTraced_)()
        for name, _ in self.t._fields_:
            setattr(self.t, name, self.v3(capi.CRgb))
        self.out = (capi.GgxShadeOut if node == "ggx" else capi.DisneyShadeOut)()
        for name, _ in self.out._fields_:
            setattr(self.out, name, self.v3(capi.Rgb))
        self.qp, self.tp, self.op = C.byref(self.q), C.byref(self.t), C.byref(self.out)
        self.add_state()
        self.scale = capi.Param(None, 0.5)                       # rlDisney's two scales of the bounce resolve

    def emit(self):
        w, lib, state = self, self.lib, (self.sp, self.dp)
        if w.node == "ggx":
            head = (w.ctxp, w.n, w.cp(), C.byref(w.sh), w.P, w.lights, w.nl)
            return lib.rls_trace_ggx_bounce_emit(*head, w.spp_n, 7, 0, *state, w.qp) if w.bounce else \
                lib.rls_trace_ggx_shade_emit(*head, 1, w.spp_n, 7, 0, w.qp)
        head = (w.ctxp, w.n, w.cp(), w.P, w.lights, w.nl, w.spp_n, 7, 0)
        return lib.rls_trace_disney_bounce_emit(*head, *state, w.qp) if w.bounce else lib.rls_trace_disney_shade_emit(*head, w.qp)

    def resolve(self):
        w, lib, state = self, self.lib, (self.sp, self.dp)
        if w.node == "ggx":
            head = (w.ctxp, w.n, w.cp(), C.byref(w.sh), w.lights, w.nl)
            return lib.rls_trace_ggx_bounce_resolve(*head, w.spp_n, *state, w.qp, w.tp, w.op) if w.bounce else \
                lib.rls_trace_ggx_shade_resolve(*head, 1, w.spp_n, w.qp, w.tp, w.op)
        if w.bounce:
            return lib.rls_trace_disney_bounce_resolve(w.ctxp, w.n, w.cp(), w.scale, w.scale, w.lights, w.nl, w.spp_n, *state,
                                                       w.qp, w.tp, w.op)
        return lib.rls_trace_disney_shade_resolve(w.ctxp, w.n, w.lights, w.nl, w.spp_n, w.qp, w.tp, w.op)


# the tables: (what, edit of a valid world, message text)
BATCH = [                                                        # every node call, rlSkin's included
    ("ctx NULL", lambda w: put(w, "ctxp", None), "ctx is NULL"),
    ("n < 0", lambda w: put(w, "n", -1), "n < 0"),
    ("spp_n 0", lambda w: put(w, "spp_n", 0), "spp_n must be in [1, 16]"),
    ("spp_n 17", lambda w: put(w, "spp_n", 17), "spp_n must be in [1, 16]"),
    ("queues NULL", lambda w: put(w, "qp", None), "queues is NULL"),
    ("n_lights 9", lambda w: put(w, "nl", 9), "n_lights out of range (RLS_MAX_LIGHTS)"),
    ("n_lights -1", lambda w: put(w, "nl", -1), "n_lights out of range (RLS_MAX_LIGHTS)"),
]
OUTPUTS = [                                                      # every node resolve, rlSkin's included
    ("traced NULL", lambda w: put(w, "tp", None), "traced or out is NULL"),
    ("out NULL", lambda w: put(w, "op", None), "traced or out is NULL"),
    ("out.out partly set", lambda w: put(w.out, "out", w.capi.Rgb(w.p, None, None)), "out planes must be all set or all NULL"),
    ("ray weight NULL", lambda w: put(w.rays[0], "weight", w.none3(w.capi.Rgb)), "queue.weight plane is NULL"),
]
BOTH = BATCH + [                                                 # rlGgx and rlDisney, shade and bounce, emit and resolve
    ("shadow NULL with lights", lambda w: put(w.q, "shadow", None), "queues.shadow is NULL but n_lights > 0"),
    ("shadow set without lights", lambda w: put(w, "nl", 0), "queues.shadow is set but n_lights is 0"),
    ("a ray queue NULL", lambda w: put(w.q, w.q._fields_[-1][0], None), None),
    ("shadow capacity short", lambda w: put(w.shadow, "capacity", w.shadow.capacity - 1),
     "queue.capacity < n * n_lights * 3 * spp_n^2"),
    ("ray capacity short", lambda w: put(w.rays[-1], "capacity", w.rays[-1].capacity - 1), "queue.capacity < n * spp_n^2"),
    ("lights NULL", lambda w: put(w, "lights", None), None),
]
EMIT_ONLY = [
    ("ray scratch short", lambda w: put(w.rays[-1], "scratch_bytes", w.rays[-1].scratch_bytes - 1), SCRATCH),
    ("ray scratch NULL", lambda w: put(w.rays[-1], "scratch", None), SCRATCH),
    ("shadow scratch short", lambda w: put(w.shadow, "scratch_bytes", w.shadow.scratch_bytes - 1), SHADOW_SCRATCH),
    ("ray offsets NULL", lambda w: put(w.rays[0], "offsets", None), "queue.offsets is NULL"),
    ("ray dir NULL", lambda w: put(w.rays[0], "dir", w.none3(w.capi.Vec3)), "queue.dir plane is NULL"),
    ("P NULL", lambda w: put(w, "P", w.none3(w.capi.CVec3)), "wo/N/T/P plane is NULL"),
]
RESOLVE_ONLY = OUTPUTS + [
    ("an AOV plane NULL", lambda w: put(w.out, "indirect_specular", w.none3(w.capi.Rgb)), "NULL AOV plane"),
    ("visibility NULL", lambda w: put(w.t, "visibility", w.none3(w.capi.CRgb)), "visibility plane is NULL"),
    ("radiance NULL", lambda w: put(w.t, w.t._fields_[-1][0], w.none3(w.capi.CRgb)), "radiance plane is NULL"),
]
CLOSURE = ("closure NULL", lambda w: put(w, "c", None))
PLANES = "state.ray_type, state.Rr, state.Rr_diff, state.Rr_gloss or state.Rr_refr plane is NULL"
STATE = [("state NULL", lambda w: put(w, "sp", None), "state is NULL"),           # every bounce call, rlSkin's included
         ("depths NULL", lambda w: put(w, "dp", None), "depths is NULL")] + \
        [(f"state.{name} NULL", (lambda name: lambda w: put(w.state, name, None))(name), PLANES)
         for name in ("ray_type", "Rr", "Rr_diff", "Rr_gloss", "Rr_refr")]


def node_table(node, bounce, verb):
    """the rows that hold for rls_trace_<node>_<shade | bounce>_<verb>"""
    table = BOTH + (STATE if bounce else []) + (EMIT_ONLY if verb == "emit" else RESOLVE_ONLY)
    if node == "ggx":
        return table + [(*CLOSURE, "closure or shader is NULL")]
    if bounce or verb == "emit":                                 # (rls_trace_disney_shade_resolve takes no closure)
        return table + [(*CLOSURE, "closure is NULL")]
    return table


def empty_state(w):
    """an empty batch reads no state plane"""
    w.state = type(w.state)()
    w.sp = C.byref(w.state)
