"""CPU: the shadow rays' hits calls of the companion library (rls_trace_ggx_opacity, rls_trace_disney_opacity,
rls_trace_skin_opacity, rls_trace_shadow_visibility; include/rlshaders_amd_trace.h, librls_trace.so).

The four symbols are declared, exported and bound with matching arity and struct members; the header compiles as C99 and C++14;
the library still holds two code objects, the four mode-free kernels in the EXACT one and none in the product library; every
refusal comes through ctypes with dummy planes and a dummy context (refused before the context is read) with its exact message;
an empty batch succeeds without a device; the header's "Not covered:" paragraph no longer lists the two branches."""
import ctypes as C
import re
import subprocess

import pytest

from test_trace_shade_abi import HEADER, INVALID, ROOT, _declarations, trace_lib  # noqa: F401

ARITY = dict(rls_trace_ggx_opacity=5, rls_trace_disney_opacity=5, rls_trace_skin_opacity=6, rls_trace_shadow_visibility=5)
KERNELS = ("ggx_opacity_kernel", "disney_opacity_kernel", "skin_opacity_kernel", "shadow_visibility_kernel")
STRUCTS = (("GgxOpacity_", "rls_ggx_opacity"), ("DisneyOpacity_", "rls_disney_opacity"), ("SkinOpacity_", "rls_skin_opacity"),
           ("ShadowHits_", "rls_shadow_hits"))


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
    assert all(callable(getattr(trace, f)) for f in ("ggx_opacity", "disney_opacity", "skin_opacity", "ShadowHits",
                                                     "shadow_visibility"))
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for cls, c_name in STRUCTS:
        body = re.search(r"typedef struct %s\s*\{(.*?)\} %s;" % (c_name, c_name), text, flags=re.S).group(1)
        members = [re.findall(r"\w+", part)[-1] for d in body.split(";") if d.strip() for part in d.split(",")]
        assert members == [f[0] for f in getattr(trace, cls)._fields_], (c_name, members)
    # the section is the header's last: nothing is declared after the fold
    assert text.rindex("rls_trace_shadow_visibility") > max(text.rindex(s) for s in _declarations() if s not in ARITY)


def test_header_compiles_as_c_and_cxx(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "rlshaders_amd_trace.h"\n'
                   'int main(void){ rls_ggx_opacity g = {{0, 1.0f}, {0, 0, 0, 1.0f, 1.0f, 1.0f}, {0, 0, 0, 0.2f, 0.9f, 0.7f},\n'
                   '                                     {0, 0.5f}, {0, 0}};\n'
                   '  rls_disney_opacity d = {{0, 0, 0, 1.0f, 1.0f, 1.0f}, {0, 0}};\n'
                   '  rls_skin_opacity s = {{0, 1.0f}, {0, 0, 0, 1.0f, 1.0f, 1.0f}, {0, 0}};\n'
                   '  rls_shadow_hits h = {4, 0, 0, {0, 0, 0}, 0, 0}; rls_rgb o = {0, 0, 0}; rls_crgb b = {0, 0, 0};\n'
                   '  return rls_trace_ggx_opacity(0, 0, &g, 0, o) + rls_trace_disney_opacity(0, 0, &d, 0, o) +\n'
                   '         rls_trace_skin_opacity(0, 0, &s, 0, b, o) + rls_trace_shadow_visibility(0, 0, &h, b, o); }\n')
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++14")):
        p = subprocess.run([cc, std, "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{ROOT / 'include'}",
                            "-x", "c" if cc == "gcc" else "c++", str(src)], capture_output=True, text=True)
        assert p.returncode == 0, (cc, p.stderr)


def test_still_two_code_objects_with_the_four_kernels_in_the_exact_one(trace_lib):
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
    for elf in code_objects(fatbin(build.build_library())):
        for k in KERNELS:
            assert k.encode() not in elf, k


class World:
    """a valid argument set of the four calls over dummy planes (never read: every case below returns before a launch)"""

    def __init__(self):
        from rlshaders_amd import _capi as capi, trace
        self.capi, self.trace, self.lib = capi, trace, trace.load()
        self.ctx = C.create_string_buffer(4096)                  # non-NULL; a refused call does not read it
        self.mem = C.create_string_buffer(1 << 12)
        p = self.p = C.addressof(self.mem)
        self.ctxp, self.n = C.addressof(self.ctx), 8
        self.ggx = trace.GgxOpacity_(capi.Param(None, 1.0), capi.ParamRgb(None, None, None, 1.0, 1.0, 1.0),
                                     capi.ParamRgb(p, p, p, 0.0, 0.0, 0.0), capi.Param(p, 0.0), capi.MaterialIndex(p, 3))
        self.disney = trace.DisneyOpacity_(capi.ParamRgb(p, p, p, 0.0, 0.0, 0.0), capi.MaterialIndex(None, 0))
        self.skin = trace.SkinOpacity_(capi.Param(p, 0.0), capi.ParamRgb(None, None, None, 1.0, 1.0, 1.0),
                                       capi.MaterialIndex(None, 0))
        self.hits = trace.ShadowHits_(4, self.n, p, capi.CRgb(p, p, p), p, 2)
        self.params = dict(ggx=C.byref(self.ggx), disney=C.byref(self.disney), skin=C.byref(self.skin), fold=C.byref(self.hits))
        self.ray_type = p
        self.side = capi.CRgb(p, p, p)                           # rlSkin's incoming, the fold's base
        self.out = capi.Rgb(p, p, p)

    def call(self, verb):
        if verb == "ggx":
            return self.lib.rls_trace_ggx_opacity(self.ctxp, self.n, self.params[verb], self.ray_type, self.out)
        if verb == "disney":
            return self.lib.rls_trace_disney_opacity(self.ctxp, self.n, self.params[verb], self.ray_type, self.out)
        if verb == "skin":
            return self.lib.rls_trace_skin_opacity(self.ctxp, self.n, self.params[verb], self.ray_type, self.side, self.out)
        return self.lib.rls_trace_shadow_visibility(self.ctxp, self.n, self.params[verb], self.side, self.out)


ENTRY = dict(ggx="rls_trace_ggx_opacity", disney="rls_trace_disney_opacity", skin="rls_trace_skin_opacity",
             fold="rls_trace_shadow_visibility")
COLOURS = "colour planes must be all set or all NULL"
MATERIALS = "materials.id is set but materials.count is 0"


def _half(w, cls):
    return cls(w.p, None, w.p)


def _set(obj, name, value):
    setattr(obj, name, value)


OPACITY = [
    ("ctx NULL", lambda w, v: _set(w, "ctxp", None), "ctx is NULL"),
    ("n < 0", lambda w, v: _set(w, "n", -1), "n < 0"),
    ("struct NULL", lambda w, v: w.params.__setitem__(v, None), "params is NULL"),
    ("materials without count", lambda w, v: _set(getattr(w, v), "materials", w.capi.MaterialIndex(w.p, 0)), MATERIALS),
    ("output NULL", lambda w, v: _set(w, "out", w.capi.Rgb(None, None, None)), "NULL output plane"),
    ("output partly NULL", lambda w, v: _set(w, "out", _half(w, w.capi.Rgb)), "NULL output plane"),
]
PER_VERB = dict(
    ggx=[("opacity_color partly NULL", lambda w, v: _set(w.ggx.opacity_color, "g", w.p), COLOURS),
         ("KtColor partly NULL", lambda w, v: _set(w.ggx.KtColor, "b", None), COLOURS)],
    disney=[("opacity partly NULL", lambda w, v: _set(w.disney.opacity, "r", None), COLOURS)],
    skin=[("opacity_color partly NULL", lambda w, v: _set(w.skin.opacity_color, "r", w.p), COLOURS),
          ("incoming partly NULL", lambda w, v: _set(w, "side", _half(w, w.capi.CRgb)), "incoming planes must be all set or all NULL")])
FOLD = [
    ("ctx NULL", lambda w, v: _set(w, "ctxp", None), "ctx is NULL"),
    ("rays < 0", lambda w, v: _set(w, "n", -1), "rays < 0"),
    ("struct NULL", lambda w, v: w.params.__setitem__(v, None), "hits is NULL"),
    ("max_hits 0", lambda w, v: _set(w.hits, "max_hits", 0), "hits.max_hits must be in [1, 255]"),
    ("max_hits 256", lambda w, v: _set(w.hits, "max_hits", 256), "hits.max_hits must be in [1, 255]"),
    ("stride short", lambda w, v: _set(w.hits, "stride", w.n - 1), "hits.stride < rays"),
    ("index without table", lambda w, v: _set(w.hits, "table_count", 0), "hits.index is set but hits.table_count is 0"),
    ("base partly NULL", lambda w, v: _set(w, "side", _half(w, w.capi.CRgb)), "base planes must be all set or all NULL"),
    ("count NULL", lambda w, v: _set(w.hits, "count", None), "hits.count or hits.opacity plane is NULL"),
    ("opacity NULL", lambda w, v: _set(w.hits, "opacity", w.capi.CRgb(None, None, None)), "hits.count or hits.opacity plane is NULL"),
    ("opacity partly NULL", lambda w, v: _set(w.hits, "opacity", _half(w, w.capi.CRgb)), "hits.count or hits.opacity plane is NULL"),
    ("output NULL", lambda w, v: _set(w, "out", w.capi.Rgb(None, None, None)), "NULL output plane"),
    ("output partly NULL", lambda w, v: _set(w, "out", _half(w, w.capi.Rgb)), "NULL output plane"),
]


@pytest.mark.parametrize("verb", ["ggx", "disney", "skin", "fold"])
def test_every_refusal_names_the_entry_point(trace_lib, verb):
    from rlshaders_amd import _capi as capi
    wrong = []
    for what, breakit, text in (FOLD if verb == "fold" else OPACITY + PER_VERB[verb]):
        w = World()
        breakit(w, verb)
        st = w.call(verb)
        msg = capi.load().rls_last_error().decode()
        if st != INVALID or msg != f"{ENTRY[verb]}: {text}":
            wrong.append(f'{ENTRY[verb]} / {what}: status {st} "{msg}", want "{text}"')
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("verb", ["ggx", "disney", "skin", "fold"])
def test_an_empty_batch_succeeds_without_a_device(trace_lib, verb):
    """n == 0 / rays == 0 launches nothing: the dummy context is not read, no plane is needed; a NULL struct is still refused"""
    w = World()
    w.n = 0
    w.out, w.side, w.ray_type = w.capi.Rgb(None, None, None), w.capi.CRgb(None, None, None), None
    if verb == "fold":
        w.hits.stride, w.hits.count, w.hits.opacity, w.hits.index = 0, None, w.capi.CRgb(None, None, None), None
    assert w.call(verb) == 0
    w.params[verb] = None
    assert w.call(verb) == INVALID


def test_the_first_not_covered_paragraph_names_neither_branch():
    text = HEADER.read_text()
    block = " ".join(text.split("Not covered:")[1].split("*/")[0].replace(" * ", " ").split())
    assert "opacity branch" not in block and "shadow-ray branch" not in block
    assert "AiShaderGlobalsApplyOpacity" in block and "trace_diffuse" in block
    # the new section says what stays with the renderer
    tail = " ".join(text[text.index("Shadow rays' hits"):].replace(" * ", " ").split())
    assert "AiShaderGlobalsApplyOpacity" in tail and "closed service" in tail and "WITHOUT the shadow bit" in tail
    assert "bounding it is the renderer's job" in tail
