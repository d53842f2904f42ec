"""CPU: the shadow rays' hits calls of the companion library (rls_trace_ggx_opacity, rls_trace_disney_opacity,
rls_trace_skin_opacity, rls_trace_shadow_visibility; include/rlshaders_amd_trace.h, librls_trace.so).

Every refusal comes through ctypes with dummy planes and a dummy context (refused before the context is read) with its exact
message; an empty batch succeeds without a device; the section is the header's last, and its "Not covered:" paragraph no longer
lists the two branches.  The family's rows of tests/trace_abi_tables.py are checked with the whole table by
tests/test_trace_abi.py; the two tests that repeat those checks on this family's rows alone keep their names from before the
table."""
import ctypes as C

import pytest

from trace_abi_tables import FAMILIES
from trace_abi_util import (HEADER, INVALID, Dummies, check_absent_from_product, check_bound, check_callables, check_members,
                            check_placement, code_text, declarations, put, refusals, trace_lib)  # noqa: F401

F = FAMILIES["opacity"]


def test_declared_exported_and_bound_with_matching_arity(trace_lib):
    check_bound(trace_lib, F["arity"])
    check_callables(F["callables"])
    check_members(F["structs"])
    # the section is the header's last: nothing is declared after the fold
    text = code_text()
    assert text.rindex("rls_trace_shadow_visibility") > max(text.rindex(s) for s in declarations() if s not in F["arity"])


def test_still_two_code_objects_with_the_four_kernels_in_the_exact_one(trace_lib):
    check_placement(trace_lib, F["width"], F["mode"], F["free"])
    check_absent_from_product(F["free"])


class World(Dummies):
    """a valid argument set of one of the four calls (verb "fold": the visibility fold); `side` is rlSkin's incoming and the
    fold's base"""
    ENTRY = dict(ggx="rls_trace_ggx_opacity", disney="rls_trace_disney_opacity", skin="rls_trace_skin_opacity",
                 fold="rls_trace_shadow_visibility")

    def __init__(self, verb):
        super().__init__()
        capi, trace, p = self.capi, self.trace, self.p
        self.verb = verb
        self.ggx = trace.GgxOpacity_(capi.Param(None, 1.0), capi.ParamRgb(None, None, None, 1.0, 1.0, 1.0),
                                     capi.ParamRgb(p, p, p, 0.0, 0.0, 0.0), capi.Param(p, 0.0), capi.MaterialIndex(p, 3))
        self.disney = trace.DisneyOpacity_(capi.ParamRgb(p, p, p, 0.0, 0.0, 0.0), capi.MaterialIndex(None, 0))
        self.skin = trace.SkinOpacity_(capi.Param(p, 0.0), capi.ParamRgb(None, None, None, 1.0, 1.0, 1.0),
                                       capi.MaterialIndex(None, 0))
        self.hits = trace.ShadowHits_(4, self.n, p, capi.CRgb(p, p, p), p, 2)
        self.struct = dict(ggx=self.ggx, disney=self.disney, skin=self.skin, fold=self.hits)[verb]
        self.params = C.byref(self.struct)
        self.ray_type, self.side, self.out = p, self.v3(capi.CRgb), self.v3(capi.Rgb)

    def call(self):
        w, fn = self, getattr(self.lib, self.ENTRY[self.verb])
        if w.verb == "skin":
            return fn(w.ctxp, w.n, w.params, w.ray_type, w.side, w.out)
        if w.verb == "fold":
            return fn(w.ctxp, w.n, w.params, w.side, w.out)
        return fn(w.ctxp, w.n, w.params, w.ray_type, w.out)


COLOURS = "colour planes must be all set or all NULL"
HIT_PLANES = "hits.count or hits.opacity plane is NULL"
OUTPUT = [
    ("output NULL", lambda w: put(w, "out", w.none3(w.capi.Rgb)), "NULL output plane"),
    ("output partly NULL", lambda w: put(w, "out", w.half3(w.capi.Rgb)), "NULL output plane"),
]
OPACITY = [
    ("ctx NULL", lambda w: put(w, "ctxp", None), "ctx is NULL"),
    ("n < 0", lambda w: put(w, "n", -1), "n < 0"),
    ("struct NULL", lambda w: put(w, "params", None), "params is NULL"),
    ("materials without count", lambda w: put(w.struct, "materials", w.capi.MaterialIndex(w.p, 0)),
     "materials.id is set but materials.count is 0"),
] + OUTPUT
PER_VERB = dict(
    ggx=[("opacity_color partly NULL", lambda w: put(w.ggx.opacity_color, "g", w.p), COLOURS),
         ("KtColor partly NULL", lambda w: put(w.ggx.KtColor, "b", None), COLOURS)],
    disney=[("opacity partly NULL", lambda w: put(w.disney.opacity, "r", None), COLOURS)],
    skin=[("opacity_color partly NULL", lambda w: put(w.skin.opacity_color, "r", w.p), COLOURS),
          ("incoming partly NULL", lambda w: put(w, "side", w.half3(w.capi.CRgb)), "incoming planes must be all set or all NULL")])
FOLD = [
    ("ctx NULL", lambda w: put(w, "ctxp", None), "ctx is NULL"),
    ("rays < 0", lambda w: put(w, "n", -1), "rays < 0"),
    ("struct NULL", lambda w: put(w, "params", None), "hits is NULL"),
    ("max_hits 0", lambda w: put(w.hits, "max_hits", 0), "hits.max_hits must be in [1, 255]"),
    ("max_hits 256", lambda w: put(w.hits, "max_hits", 256), "hits.max_hits must be in [1, 255]"),
    ("stride short", lambda w: put(w.hits, "stride", w.n - 1), "hits.stride < rays"),
    ("index without table", lambda w: put(w.hits, "table_count", 0), "hits.index is set but hits.table_count is 0"),
    ("base partly NULL", lambda w: put(w, "side", w.half3(w.capi.CRgb)), "base planes must be all set or all NULL"),
    ("count NULL", lambda w: put(w.hits, "count", None), HIT_PLANES),
    ("opacity NULL", lambda w: put(w.hits, "opacity", w.none3(w.capi.CRgb)), HIT_PLANES),
    ("opacity partly NULL", lambda w: put(w.hits, "opacity", w.half3(w.capi.CRgb)), HIT_PLANES),
] + OUTPUT


@pytest.mark.parametrize("verb", ["ggx", "disney", "skin", "fold"])
def test_every_refusal_names_the_entry_point(trace_lib, verb):
    wrong = refusals(lambda: World(verb), World.call, World.ENTRY[verb], FOLD if verb == "fold" else OPACITY + PER_VERB[verb])
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("verb", ["ggx", "disney", "skin", "fold"])
def test_an_empty_batch_succeeds_without_a_device(trace_lib, verb):
    """n == 0 / rays == 0 launches nothing: the dummy context is not read, no plane is needed; a NULL struct is still refused"""
    w = World(verb)
    w.n = 0
    w.out, w.side, w.ray_type = w.none3(w.capi.Rgb), w.none3(w.capi.CRgb), None
    w.hits.stride, w.hits.count, w.hits.opacity, w.hits.index = 0, None, w.none3(w.capi.CRgb), None
    assert w.call() == 0
    w.params = None
    assert w.call() == INVALID


def test_the_first_not_covered_paragraph_names_neither_branch():
    text = HEADER.read_text()
    block = " ".join(text.split("Not covered:")[1].split("*/")[0].replace(" * ", " ").split())
    assert "opacity branch" not in block and "shadow-ray branch" not in block
    assert "AiShaderGlobalsApplyOpacity" in block and "trace_diffuse" in block
    # the new section says what stays with the renderer
    tail = " ".join(text[text.index("Shadow rays' hits"):].replace(" * ", " ").split())
    assert "AiShaderGlobalsApplyOpacity" in tail and "closed service" in tail and "WITHOUT the shadow bit" in tail
    assert "bounding it is the renderer's job" in tail
