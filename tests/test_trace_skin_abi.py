"""CPU: the caller-traced rlSkin node in the companion library and its secondary-ray calls (rls_trace_skin_emit / _resolve,
rls_trace_skin_bounce_emit / _resolve; include/rlshaders_amd_trace.h, librls_trace.so).

Every refusal -- the node's tables, the state's (tests/trace_abi_util.py) and the sixth queue's -- returns
RLS_ERR_INVALID_ARGUMENT with the entry point's name in the message.  The checks run through ctypes with dummy planes and a dummy
context: a refused call returns before the context is read or anything is launched, so no device is needed.  The two families'
rows of tests/trace_abi_tables.py are checked with the whole table by tests/test_trace_abi.py; the four tests that repeat those
checks on these rows alone keep their names from before the table."""
import ctypes as C

import pytest

from trace_abi_tables import FAMILIES, every
from trace_abi_util import (BATCH, CLOSURE, INVALID, OUTPUTS, SCRATCH, SHADOW_SCRATCH, STATE, Dummies, check_absent_from_product,
                            check_bound, check_callables, check_members, check_placement, empty_state, last_error, put, refusals,
                            trace_lib)  # noqa: F401

F, FB = FAMILIES["skin"], FAMILIES["skin_bounce"]


def test_declared_exported_and_bound_with_matching_arity(trace_lib):
    check_bound(trace_lib, {**F["arity"], **FB["arity"]})
    check_callables(F["callables"] + FB["callables"])
    check_members(F["structs"] + FB["structs"])


def test_two_code_objects_with_the_skin_kernels(trace_lib):
    check_placement(trace_lib, F["width"] + FB["width"], F["mode"] + FB["mode"], ())


def test_the_fast_unit_holds_no_copy_of_a_mode_free_kernel(trace_lib):
    """the scan, compaction and resolve kernels are templates (or guarded) and are launched from the EXACT unit's host code
    alone: the FAST code object must not instantiate any of them -- nor any other mode-free kernel of the table"""
    check_placement(trace_lib, (), (), every("free"))


def test_no_skin_node_kernel_in_the_product_library(trace_lib):
    check_absent_from_product(F["width"] + F["mode"] + FB["width"] + FB["mode"])


# ---- argument checks, no device ------------------------------------------------------------------------------------------------
class World(Dummies):
    """rlSkin's whole node (skin_emit / _resolve); with `bounce` the state-aware calls, whose structs embed the node's first:
    `q` and `t` are the node structs either way (views into `bq` / `bt`), so one set of tables edits both.  (The bounce structs,
    the sixth queue and the state are built for the node calls too, unused: one shape for the tables.)"""

    def __init__(self, bounce=False):
        super().__init__()
        capi, trace = self.capi, self.trace
        self.bounce = bounce
        self.add_closure(capi.SkinClosure())
        self.shadows = [self.shadow_queue(2, diffuse=False) for _ in range(2)]
        self.rays = [self.ray_queue() for _ in range(2)]
        self.probes, self.hits = self.probe_queue(), self.probe_hits()
        self.bq, self.bt = trace.SkinBounceQueues_(), trace.SkinBounceTraced_()
        q, t = (self.bq.node, self.bt.node) if bounce else (trace.SkinNodeQueues_(), trace.SkinNodeTraced_())
        q.sheen_shadow, q.specular_shadow = C.pointer(self.shadows[0]), C.pointer(self.shadows[1])
        q.sheen_glossy, q.specular_glossy = C.pointer(self.rays[0]), C.pointer(self.rays[1])
        q.probes = C.pointer(self.probes)
        q.sheenFresnel = q.specularFresnel = q.sssWeight = self.p
        for name in ("sheen_visibility", "specular_visibility", "sheen_glossy", "specular_glossy"):
            setattr(t, name, self.v3(capi.CRgb))
        t.hits = C.pointer(self.hits)
        self.q, self.t = q, t
        self.out = capi.SkinIntegrateOut()
        for name in ("sheen", "specular", "sss", "out"):
            setattr(self.out, name, self.v3(capi.Rgb))
        # the sixth queue: integrateScatter's light loop on diffuse rays, hit-list-shaped (weight_diffuse.r its only weight plane)
        self.diffuse = self.shadow_queue(2, specular=False)
        self.diffuse.weight_diffuse = capi.Rgb(self.p, None, None)
        self.bq.diffuse_shadow = C.pointer(self.diffuse)
        self.bt.diffuse_visibility = self.v3(capi.CRgb)
        self.qp, self.tp = (C.byref(self.bq), C.byref(self.bt)) if bounce else (C.byref(q), C.byref(t))
        self.op = C.byref(self.out)
        self.add_state()

    def emit(self):
        w = self
        head = (w.ctxp, w.n, w.cp(), w.P, w.lights, w.nl, w.spp_n, 7, 0)
        return w.lib.rls_trace_skin_bounce_emit(*head, w.sp, w.dp, w.qp) if w.bounce else w.lib.rls_trace_skin_emit(*head, w.qp)

    def resolve(self):
        w = self
        head = (w.ctxp, w.n, w.cp(), w.P, w.lights, w.nl, 0, 0, w.spp_n)
        return w.lib.rls_trace_skin_bounce_resolve(*head, w.sp, w.dp, w.qp, w.tp, w.op) if w.bounce else \
            w.lib.rls_trace_skin_resolve(*head, w.qp, w.tp, w.op)


BOTH = BATCH + [
    ("lights NULL", lambda w: put(w, "lights", None), "lights is NULL"),
    ("one shadow NULL with lights", lambda w: put(w.q, "specular_shadow", None),
     "queues.sheen_shadow or queues.specular_shadow is NULL but n_lights > 0"),
    ("shadows set without lights", lambda w: put(w, "nl", 0), "queues.sheen_shadow or queues.specular_shadow is set but n_lights is 0"),
    ("a glossy queue NULL", lambda w: put(w.q, "specular_glossy", None),
     "queues.sheen_glossy, queues.specular_glossy or queues.probes is NULL"),
    ("probes NULL", lambda w: put(w.q, "probes", None), "queues.sheen_glossy, queues.specular_glossy or queues.probes is NULL"),
    ("a scalar plane NULL", lambda w: put(w.q, "sssWeight", None),
     "queues.sheenFresnel, queues.specularFresnel or queues.sssWeight is NULL"),
    ("offsets NULL", lambda w: put(w.rays[0], "offsets", None), "queue.offsets is NULL"),
    (*CLOSURE, "closure is NULL"),
    ("P NULL", lambda w: put(w, "P", w.none3(w.capi.CVec3)), "wo/N/T/P plane is NULL"),
    ("shadow capacity short", lambda w: put(w.shadows[1], "capacity", w.shadows[1].capacity - 1),
     "queue.capacity < n * n_lights * 2 * spp_n^2"),
    ("shadow weight NULL", lambda w: put(w.shadows[0], "weight_specular", w.none3(w.capi.Rgb)), "queue.weight_specular plane is NULL"),
    ("ray capacity short", lambda w: put(w.rays[1], "capacity", w.rays[1].capacity - 1), "queue.capacity < n * spp_n^2"),
    ("probe capacity short", lambda w: put(w.probes, "capacity", w.probes.capacity - 1), "queue.capacity < n * spp_n^2"),
]
# (the world sizes a lobe's scratch with rls_trace_shadow_scratch_bytes, more than its two-segment loop needs: hence 16 bytes,
# not one byte less)
EMIT_ONLY = [
    ("ray scratch short", lambda w: put(w.rays[1], "scratch_bytes", 16), SCRATCH),
    ("ray scratch NULL", lambda w: put(w.rays[0], "scratch", None), SCRATCH),
    ("shadow scratch short", lambda w: put(w.shadows[0], "scratch_bytes", 16), SHADOW_SCRATCH),
    ("shadow scratch NULL", lambda w: put(w.shadows[1], "scratch", None), SHADOW_SCRATCH),
    ("ray dir NULL", lambda w: put(w.rays[0], "dir", w.none3(w.capi.Vec3)), "queue.dir plane is NULL"),
    ("probe maxdist NULL", lambda w: put(w.probes, "maxdist", None), "queue.origin, queue.dir or queue.maxdist plane is NULL"),
]
RESOLVE_ONLY = OUTPUTS + [
    ("hits NULL", lambda w: put(w.t, "hits", None), "traced.hits is NULL"),
    ("max_hits 0", lambda w: put(w.hits, "max_hits", 0), "hits.max_hits must be in [1, 12]"),
    ("max_hits 13", lambda w: put(w.hits, "max_hits", 13), "hits.max_hits must be in [1, 12]"),
    ("stride short", lambda w: put(w.hits, "stride", w.n * 4 - 1), "hits.stride < n * spp_n^2"),
    ("a hit plane NULL", lambda w: put(w.hits, "count", None), "hits.count, hits.P, hits.N or hits.irradiance plane is NULL"),
    ("an AOV plane NULL", lambda w: put(w.out, "sss", w.none3(w.capi.Rgb)), "NULL AOV plane"),
    ("visibility NULL", lambda w: put(w.t, "specular_visibility", w.none3(w.capi.CRgb)), "visibility plane is NULL"),
    ("radiance NULL", lambda w: put(w.t, "sheen_glossy", w.none3(w.capi.CRgb)), "radiance plane is NULL"),
]


def _no_lights_but_sixth(w):
    w.nl = 0
    w.q.sheen_shadow = None
    w.q.specular_shadow = None


SIXTH = [
    ("diffuse_shadow NULL with lights", lambda w: put(w.bq, "diffuse_shadow", None), "queues.diffuse_shadow is NULL but n_lights > 0"),
    ("diffuse_shadow offsets NULL", lambda w: put(w.diffuse, "offsets", None), "queue.offsets is NULL"),
    ("diffuse_shadow dir NULL", lambda w: put(w.diffuse, "dir", w.none3(w.capi.Vec3)), "queue.dir or queue.maxdist plane is NULL"),
    ("diffuse_shadow weight NULL", lambda w: put(w.diffuse, "weight_diffuse", w.none3(w.capi.Rgb)),
     "queue.weight_specular or queue.weight_diffuse plane is NULL"),
    ("diffuse_shadow kind NULL", lambda w: put(w.diffuse, "kind", None), "queue.kind is NULL"),
    ("diffuse_shadow capacity short", lambda w: put(w.diffuse, "capacity", w.diffuse.capacity - 1),
     "queue.capacity < n * n_lights * 2 * spp_n^2"),
    ("diffuse_shadow set without lights", _no_lights_but_sixth, "queues.diffuse_shadow is set but n_lights is 0"),
]
SIXTH_EMIT = [
    ("diffuse_shadow scratch short", lambda w: put(w.diffuse, "scratch_bytes", 16), SHADOW_SCRATCH),
    ("diffuse_shadow scratch NULL", lambda w: put(w.diffuse, "scratch", None), SHADOW_SCRATCH),
]
SIXTH_RESOLVE = [
    ("diffuse_visibility NULL", lambda w: put(w.bt, "diffuse_visibility", w.none3(w.capi.CRgb)), "visibility plane is NULL"),
]


@pytest.mark.parametrize("verb", ["emit", "resolve"])
def test_argument_checks_name_the_entry_point(trace_lib, verb):
    wrong = refusals(World, lambda w: getattr(w, verb)(), f"rls_trace_skin_{verb}",
                     BOTH + (EMIT_ONLY if verb == "emit" else RESOLVE_ONLY))
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("verb", ["emit", "resolve"])
def test_the_bounce_calls_refuse_by_name_before_the_context_is_read(trace_lib, verb):
    table = BOTH + STATE + SIXTH + (EMIT_ONLY + SIXTH_EMIT if verb == "emit" else RESOLVE_ONLY + SIXTH_RESOLVE)
    wrong = refusals(lambda: World(bounce=True), lambda w: getattr(w, verb)(), f"rls_trace_skin_bounce_{verb}", table)
    assert not wrong, "\n".join(wrong)


def test_a_resolve_of_nothing_succeeds_without_a_device(trace_lib):
    w = World()
    w.n = 0
    assert w.resolve() == 0
    w.spp_n = 17
    assert w.resolve() == INVALID


def test_a_bounce_resolve_of_nothing_succeeds_without_a_device(trace_lib):
    w = World(bounce=True)
    w.n = 0
    empty_state(w)
    assert w.resolve() == 0
    w.sp = None
    assert w.resolve() == INVALID


@pytest.mark.parametrize("node", ["skin", "skin_bounce"])
def test_an_emit_refused_at_its_last_shadow_queue_launches_nothing(trace_lib, node):
    """A valid call but for the last-checked argument of the queue that is filled last (the second lobe's shadow queue; of the
    bounce call the sixth queue), its scratch too small: every check of the node emit runs ahead of its first launch, so the call
    is refused with the entry point's name before the (dummy) context is read -- the emits earlier in stream order included."""
    w = World(bounce=node == "skin_bounce")
    (w.diffuse if w.bounce else w.shadows[1]).scratch_bytes = 16
    assert w.emit() == INVALID
    assert last_error() == f"rls_trace_{node}_emit: {SHADOW_SCRATCH}"
