"""CPU: the secondary-ray calls of the companion library (rls_trace_ggx_bounce_emit / _resolve, rls_trace_disney_bounce_emit /
_resolve, rls_trace_ray_state_advance; include/rlshaders_amd_trace.h, librls_trace.so).

Every refusal -- the node calls' table and the state's (tests/trace_abi_util.py) -- returns RLS_ERR_INVALID_ARGUMENT with the
entry point's name in the message.  The checks run through ctypes with dummy planes and a dummy context: a refused call returns
before the context is read.  The family's rows of tests/trace_abi_tables.py are checked with the whole table by
tests/test_trace_abi.py; the three tests that repeat those checks on this family's rows alone keep their names from before the
table."""
import ctypes as C

import pytest

from trace_abi_tables import FAMILIES
from trace_abi_util import (INVALID, PLANES, Dummies, NodeWorld, check_absent_from_product, check_bound, check_callables,
                            check_members, check_placement, empty_state, node_table, put, refusals, trace_lib)  # noqa: F401

F = FAMILIES["bounce"]


def test_declared_exported_and_bound_with_matching_arity(trace_lib):
    check_bound(trace_lib, F["arity"])
    check_callables(F["callables"])
    check_members(F["structs"])          # (the RLS_RT_* bits: tests/test_trace_abi.py::test_the_constants_are_the_headers)


def test_still_two_code_objects_with_the_bounce_kernels(trace_lib):
    check_placement(trace_lib, F["width"], F["mode"], F["free"])


def test_no_bounce_kernel_in_the_product_library(trace_lib):
    check_absent_from_product(F["width"] + F["free"])


@pytest.mark.parametrize("verb", ["emit", "resolve"])
@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_every_refusal_names_the_entry_point(trace_lib, node, verb):
    wrong = refusals(lambda: NodeWorld(node, bounce=True), lambda w: getattr(w, verb)(), f"rls_trace_{node}_bounce_{verb}",
                     node_table(node, True, verb))
    assert not wrong, "\n".join(wrong)


class AdvanceWorld(Dummies):
    """rls_trace_ray_state_advance over 4 rays"""

    def __init__(self):
        super().__init__()
        self.rays, self.point, self.ray_type = 4, self.p, 0x40
        self.parent, self.child = self.ray_state(), self.ray_state()
        self.pp, self.chp = C.byref(self.parent), C.byref(self.child)

    def call(self):
        return self.lib.rls_trace_ray_state_advance(self.ctxp, self.rays, self.point, self.pp, self.ray_type, self.chp)


ADVANCE = [
    ("ctx NULL", lambda w: put(w, "ctxp", None), "ctx is NULL"),
    ("rays < 0", lambda w: put(w, "rays", -1), "rays < 0"),
    ("parent NULL", lambda w: put(w, "pp", None), "parent or child is NULL"),
    ("child NULL", lambda w: put(w, "chp", None), "parent or child is NULL"),
    ("ray_type 0x100", lambda w: put(w, "ray_type", 0x100), "ray_type is not a byte of RLS_RT_* bits"),
    ("point NULL", lambda w: put(w, "point", None), "point is NULL"),
    ("a child plane NULL", lambda w: put(w.child, "Rr_refr", None), PLANES),
    ("a parent plane NULL", lambda w: put(w.parent, "Rr_refr", None), PLANES),
]


def test_the_advance_call_refuses_by_name_and_takes_no_rays_without_a_device(trace_lib):
    wrong = refusals(AdvanceWorld, AdvanceWorld.call, "rls_trace_ray_state_advance", ADVANCE)
    assert not wrong, "\n".join(wrong)
    w = AdvanceWorld()                   # rays == 0 launches nothing: the dummy context is not read
    w.rays, w.point = 0, None
    assert w.call() == 0


@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_a_resolve_of_nothing_succeeds_without_a_device(trace_lib, node):
    w = NodeWorld(node, bounce=True)
    w.n = 0
    empty_state(w)
    assert w.resolve() == 0
    w.sp = None
    assert w.resolve() == INVALID
