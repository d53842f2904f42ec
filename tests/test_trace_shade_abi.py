"""CPU: the caller-traced whole nodes in the companion library (rls_trace_ggx_shade_emit / _resolve,
rls_trace_disney_shade_emit / _resolve; include/rlshaders_amd_trace.h, librls_trace.so).

Every argument check returns RLS_ERR_INVALID_ARGUMENT with the entry point's name in the message.  The checks run through
ctypes with dummy planes and a dummy context (tests/trace_abi_util.py's NodeWorld): a refused call returns before the context is
read or anything is launched, so no device is needed.  The family's rows of tests/trace_abi_tables.py are checked with the whole
table by tests/test_trace_abi.py; the three tests that repeat those checks on this family's rows alone keep their names from
before the table."""
import pytest

from trace_abi_tables import FAMILIES
from trace_abi_util import (INVALID, SCRATCH, NodeWorld, check_absent_from_product, check_bound, check_callables, check_members,
                            check_placement, last_error, node_table, refusals, trace_lib)  # noqa: F401

F = FAMILIES["shade"]


def test_declared_exported_and_bound_with_matching_arity(trace_lib):
    check_bound(trace_lib, F["arity"])
    check_callables(F["callables"])
    check_members(F["structs"])


def test_two_code_objects_with_the_node_kernels(trace_lib):
    check_placement(trace_lib, F["width"], F["mode"], F["free"])


def test_no_node_kernel_in_the_product_library(trace_lib):
    check_absent_from_product(F["width"] + F["free"])


@pytest.mark.parametrize("verb", ["emit", "resolve"])
@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_argument_checks_name_the_entry_point(trace_lib, node, verb):
    wrong = refusals(lambda: NodeWorld(node), lambda w: getattr(w, verb)(), f"rls_trace_{node}_shade_{verb}",
                     node_table(node, False, verb))
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_a_resolve_of_nothing_succeeds_without_a_device(trace_lib, node):
    """n == 0: the resolve has nothing to write and launches nothing (the emit of n == 0 writes offsets[0] = 0 on the device:
    tests/test_gpu_trace_shade.py)"""
    w = NodeWorld(node)
    w.n = 0
    assert w.resolve() == 0
    w.spp_n = 17
    assert w.resolve() == INVALID


@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_an_emit_refused_at_its_last_ray_queue_launches_nothing(trace_lib, node):
    """A valid call but for the last-checked argument of the last ray queue, its scratch one byte short: every check of a
    node emit runs ahead of its first launch, so the call is refused with the entry point's name before the (dummy) context
    is read -- the light loop's emit, first in stream order, included."""
    w = NodeWorld(node)
    w.rays[-1].scratch_bytes -= 1
    assert w.emit() == INVALID
    assert last_error() == f"rls_trace_{node}_shade_emit: {SCRATCH}"
