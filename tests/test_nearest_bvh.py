"""CPU: the tree of librls_nearest.so (rlshaders_amd/csrc_nearest/rls_nearest_bvh.hpp) built by the stand-alone host program
tests/native/nearest_host_check.cpp -- no HIP, no library: for leaf_size 1, 2, 4, 8 and nt = 0, 1, 2, 3, 1025, the icosphere, the
quad grid and 64 coincident triangles, every triangle is in exactly one leaf, every node's box contains its children's and its
triangles', the depth is within ceil(log2(nt / leaf)) + 1, a second build gives the same bytes; the header compiles without
HIP, which the program's build shows; and the triangle limit fits the stack as arithmetic over the header's constants (a tree of
that size, and the deep trees that fill the stack, are built by test_nearest_deep.py)."""
import math
import re

import pytest

from nearest_host_check_util import ROOT, build, run

BVH = ROOT / "rlshaders_amd" / "csrc_nearest" / "rls_nearest_bvh.hpp"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("nearest_bvh"))


def test_tree_invariants(exe):
    assert run(exe, "bvh") == ["ok bvh"]


def test_the_builder_needs_no_hip_and_the_limit_fits_the_stack():
    text = BVH.read_text()
    assert "hip" not in re.sub(r"//.*", "", text).lower()
    header = (ROOT / "include" / "rlshaders_amd_nearest.h").read_text()
    stack = int(re.search(r"#define RLS_NEAREST_STACK (\d+)", header).group(1))
    shift = int(re.search(r"#define RLS_NEAREST_MAX_TRIANGLES \(\(int64_t\)1 << (\d+)\)", header).group(1))
    # leaf_size 1: ceil(log2(nt)) + 1 levels, one stack entry per inner level
    assert math.ceil(math.log2(1 << shift)) + 1 - 1 <= stack
    device = (ROOT / "rlshaders_amd" / "csrc_nearest" / "rls_nearest_device.hpp").read_text()
    assert f"constexpr int kNearestStack = {stack};" in device
