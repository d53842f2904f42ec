"""CPU: the traversal of librls_nearest.so -- the host + device functions of rlshaders_amd/csrc_nearest/rls_nearest_device.hpp,
compiled for the host with -ffp-contract=off by tests/native/nearest_host_check.cpp -- equals that program's own brute force over
the statement of include/rlshaders_amd_nearest.h bit for bit in (hit, t, prim): 10^6 rays over the icosphere, the quad grid and a
1025-triangle soup with degenerate triangles, for leaf_size 1, 2, 4 and 8, random and hostile rays (vertices and edges, signed
zeros, origins on box planes, NaN / inf, hostile reaches, skipped triangles).  The same program runs once more, on fewer rays,
under the address and undefined-behaviour sanitizers: a stand-alone binary, nothing is loaded into Python."""
import re

import pytest

from nearest_host_check_util import build, run

RAYS = 1_000_000


def _check(lines, rays):
    assert lines and all(l.startswith("ok ") for l in lines), "\n".join(l for l in lines if not l.startswith("ok "))
    assert len(lines) == 3 * 4 + 1
    total = re.fullmatch(r"ok traverse: (\d+) rays, 0 differ", lines[-1])
    assert total and int(total.group(1)) >= rays
    for mesh in ("icosphere", "quad grid", "soup"):
        assert sorted(int(m.group(1)) for l in lines for m in [re.match(rf"ok {mesh} leaf (\d):", l)] if m) == [1, 2, 4, 8]


def test_traversal_equals_the_brute_force(tmp_path):
    _check(run(build(tmp_path), "traverse", RAYS), RAYS)


def test_the_same_program_under_sanitizers(tmp_path):
    exe = build(tmp_path, sanitize=True)
    assert run(exe, "bvh") == ["ok bvh"]
    _check(run(exe, "traverse", 60_000), 60_000)
