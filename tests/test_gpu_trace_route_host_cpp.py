"""GPU: the C++ mirror of the routing calls (rlshaders_amd/host/rls_trace.hpp: HitRoutes, routeHits, gatherHits, scatterToRays,
fillMisses) end to end.  host/example_trace_path.cpp shades a camera batch, routes its glossy queue's stand-in hits to an rlGgx
and an rlDisney batch and the misses, shades the batches and resolves the camera batch with their out; the bin sizes and the bits
of every plane it reports equal the Python path (tests/trace_route_util.py, two_bounces) on the same inputs."""
import json
import subprocess

import pytest

import trace_route_util as U
from test_gpu_trace_host_cpp import _fnv

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,spp_n", [(777, 3), (300, 2)])
def test_the_path_example_matches_the_python_path(n, spp_n):
    import numpy as np
    import rlshaders_amd as R
    from rlshaders_amd import build
    exe = build.build_trace_example(name="example_trace_path")
    p = subprocess.run([str(exe), str(n), str(spp_n)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["points"] == n and got["spp_n"] == spp_n
    ctx = R.Context(0)
    try:
        want = U.two_bounces(ctx, n, spp_n, U.example_bins, "route")
    finally:
        ctx.close()
    assert got["rays"] == want["rays"] > n and got["sizes"] == want["sizes"] and min(got["sizes"]) > 0
    aovs = np.concatenate([want[k] for k in R.GgxSampler.SHADE_AOVS])
    for key, planes in (("out0", want["out0"]), ("out1", want["out1"]), ("radiance", want["radiance"]), ("aovs", aovs),
                        ("out", want["out"])):
        assert got[key] == _fnv(planes), key
    assert got["mean_out"] > 0
