"""GPU: the secondary-ray calls (rls_trace_ggx_bounce_* / rls_trace_disney_bounce_*) where their kernels' loops take more than one
round, as tests/test_gpu_trace_node_edges.py holds the node calls there.

On a context of one workgroup per CU a round of the bounce resolves' loops and of the state-aware emits' (at one lane per point)
covers compute_units x kBlock points; n = 2.5 x compute_units x kBlock (+ a ragged tail) gives every new emit kernel and both
resolve kernels two and a half rounds.  Every queue plane and every output holds the bytes of the default context, whose
results tests/test_gpu_trace_bounce.py holds to the existing calls; rls_trace_ray_state_advance likewise, over the shadow
queue's rays."""
import numpy as np
import pytest
import torch

from gpu_util import host
from test_gpu_shade import _lights
from test_gpu_trace_bounce import DEPTHS, GLS, Bounce, _planes, _queue_hosts, _resolve, _same_queues
from test_gpu_trace_node_edges import _with_group, one_block_per_cu  # noqa: F401
from test_gpu_trace_shade import KBLOCK, T, _same  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("node", ["ggx", "disney"])
def test_two_and_a_half_grid_rounds_of_every_bounce_kernel(gpu, oracle, T, one_block_per_cu, node, fast):
    ctx = one_block_per_cu
    rnd = ctx.device_info()["compute_units"] * KBLOCK
    n, spp_n = 2 * rnd + rnd // 2 + 37, 2
    _, lights = _lights(oracle)
    for c in (gpu, ctx):
        c.set_math_mode(fast)
    try:
        b1, b0 = Bounce(T, ctx, oracle, node, n), Bounce(T, gpu, oracle, node, n)
        st, s1 = b1.state()
        _, s0 = b0.state()
        for g in (1, 64):
            q1 = _with_group(g, lambda: b1.bounce(lights, spp_n, s1, DEPTHS))
            q0 = _with_group(g, lambda: b0.bounce(lights, spp_n, s0, DEPTHS))
            h1 = _queue_hosts(q1)
            _same_queues(h1, _queue_hosts(q0), (node, g, "emit vs the default context"))
            assert all(h["count"] > n // 8 for h in h1.values()), {r: h["count"] for r, h in h1.items()}
            planes = _planes(gpu, q0, seed=7)
            _same(_resolve(q1, planes), _resolve(q0, planes), (node, g, "resolve vs the default context"))
        # the advance kernel over the shadow queue's rays: several rounds too
        q = q1.shadow
        assert q.count > 2 * rnd + rnd // 2
        c1, c0 = T.advance_state(ctx, q, s1, GLS), T.advance_state(gpu, q0.shadow, s0, GLS)
        for k in T.RayState.PLANES:
            assert torch.equal(getattr(c1, k), getattr(c0, k)), k
        pts = host(q.point).astype(np.int64)
        np.testing.assert_array_equal(host(c1.Rr_gloss), np.minimum(255, st[3][pts].astype(np.int64) + 1).astype(np.uint8))
    finally:
        for c in (gpu, ctx):
            c.set_math_mode(False)
