"""GPU: the C++ mirror of the caller-traced whole nodes (rlshaders_amd/host/rls_trace.hpp: GgxNodeQueues, DisneyNodeQueues,
emitNode, resolveNode) end to end.  host/example_trace.cpp emits every queue of the rlGgx and the rlDisney node under two
lights, shadows the second light with the half-space x > 3 on the host, lights the ray queues with its sky and resolves; the
ray counts per queue, the blocked rays and the bits of the AOVs and of sg->out.RGB equal the Python path
(rlshaders_amd/trace.py) on the same inputs, and the direct AOVs equal the analytic node call with the first light alone."""
import json
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_trace_host_cpp import _fnv
from test_gpu_trace_lights_host_cpp import LIGHTS, SEED

pytestmark = pytest.mark.gpu

SHADER = dict(KdColor=(0.7, 0.5, 0.2), Kd=0.8, diffuseRoughness=0.3, Ks=0.6, KtColor=(0.2, 0.9, 0.7), Kt=0.5)


def _sky(q):
    """example_trace.cpp, sky(): float32, brighter towards +z, warm-tinted"""
    up = 0.25 + 0.75 * torch.clamp(q.dir[2], min=0.0)
    L = torch.stack([up, up * 0.875, up * 0.75]).contiguous()
    return L if L.shape[1] else torch.zeros(3, 1, device=L.device)


def _python_path(n, spp_n):
    import rlshaders_amd as R
    from rlshaders_amd import trace as T
    from rlshaders_amd.closures import make_light
    ctx = R.Context(0)
    try:
        wo, N, Tn = R.gen_frame(ctx, SEED, 0, n)
        lights = [make_light(**kw) for kw in LIGHTS]
        P = torch.zeros(3, n, device=ctx.torch_device)
        g = R.GgxSampler(ctx, wo, N, Tn, specColor=(0.9, 0.6, 0.3), roughness=0.4, ior=1.6, anisotropic=0.5)
        d = R.DisneySampler(ctx, wo, N, Tn, base_color=(0.8, 0.5, 0.3), subsurface=0.1, metallic=0.2, specular=0.5,
                            specular_tint=0.1, roughness=0.35, anisotropic=0.3, sheen=0.2, sheen_tint=0.5, clearcoat=0.3,
                            clearcoat_gloss=0.6)
        got = {}
        for name in ("ggx_node", "disney_node"):
            if name == "ggx_node":
                nq = T.ggx_node_rays(g, T.ggx_shader(g, **SHADER), P, lights, spp_n, SEED)
                alone = g.shade(P, lights[0], spp_n, SEED, **SHADER)
                s = g
            else:
                nq = T.disney_node_rays(d, P, lights, spp_n, SEED)
                alone = d.shade(P, lights[0], spp_n, SEED)
                s = d
            sq = nq.shadow
            blocked = (sq.maxdist * sq.dir[0]) > 3.0
            vis = (~blocked).to(torch.float32)[None, :].repeat(3, 1).contiguous()
            out = nq.resolve(vis, *[_sky(getattr(nq, r)) for r in nq.RAYS])
            aovs = np.concatenate([out[k].cpu().numpy() for k in s.SHADE_AOVS])
            got[name] = {"rays": [sq.count] + [getattr(nq, r).count for r in nq.RAYS], "blocked": int(blocked.sum().item()),
                         "aovs": _fnv(aovs), "out": _fnv(out["out"].cpu().numpy())}
            # the shadowed light adds +0: by value the first light alone
            for k in ("direct_diffuse", "direct_specular"):
                np.testing.assert_array_equal(out[k].cpu().numpy(), alone[k].cpu().numpy())
            assert (out["indirect_specular"] > 0).float().mean() > 0.5
            if name == "ggx_node":
                assert (out["refraction"] > 0).float().mean() > 0.5
        return got
    finally:
        ctx.close()


@pytest.mark.parametrize("n,spp_n", [(4096, 4), (777, 3)])
def test_node_section_of_the_example_matches_the_python_path(n, spp_n):
    from rlshaders_amd import build
    exe = build.build_trace_example()
    p = subprocess.run([str(exe), str(n), str(spp_n)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["points"] == n and got["spp_n"] == spp_n
    want = _python_path(n, spp_n)
    for name, queues in (("ggx_node", 4), ("disney_node", 3)):
        assert len(got[name]["rays"]) == queues and all(r > 0 for r in got[name]["rays"])
        assert 0 < got[name]["blocked"] < got[name]["rays"][0]
        for key in ("rays", "blocked", "aovs", "out"):
            assert got[name][key] == want[name][key], (name, key)
        assert got[name]["mean_out"] > 0
