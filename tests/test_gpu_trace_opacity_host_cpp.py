"""GPU: the C++ mirror of the shadow rays' hits calls (rlshaders_amd/host/rls_trace.hpp: ggxOpacity, skinOpacity, ShadowHits,
foldVisibility) end to end.  host/example_trace_shadow.cpp emits the shadow rays of rlGgx points under two lights, gives every
ray a hit on a tinted rlGgx sheet and the odd rays a second one on an rlSkin surface through a two-entry table, folds the hits
into the visibility and resolves the light loop under it; the ray count and the bits of the visibility and of both AOVs equal
the Python path (rlshaders_amd/trace.py) on the same inputs."""
import json
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_trace_host_cpp import _fnv
from test_gpu_trace_lights_host_cpp import LIGHTS, SEED, SHADER

pytestmark = pytest.mark.gpu


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
        q = T.ggx_shadow_rays(g, T.ggx_shader(g, **SHADER), P, lights, spp_n, SEED)
        rays = q.count
        shadow = torch.full((1,), T.RLS_RT_SHADOW, dtype=torch.uint8, device=ctx.torch_device)
        table = ctx.empty(3, 2)
        table[:, 0:1] = T.ggx_opacity(ctx, 1, KtColor=(0.2, 0.9, 0.7), Kt=0.5, ray_type=shadow)
        table[:, 1:2] = T.skin_opacity(ctx, 1, opacity=0.75, opacity_color=(0.9, 0.8, 0.6), ray_type=shadow)
        j = torch.arange(rays, device=ctx.torch_device)
        count = (1 + (j & 1)).to(torch.uint8)
        index = torch.stack([torch.zeros_like(j), torch.ones_like(j)]).to(torch.int32).contiguous()      # [max_hits 2, rays]
        vis = T.shadow_visibility(ctx, rays, T.ShadowHits(count, table, 2, index=index))
        dd, ds = q.resolve(vis)
        h = vis.cpu().numpy()
        # even rays cross the sheet alone, odd rays the skin surface too: darker in every channel
        even, odd = h[:, 0::2], h[:, 1::2]
        assert (h > 0).all() and (h < 1).all() and (odd < even[:, :odd.shape[1]]).all()
        return {"rays": rays, "visibility": _fnv(h), "direct_diffuse": _fnv(dd.cpu().numpy()),
                "direct_specular": _fnv(ds.cpu().numpy())}
    finally:
        ctx.close()


@pytest.mark.parametrize("n,spp_n", [(4096, 4), (777, 3)])
def test_the_shadow_example_matches_the_python_path(n, spp_n):
    from rlshaders_amd import build
    exe = build.build_trace_example(name="example_trace_shadow")
    p = subprocess.run([str(exe), str(n), str(spp_n)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["points"] == n and got["spp_n"] == spp_n and got["rays"] > n
    want = _python_path(n, spp_n)
    for key in ("rays", "visibility", "direct_diffuse", "direct_specular"):
        assert got[key] == want[key], (key, got, want)
    assert 0.0 < got["mean_visibility"] < 1.0
    assert np.isfinite(got["mean_visibility"])
