"""GPU: the C++ mirror of the caller-traced light loops (rlshaders_amd/host/rls_trace.hpp: ShadowQueue, emitDirect,
resolveDirect) end to end.  host/example_trace.cpp emits the shadow rays of rlGgx's and rlDisney's light loops under two
lights, shadows the second light with the half-space x > 3 on the host and resolves; the ray counts, the blocked rays and
the bits of both AOVs equal the Python path (rlshaders_amd/trace.py) on the same inputs, and the AOVs equal the analytic call
with the first light alone by value."""
import json
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_trace_host_cpp import _fnv

pytestmark = pytest.mark.gpu

SEED = 1234          # example_trace.cpp, kSeed
LIGHTS = (dict(center=(-4.0, 2.0, 3.0), radius=1.0, radiance=(3.0, 2.0, 1.0)),
          dict(center=(6.0, 1.0, 2.0), radius=1.0, radiance=(1.0, 4.0, 2.0)))
SHADER = dict(KdColor=(0.7, 0.5, 0.2), Kd=0.8, diffuseRoughness=0.3, Ks=0.6)


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
        for name in ("ggx_lights", "disney_lights"):
            if name == "ggx_lights":
                q = T.ggx_shadow_rays(g, T.ggx_shader(g, **SHADER), P, lights, spp_n, SEED)
                alone = g.directLighting(P, lights[0], spp_n, SEED, **SHADER)
            else:
                q = T.disney_shadow_rays(d, P, lights, spp_n, SEED)
                alone = d.directLighting(P, lights[0], spp_n, SEED)
            blocked = (q.maxdist * q.dir[0]) > 3.0
            kind = q.kind.cpu().numpy()
            assert np.array_equal(blocked.cpu().numpy(), (kind & T.RLS_SHADOW_LIGHT_MASK) == 1)
            vis = (~blocked).to(torch.float32)[None, :].repeat(3, 1).contiguous()
            dd, ds = q.resolve(vis)
            got[name] = {"rays": q.count, "blocked": int(blocked.sum().item()), "direct_diffuse": _fnv(dd.cpu().numpy()),
                         "direct_specular": _fnv(ds.cpu().numpy())}
            # the shadowed light adds +0: by value the first light alone
            np.testing.assert_array_equal(dd.cpu().numpy(), alone[0].cpu().numpy())
            np.testing.assert_array_equal(ds.cpu().numpy(), alone[1].cpu().numpy())
        return got
    finally:
        ctx.close()


@pytest.mark.parametrize("n,spp_n", [(4096, 4), (777, 3)])
def test_light_section_of_the_example_matches_the_python_path(n, spp_n):
    from rlshaders_amd import build
    exe = build.build_trace_example()
    p = subprocess.run([str(exe), str(n), str(spp_n)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["points"] == n and got["spp_n"] == spp_n
    want = _python_path(n, spp_n)
    for name in ("ggx_lights", "disney_lights"):
        assert 0 < got[name]["blocked"] < got[name]["rays"] <= n * 2 * 3 * spp_n * spp_n
        for key in ("rays", "blocked", "direct_diffuse", "direct_specular"):
            assert got[name][key] == want[name][key], (name, key)
        assert got[name]["mean_diffuse"] > 0 and got[name]["mean_specular"] > 0
