"""GPU: the C++ mirror of the secondary-ray calls (rlshaders_amd/host/rls_trace.hpp: RayState, emitBounce, resolveBounce,
advanceState) end to end.  host/example_trace_bounce.cpp shades the camera hits of an rlGgx surface, advances the state along
the glossy queue and shades stand-in hits of those rays as glossy secondary rlGgx and rlDisney points; the ray counts per queue
and the bits of the advanced state, the AOVs and sg->out.RGB equal the Python path (rlshaders_amd/trace.py) on the same
inputs."""
import json
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_trace_host_cpp import _fnv
from test_gpu_trace_lights_host_cpp import LIGHTS, SEED
from test_gpu_trace_shade_host_cpp import SHADER, _sky

pytestmark = pytest.mark.gpu

DEPTHS = dict(total=4, diffuse=1, glossy=1, refraction=2)


def _fnv_bytes(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


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

        def shade(nq, s):
            vis = torch.ones(3, max(nq.shadow.count, 1), device=ctx.torch_device)
            out = nq.resolve(vis, *[_sky(getattr(nq, r)) for r in nq.RAYS])
            aovs = np.concatenate([out[k].cpu().numpy() for k in s.SHADE_AOVS])
            return {"points": s.n, "rays": [nq.shadow.count] + [getattr(nq, r).count for r in nq.RAYS], "aovs": _fnv(aovs),
                    "out": _fnv(out["out"].cpu().numpy())}, out

        got = {}
        camera = T.RayState.camera(ctx, n)
        nq = T.ggx_bounce_rays(g, T.ggx_shader(g, **SHADER), P, lights, spp_n, SEED, camera, DEPTHS)
        got["camera"], out = shade(nq, g)
        assert (out["indirect_specular"] > 0).float().mean() > 0.5
        hits = T.advance_state(ctx, nq.glossy, camera, T.RLS_RT_GLOSSY)
        state = np.stack([getattr(hits, k).cpu().numpy() for k in T.RayState.PLANES])
        got["advanced"] = {"rays": nq.glossy.count, "state": _fnv_bytes(state)}
        assert (state[0] == T.RLS_RT_GLOSSY).all() and (state[1] == 1).all() and (state[3] == 1).all() and not state[2].any()
        m = min(nq.glossy.count, n)
        sec = T.RayState(*[getattr(hits, k)[:m].contiguous() for k in T.RayState.PLANES])
        cut = lambda t: t[:, :m].contiguous()
        g2 = R.GgxSampler(ctx, cut(wo), cut(N), cut(Tn), specColor=(0.9, 0.6, 0.3), roughness=0.4, ior=1.6, anisotropic=0.5)
        d2 = R.DisneySampler(ctx, cut(wo), cut(N), cut(Tn), base_color=(0.8, 0.5, 0.3), subsurface=0.1, metallic=0.2, specular=0.5,
                             specular_tint=0.1, roughness=0.35, anisotropic=0.3, sheen=0.2, sheen_tint=0.5, clearcoat=0.3,
                             clearcoat_gloss=0.6)
        q2 = T.ggx_bounce_rays(g2, T.ggx_shader(g2, **SHADER), cut(P), lights, spp_n, SEED, sec, DEPTHS, first_index=n)
        got["glossy_hits"], out = shade(q2, g2)
        # a glossy secondary point: the specular light term is there at Rr_gloss = GI_glossy_depth, no indirect ray leaves it
        assert q2.glossy.count == 0 and q2.diffuse.count == 0 and q2.refract.count > 0
        assert not out["indirect_specular"].any() and not out["indirect_diffuse"].any() and (out["direct_specular"] > 0).any()
        q3 = T.disney_bounce_rays(d2, cut(P), lights, spp_n, SEED, sec, DEPTHS, first_index=n, indirectDiffuseScale=0.5,
                                  indirectSpecularScale=0.25)
        got["disney_glossy_hits"], out = shade(q3, d2)
        assert q3.diffuse.count == 0 and q3.specular.count == 0
        return got
    finally:
        ctx.close()


@pytest.mark.parametrize("n,spp_n", [(4096, 4), (777, 3)])
def test_the_bounce_example_matches_the_python_path(n, spp_n):
    from rlshaders_amd import build
    exe = build.build_trace_example(name="example_trace_bounce")
    p = subprocess.run([str(exe), str(n), str(spp_n)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["points"] == n and got["spp_n"] == spp_n
    want = _python_path(n, spp_n)
    assert got["advanced"] == want["advanced"] and got["advanced"]["rays"] > n
    for name in ("camera", "glossy_hits", "disney_glossy_hits"):
        for key in ("points", "rays", "aovs", "out"):
            assert got[name][key] == want[name][key], (name, key, got[name], want[name])
        assert got[name]["rays"][0] > 0 and got[name]["mean_out"] > 0
