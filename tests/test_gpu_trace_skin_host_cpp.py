"""GPU: the C++ mirror of the caller-traced rlSkin node (rlshaders_amd/host/rls_trace.hpp: SkinNodeQueues, emitNode,
resolveNode) end to end.  host/example_trace.cpp emits the node's five queues under two unoccluded lights, puts the radiance
(0.7, 0.8, 0.9) on every glossy ray, walks the probe rays through each point's tangent plane on the host (E = 1 / pi) and
resolves; the ray counts, the hits found and the bits of the AOVs, of sg->out.RGB and of the three hand-down scalars equal the
Python path (rlshaders_amd/trace.py, skin_node_rays) on the same inputs."""
import json
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_trace_lights_host_cpp import LIGHTS, SEED
from test_gpu_trace_sss_host_cpp import INV_PI, _fnv

pytestmark = pytest.mark.gpu

SKIN = dict(sss_color=(0.8, 0.5, 0.3), sss_weight=0.9, sss_dist_multiplier=0.5, sss_scatter_dist=(0.1, 0.2, 0.4),
            specular_color=(0.9, 0.95, 1.0), specular_weight=0.6, specular_roughness=0.5, specular_ior=1.44,
            sheen_color=(1.0, 0.9, 0.8), sheen_weight=0.3, sheen_roughness=0.35, sheen_ior=1.3)
ENV = (0.7, 0.8, 0.9)


def _python_path(n, spp_n):
    import rlshaders_amd as R
    from rlshaders_amd import trace as T
    from rlshaders_amd.closures import make_light
    f = np.float32
    ctx = R.Context(0)
    try:
        wo, N, Tn = R.gen_frame(ctx, SEED, 0, n)
        lights = [make_light(**kw) for kw in LIGHTS]
        P = torch.zeros(3, n, device=ctx.torch_device)
        sk = R.SkinShader(ctx, wo, N, Tn, **SKIN)
        q = T.skin_node_rays(sk, P, lights, spp_n, SEED)
        cnt = q.counts()
        spp = spp_n * spp_n
        ones = lambda k: torch.ones(3, max(cnt[k], 1), device=ctx.torch_device)
        env = torch.tensor(ENV, device=ctx.torch_device)[:, None]
        org, d, md = (t.cpu().numpy() for t in (q.probes.origin, q.probes.dir, q.probes.maxdist))
        nrm = np.repeat(N.cpu().numpy(), spp, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            dn = ((nrm[0] * d[0]).astype(f) + nrm[1] * d[1]).astype(f) + nrm[2] * d[2]
            on = ((nrm[0] * org[0]).astype(f) + nrm[1] * org[1]).astype(f) + nrm[2] * org[2]
            t = np.where(dn != 0, (-on / dn).astype(f), f(0)).astype(f)
        ok = (t > 0) & (t <= md)
        hP = np.where(ok, (org + d * t).astype(f), f(0))[:, None, :].astype(f)
        hN = np.where(ok, nrm, f(0))[:, None, :].astype(f)
        E = np.where(ok, INV_PI, f(0))[None, None, :].repeat(3, axis=0).astype(f)
        dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        out = q.resolve(ones("sheen_shadow"), ones("specular_shadow"), (ones("sheen_glossy") * env).contiguous(),
                        (ones("specular_glossy") * env).contiguous(), dv(ok.astype(np.uint8)), dv(hP), dv(hN), dv(E),
                        use_cavity_fade=True)
        aovs = np.concatenate([out[k].cpu().numpy() for k in ("sheen", "specular", "sss")])
        scal = np.stack([out[k].cpu().numpy() for k in ("sheenFresnel", "specularFresnel", "sssWeight")])
        assert (out["sss"] > 0).float().mean() > 0.5 and (out["sheen"] > 0).float().mean() > 0.5
        return {"rays": [cnt["sheen_shadow"], cnt["specular_shadow"], cnt["sheen_glossy"], cnt["specular_glossy"], n * spp],
                "hits": int(ok.sum()), "aovs": _fnv(aovs), "out": _fnv(out["out"].cpu().numpy()), "scalars": _fnv(scal)}
    finally:
        ctx.close()


@pytest.mark.parametrize("n,spp_n", [(4096, 4), (777, 3)])
def test_skin_section_of_the_example_matches_the_python_path(n, spp_n):
    from rlshaders_amd import build
    exe = build.build_trace_example()
    p = subprocess.run([str(exe), str(n), str(spp_n)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])["skin_node"]
    want = _python_path(n, spp_n)
    assert all(r > 0 for r in got["rays"]) and 0 < got["hits"] < got["rays"][4]
    for key in ("rays", "hits", "aovs", "out", "scalars"):
        assert got[key] == want[key], key
    assert got["mean_out"] > 0
