"""GPU: the C++ mirror of the rlSkin bounce calls (rlshaders_amd/host/rls_trace.hpp: SkinBounceQueues, emitBounce, resolveBounce,
RayState, advanceState) end to end.  host/example_trace_skin_bounce.cpp shades a camera wave of skin points under two unoccluded
lights, the radiance (0.7, 0.8, 0.9) on every glossy ray and a host walk of the probe rays through each point's tangent plane
(E = 1 / pi), advances the state along the specular lobe's glossy queue with RLS_RT_GLOSSY and shades the first min(rays, points)
of those hits as a second wave; per wave the ray counts, the hits found and the bits of the AOVs, of sg->out.RGB and of the
three hand-down scalars, and the advanced state's bytes, equal the Python path (rlshaders_amd/trace.py, skin_bounce_rays,
advance_state) on the same inputs."""
import json
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_trace_lights_host_cpp import LIGHTS, SEED
from test_gpu_trace_skin_host_cpp import ENV, SKIN
from test_gpu_trace_sss_host_cpp import INV_PI, _fnv

pytestmark = pytest.mark.gpu

DEPTHS = (4, 1, 1, 2)        # example_trace_skin_bounce.cpp: one glossy bounce is allowed


def _wave(T, ctx, sk, N, P, lights, m, spp_n, state, first):
    f = np.float32
    q = T.skin_bounce_rays(sk, P, lights, spp_n, SEED, state, DEPTHS, first)
    cnt = q.counts()
    spp = spp_n * spp_n
    ones = lambda k: torch.ones(3, max(cnt[k], 1), device=ctx.torch_device)
    env = torch.tensor(ENV, device=ctx.torch_device)[:, None]
    org, d, md = (t.cpu().numpy() for t in (q.probes.origin, q.probes.dir, q.probes.maxdist))
    nrm = np.repeat(N.cpu().numpy()[:, :m], spp, axis=1)
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
                    diffuse_visibility=ones("diffuse_shadow"), use_cavity_fade=True)
    aovs = np.concatenate([out[k].cpu().numpy() for k in ("sheen", "specular", "sss")])
    scal = np.stack([out[k].cpu().numpy() for k in ("sheenFresnel", "specularFresnel", "sssWeight")])
    rec = {"points": m, "rays": [cnt[k] for k in ("sheen_shadow", "specular_shadow", "sheen_glossy", "specular_glossy", "diffuse_shadow")],
           "hits": int(ok.sum()), "aovs": _fnv(aovs), "out": _fnv(out["out"].cpu().numpy()), "scalars": _fnv(scal)}
    return q, rec, out


def _python_path(n, spp_n):
    import rlshaders_amd as R
    from rlshaders_amd import trace as T
    from rlshaders_amd.closures import make_light
    ctx = R.Context(0)
    try:
        wo, N, Tn = R.gen_frame(ctx, SEED, 0, n)
        lights = [make_light(**kw) for kw in LIGHTS]
        P = torch.zeros(3, n, device=ctx.torch_device)
        camera = T.RayState.camera(ctx, n)
        q, cam, out = _wave(T, ctx, R.SkinShader(ctx, wo, N, Tn, **SKIN), N, P, lights, n, spp_n, camera, 0)
        assert (out["sss"] > 0).float().mean() > 0.5 and (out["sheen"] > 0).float().mean() > 0.5
        glossy = q.specular_glossy.count
        child = T.advance_state(ctx, q.specular_glossy, camera, T.RLS_RT_GLOSSY)
        state = np.concatenate([getattr(child, k).cpu().numpy() for k in T.RayState.PLANES])
        m = min(glossy, n)
        second = T.RayState(*[getattr(child, k)[:m].contiguous() for k in T.RayState.PLANES])
        sk = R.SkinShader(ctx, wo[:, :m].contiguous(), N[:, :m].contiguous(), Tn[:, :m].contiguous(), **SKIN)
        q2, hits, out2 = _wave(T, ctx, sk, N, P[:, :m].contiguous(), lights, m, spp_n, second, n)
        # the second wave's points are glossy rays at Rr = 1: no glossy ray leaves them, and the hand-down moves
        assert hits["rays"][2] == 0 and hits["rays"][3] == 0 and hits["rays"][4] == 0 and hits["rays"][0] > 0
        assert not torch.equal(out2["specularFresnel"], out["specularFresnel"][:m])
        return {"camera": cam, "advanced": {"rays": glossy, "state": "%016x" % _fnv_bytes(state)}, "glossy_hits": hits}
    finally:
        ctx.close()


def _fnv_bytes(a):
    h = 1469598103934665603
    for v in np.ascontiguousarray(a, dtype=np.uint8).tobytes():
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("n,spp_n", [(1024, 3), (333, 2)])
def test_both_waves_of_the_example_match_the_python_path(n, spp_n):
    from rlshaders_amd import build
    exe = build.build_trace_example(name="example_trace_skin_bounce")
    p = subprocess.run([str(exe), str(n), str(spp_n)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    want = _python_path(n, spp_n)
    assert got["advanced"] == want["advanced"]
    for wave in ("camera", "glossy_hits"):
        assert all(r > 0 for r in got[wave]["rays"][:2]) and 0 < got[wave]["hits"] < got[wave]["points"] * spp_n * spp_n
        for key in ("points", "rays", "hits", "aovs", "out", "scalars"):
            assert got[wave][key] == want[wave][key], (wave, key)
        assert got[wave]["mean_out"] > 0
