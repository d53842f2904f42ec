"""GPU: the C++ mirror of the shadow walk (rlshaders_amd/host/rls_shadow_walk.hpp, rlsb::ShadowWalk) end to end --
example_shadow_walk emits rlGgx's light-loop shadow rays, walks them under three tinted slabs and an opaque sphere over a host
closest-hit function, resolves with resolveDirect -- prints the per-step ray counts, the black rays and the checksums the Python
path (rlshaders_amd.shadow_walk.ShadowWalk) gives on the same inputs with the same tracer restated in numpy."""
import json
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_trace_host_cpp import _fnv
from test_gpu_trace_lights_host_cpp import LIGHTS, SEED, SHADER

pytestmark = pytest.mark.gpu

F = np.float32
SLAB_Z = np.array([0.5, 0.8, 1.1], F)                             # example_shadow_walk.cpp: kSlabZ, kSlabKt, kCenter, kRadius, kTMin
SLAB_KT = np.array([[0.2, 0.9, 0.7], [0.8, 0.4, 0.6], [0.5, 0.5, 1.0]], F)
CENTER, RADIUS, TMIN = np.array([-1.63, 0.82, 1.23], F), F(0.25), F(1e-3)


def closest_hit(o, d, maxdist):
    """example_shadow_walk.cpp's closestHit in float32, the same operations in the same order -> (surface, -1 for none; t)"""
    m = o.shape[1]
    surface, t = np.full(m, -1, np.int64), np.zeros(m, F)
    with np.errstate(all="ignore"):
        for k in range(3):
            tk = ((SLAB_Z[k] - o[2]).astype(F) / d[2]).astype(F)
            ok = (d[2] != 0) & (tk > TMIN) & (tk <= maxdist) & ((surface < 0) | (tk < t))
            surface, t = np.where(ok, k, surface), np.where(ok, tk, t).astype(F)
        oc = (o - CENTER[:, None]).astype(F)
        b = ((oc[0] * d[0] + oc[1] * d[1]).astype(F) + oc[2] * d[2]).astype(F)
        c = (((oc[0] * oc[0] + oc[1] * oc[1]).astype(F) + oc[2] * oc[2]).astype(F) - RADIUS * RADIUS).astype(F)
        disc = ((b * b).astype(F) - c).astype(F)
        sq = np.sqrt(disc).astype(F)
        t0, t1 = (-b - sq).astype(F), (-b + sq).astype(F)
        ts = np.where(t0 > TMIN, t0, t1).astype(F)
        ok = (disc >= 0) & (ts > TMIN) & (ts <= maxdist) & ((surface < 0) | (ts < t))
        surface, t = np.where(ok, 3, surface), np.where(ok, ts, t).astype(F)
    return surface, t


def _python_path(n, spp_n, max_steps):
    import rlshaders_amd as R
    from rlshaders_amd import shadow_walk as W, trace as T
    from rlshaders_amd.closures import make_light
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ctx = R.Context(0)
    try:
        wo, N, Tn = R.gen_frame(ctx, SEED, 0, n)
        lights = [make_light(**kw) for kw in LIGHTS]
        P = torch.zeros(3, n, device=ctx.torch_device)
        g = R.GgxSampler(ctx, wo, N, Tn, specColor=(0.9, 0.6, 0.3), roughness=0.4, ior=1.6, anisotropic=0.5)
        q = T.ggx_shadow_rays(g, T.ggx_shader(g, **SHADER), P, lights, spp_n, SEED)
        shadow = torch.full((4,), T.RLS_RT_SHADOW, dtype=torch.uint8, device=ctx.torch_device)
        kt = dv(np.concatenate([SLAB_KT.T, np.ones((3, 1), F)], axis=1))
        table = T.ggx_opacity(ctx, 4, KtColor=kt, Kt=dv(np.array([0.5, 0.5, 0.5, 0.0], F)), ray_type=shadow)
        w = W.ShadowWalk(ctx, q, P, max_steps=max_steps)
        steps = []
        while True:
            m = w.active
            if m == 0:
                break
            steps.append(m)
            r = w.rays
            o, d, md = r.origin[:, :m].cpu().numpy(), r.dir[:, :m].cpu().numpy(), r.maxdist[:m].cpu().numpy()
            surface, t = closest_hit(o, d, md)
            hit = surface >= 0
            hp = np.where(hit, (o + (d * t).astype(F)).astype(F), F(0)).astype(F)
            w.step(W.Found(dv(hit.astype(np.uint8)), dv(t), dv(hp), table, index=dv(np.where(hit, surface, 0).astype(np.int32))),
                   bound=m)
        rays = q.count
        dd, ds = q.resolve(w.visibility)
        vis = w.visibility[:, :rays].cpu().numpy()
        return {"rays": rays, "steps": steps, "black": int((vis == 0).all(axis=0).sum()), "visibility": _fnv(vis),
                "direct_diffuse": _fnv(dd.cpu().numpy()), "direct_specular": _fnv(ds.cpu().numpy())}
    finally:
        ctx.close()


@pytest.mark.parametrize("n,spp_n,max_steps", [(1000, 2, 8), (333, 3, 2)])
def test_shadow_walk_example_matches_the_python_path(n, spp_n, max_steps):
    from rlshaders_amd import build
    exe = build.build_shadow_walk_example()
    p = subprocess.run([str(exe), str(n), str(spp_n), str(max_steps)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    want = _python_path(n, spp_n, max_steps)
    assert got["points"] == n and got["spp_n"] == spp_n and got["rays"] == want["rays"] > n
    assert got["steps"] == want["steps"] and 2 <= len(got["steps"]) <= max_steps
    assert got["black"] == want["black"] and (got["black"] > 0 or max_steps < 4)
    for key in ("visibility", "direct_diffuse", "direct_specular"):
        assert got[key] == want[key], (key, got, want)
    assert 0.0 < got["mean_visibility"] < 1.0
