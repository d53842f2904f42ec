"""GPU: the C++ mirror of the caller-traced shading of rlSss's probe hits (rlshaders_amd/host/rls_trace.hpp, HitQueues /
emitHits / resolveHits) end to end in example_trace.cpp -- the probe hits of each point's tangent plane lit by one spherical
light at visibility 1 and by the sky along the diffuse rays, then the scatter resolve on the E planes -- gives the same counts
and the same bits as the Python path (rlshaders_amd.trace.sss_hit_rays) on the same inputs."""
import json
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_trace_sss_host_cpp import SEED, _fnv

pytestmark = pytest.mark.gpu


def _python_path(n, spp_n):
    """example_trace.cpp's lit-hits section through rlshaders_amd.trace: the same closure, P = 0, the same host walk, light
    and sky"""
    import rlshaders_amd as R
    from rlshaders_amd import trace as T
    f = np.float32
    ctx = R.Context(0)
    try:
        _, N, Tn = R.gen_frame(ctx, SEED, 0, n)
        s = R.SssSampler(ctx, N, Tn, (0.8, 0.5, 0.3), (0.05, 0.1, 0.2))
        P = torch.zeros(3, n, device="cuda")
        q = T.sss_probe_rays(s, P, spp_n, SEED)
        spp = spp_n * spp_n
        org, d, md = (t.cpu().numpy() for t in (q.origin, q.dir, q.maxdist))
        nrm = np.repeat(N.cpu().numpy(), spp, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            dn = ((nrm[0] * d[0]).astype(f) + nrm[1] * d[1]).astype(f) + nrm[2] * d[2]
            on = ((nrm[0] * org[0]).astype(f) + nrm[1] * org[1]).astype(f) + nrm[2] * org[2]
            t = np.where(dn != 0, (-on / dn).astype(f), f(0)).astype(f)
        ok = (t > 0) & (t <= md)
        dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        cnt = dv(ok.astype(np.uint8))
        hP = dv(np.where(ok, (org + d * t).astype(f), f(0))[:, None, :].astype(f))
        hN = dv(np.where(ok, nrm, f(0))[:, None, :].astype(f))
        light = R.make_light(center=(1.5, 2.5, 3.5), radius=1.25, radiance=(3.0, 2.0, 0.5))
        hq = T.sss_hit_rays(s, P, q, cnt, hP, hN, light, 2, SEED, use_cavity_fade=True, trace_diffuse=True)
        dz = hq.diffuse["dir"][2].cpu().numpy()
        up = (f(0.25) + f(0.75) * np.maximum(dz, f(0))).astype(f)
        L = np.zeros((3, n * spp), f)
        L[0, :dz.size], L[1, :dz.size], L[2, :dz.size] = up, (up * f(0.875)).astype(f), (up * f(0.75)).astype(f)
        vis = torch.ones(3, max(hq.shadow_capacity, 1), device="cuda")
        E = hq.resolve(vis, dv(L))
        res = q.resolve(cnt, hP, hN, E, use_cavity_fade=True)
        return {"hits": hq.listed, "shadow_rays": hq.shadow_count, "diffuse_rays": hq.diffuse_count,
                "E_checksum": _fnv(E.cpu().numpy()), "checksum": _fnv(res.cpu().numpy()),
                "mean": float(res.cpu().numpy().astype(np.float64).mean())}
    finally:
        ctx.close()


@pytest.mark.parametrize("n,spp_n", [(777, 3)])
def test_trace_example_lit_hits_match_the_python_path(n, spp_n):
    from rlshaders_amd import build
    exe = build.build_trace_example()
    p = subprocess.run([str(exe), str(n), str(spp_n)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])["sss_hits"]
    want = _python_path(n, spp_n)
    for k in ("hits", "shadow_rays", "diffuse_rays", "E_checksum", "checksum"):
        assert got[k] == want[k], k
    assert got["hits"] > n and got["shadow_rays"] > 0 and got["diffuse_rays"] > 0
    assert got["mean"] == pytest.approx(want["mean"], rel=1e-6) and got["mean"] > 0
