"""GPU: the C++ mirror of the caller-traced rlSss integrator (rlshaders_amd/host/rls_trace.hpp, emitProbes / resolveScatter)
end to end -- emit the probe rays, walk them through each point's tangent plane on the host, resolve -- gives the same
resolved bits as the Python path (rlshaders_amd.trace.sss_probe_rays) on the same inputs, and the same result as
rls_sss_integrate_scatter where the tangent planes are one plane."""
import json
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 1234          # example_trace.cpp, kSeed
INV_PI = np.float32(0.318309886)


def _fnv(planes: np.ndarray) -> str:
    h = 1469598103934665603
    for byte in np.ascontiguousarray(planes, dtype=np.float32).tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _python_path(n, spp_n):
    """example_trace.cpp's rlSss section through rlshaders_amd.trace: the same closure, P = 0, the same host walk"""
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
        hP = np.where(ok, (org + d * t).astype(f), f(0))[:, None, :].astype(f)
        hN = np.where(ok, nrm, f(0))[:, None, :].astype(f)
        E = np.where(ok, INV_PI, f(0))[None, None, :].repeat(3, axis=0).astype(f)
        dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        res, depth = q.resolve(dv(ok.astype(np.uint8)), dv(hP), dv(hN), dv(E), use_cavity_fade=True, want_depth=True)
        res, depth = res.cpu().numpy(), depth.cpu().numpy()
        return {"rays": q.count, "checksum": _fnv(res), "mean_depth": float(depth.astype(np.float64).mean())}
    finally:
        ctx.close()


@pytest.mark.parametrize("n,spp_n", [(4096, 4), (777, 3)])
def test_trace_example_sss_matches_the_python_path(n, spp_n):
    from rlshaders_amd import build
    exe = build.build_trace_example()
    p = subprocess.run([str(exe), str(n), str(spp_n)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])["sss"]
    want = _python_path(n, spp_n)
    assert got["rays"] == want["rays"] == n * spp_n * spp_n
    assert got["checksum"] == want["checksum"]
    assert got["mean_depth"] == pytest.approx(want["mean_depth"], rel=1e-7) and 0.3 < got["mean_depth"] <= 0.5
