"""GPU: the C++ mirror of the probe walk (rlshaders_amd/host/rls_walk.hpp, rlsb::ProbeWalk) end to end -- example_walk emits
rlSss's probe rays on a sphere, walks them over a host closest-hit function, resolves -- prints the per-step ray counts and the
checksums the Python path (rlshaders_amd.walk.ProbeWalk) gives on the same inputs with the same tracer restated in numpy."""
import json
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 1234          # example_walk.cpp, kSeed
RADIUS = np.float32(0.5)
INV_PI = np.float32(0.318309886)


def _fnv(data: bytes) -> str:
    h = 1469598103934665603
    for byte in data:
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def closest_hit(o, d, maxdist):
    """example_walk.cpp's closestHit in float32, the same operations in the same order -> t, 0 for no hit"""
    f = np.float32
    with np.errstate(all="ignore"):
        a = ((d[0] * d[0] + d[1] * d[1]).astype(f) + d[2] * d[2]).astype(f)
        b = ((o[0] * d[0] + o[1] * d[1]).astype(f) + o[2] * d[2]).astype(f)
        c = (((o[0] * o[0] + o[1] * o[1]).astype(f) + o[2] * o[2]).astype(f) - RADIUS * RADIUS).astype(f)
        disc = ((b * b).astype(f) - (a * c).astype(f)).astype(f)
        sq = np.sqrt(disc).astype(f)
        t0, t1 = ((-b - sq).astype(f) / a).astype(f), ((-b + sq).astype(f) / a).astype(f)
        t = np.where(t0 > 0, t0, t1)
        ok = (disc >= 0) & (a != 0) & (t > 0) & (t <= maxdist)
    return np.where(ok, t, f(0)).astype(f)


def _python_path(n, spp_n):
    import rlshaders_amd as R
    from rlshaders_amd import trace as T, walk as W
    f = np.float32
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ctx = R.Context(0)
    try:
        _, N, Tn = R.gen_frame(ctx, SEED, 0, n)
        s = R.SssSampler(ctx, N, Tn, (0.8, 0.5, 0.3), (0.05, 0.1, 0.2))
        P = dv((RADIUS * N.cpu().numpy()).astype(f))
        q = T.sss_probe_rays(s, P, spp_n, SEED)
        w = W.ProbeWalk(ctx, q, P)
        steps = []
        while True:
            m = w.active
            if m == 0:
                break
            steps.append(m)
            r = w.rays
            o, d, md = r.origin[:, :m].cpu().numpy(), r.dir[:, :m].cpu().numpy(), r.maxdist[:m].cpu().numpy()
            t = closest_hit(o, d, md)
            hp = (o + (d * t).astype(f)).astype(f)
            nrm = (hp / RADIUS).astype(f)
            w.step(W.Found(dv((t != 0).astype(np.uint8)), dv(t), dv(hp), dv(nrm), dv(nrm)), bound=m)
        cnt, hP, hN, _ = w.hits()
        E = torch.full((3, w.max_hits, q.count), float(INV_PI), device="cuda")
        res, depth = q.resolve(cnt, hP, hN, E, want_depth=True)
        cnt = cnt.cpu().numpy()
        return {"rays": q.count, "steps": steps, "hits": int(cnt.sum()), "count_checksum": _fnv(cnt.tobytes()),
                "checksum": _fnv(res.cpu().numpy().astype(f).tobytes()),
                "mean_depth": float(depth.cpu().numpy().astype(np.float64).mean())}
    finally:
        ctx.close()


@pytest.mark.parametrize("n,spp_n", [(1000, 2), (333, 3)])
def test_walk_example_matches_the_python_path(n, spp_n):
    from rlshaders_amd import build
    exe = build.build_walk_example()
    p = subprocess.run([str(exe), str(n), str(spp_n)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    want = _python_path(n, spp_n)
    assert got["rays"] == want["rays"] == n * spp_n * spp_n
    assert got["steps"] == want["steps"] and 2 <= len(got["steps"]) <= 12
    assert got["hits"] == want["hits"] > 0 and got["count_checksum"] == want["count_checksum"]
    assert got["checksum"] == want["checksum"]
    assert got["mean_depth"] == pytest.approx(want["mean_depth"], rel=1e-7) and got["mean_depth"] > 0.2
