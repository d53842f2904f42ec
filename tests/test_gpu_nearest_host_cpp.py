"""GPU: the C++ mirror of the nearest-hit queries (rlshaders_amd/host/rls_nearest.hpp, rlsb::NearestScene / NearestFound) end to
end -- example_nearest emits rlGgx's light-loop shadow rays, walks them under a tinted quad and an opaque tessellated sphere with
the device's nearest hits and no host tracer, resolves with resolveDirect -- prints the per-step ray counts, the black rays and
the checksums the Python path (rlshaders_amd.nearest.tracer under shadow_walk.run) gives on the same mesh, built here by the same
operations; then it walks rlSss's probe rays of points on the sphere through the same scene (rlsb::ProbeWalk over
NearestFound::walkFound) and prints the steps, the hit counts and checksums of the stored hits' P and N, which must be those of
walk.run over nearest.tracer: the sphere carries per-vertex normals, so an N / Ns mix-up in the hand-over would show."""
import json
import math
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_trace_host_cpp import _fnv
from test_gpu_trace_lights_host_cpp import LIGHTS, SEED, SHADER

pytestmark = pytest.mark.gpu

F = np.float32
QUAD_Z, QUAD_HALF, QUAD_KT = 0.8, 10.0, (0.2, 0.9, 0.7)             # example_nearest.cpp: kQuadZ, kQuadHalf, kQuadKt
CENTER, RADIUS, LEVEL = (-1.63, 0.82, 1.23), 0.25, 3                 # kCenter, kRadius, kLevel


def _fnv_bytes(data: bytes) -> str:
    h = 1469598103934665603
    for byte in data:
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def build_mesh():
    """example_nearest.cpp's buildMesh, the same double operations in the same order -> V float32 [nv, 3], T [nt, 3], S [nt], the per-vertex
    normals float32 [nv, 3]"""
    U = [[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]]
    T = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(LEVEL):
        mid, T2 = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x, y, z = U[a][0] + U[b][0], U[a][1] + U[b][1], U[a][2] + U[b][2]
                l = math.sqrt((x * x + y * y) + z * z)
                U.append([x / l, y / l, z / l])
                mid[key] = len(U) - 1
            return mid[key]

        for a, b, c in T:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            T2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        T = T2
    V = [[CENTER[k] + RADIUS * u[k] for k in range(3)] for u in U]
    S = [1] * len(T)
    q = len(V)
    h = QUAD_HALF
    V += [[-h, -h, QUAD_Z], [h, -h, QUAD_Z], [h, h, QUAD_Z], [-h, h, QUAD_Z]]
    T += [(q, q + 1, q + 2), (q, q + 2, q + 3)]
    S += [0, 0]
    normals = np.array([list(u) for u in U] + [[0.0, 0.0, 1.0]] * 4, np.float64).astype(F)
    return np.array(V, np.float64).astype(F), np.array(T, np.uint32), np.array(S, np.uint32), normals


def _python_path(n, spp_n, max_steps):
    import rlshaders_amd as R
    from rlshaders_amd import nearest, shadow_walk as W, trace as T
    from rlshaders_amd.closures import make_light
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ctx = R.Context(0)
    try:
        wo, N, Tn = R.gen_frame(ctx, SEED, 0, n)
        lights = [make_light(**kw) for kw in LIGHTS]
        P = torch.zeros(3, n, device=ctx.torch_device)
        g = R.GgxSampler(ctx, wo, N, Tn, specColor=(0.9, 0.6, 0.3), roughness=0.4, ior=1.6, anisotropic=0.5)
        q = T.ggx_shadow_rays(g, T.ggx_shader(g, **SHADER), P, lights, spp_n, SEED)
        shadow = torch.full((2,), T.RLS_RT_SHADOW, dtype=torch.uint8, device=ctx.torch_device)
        kt = dv(np.array([[QUAD_KT[0], 1.0], [QUAD_KT[1], 1.0], [QUAD_KT[2], 1.0]], F))
        table = T.ggx_opacity(ctx, 2, KtColor=kt, Kt=dv(np.array([0.5, 0.0], F)), ray_type=shadow)
        V, tri, S, normals = build_mesh()
        scene = nearest.Scene(ctx, V, tri, surface=S, normals=normals)
        steps = []

        class counting(nearest.tracer):
            def __call__(self, rays, active):
                steps.append(active)
                return super().__call__(rays, active)

        w = W.run(q, P, counting(scene, opacity=table), max_steps=max_steps)
        rays = q.count
        dd, ds = q.resolve(w.visibility)
        vis = w.visibility[:, :rays].cpu().numpy()
        out = {"rays": rays, "steps": steps, "black": int((vis == 0).all(axis=0).sum()), "visibility": _fnv(vis),
               "direct_diffuse": _fnv(dd.cpu().numpy()), "direct_specular": _fnv(ds.cpu().numpy()),
               "triangles": scene.nt, "nodes": scene.nodes, "depth": scene.depth}
        # the probes of n points on the sphere, where their normals point
        from rlshaders_amd import walk
        s = R.SssSampler(ctx, N, Tn, (0.8, 0.5, 0.3), (0.05, 0.1, 0.2))
        Pp = dv((np.array(CENTER, F)[:, None] + F(RADIUS) * N.cpu().numpy()).astype(F))
        pq = T.sss_probe_rays(s, Pp, spp_n, SEED)
        psteps = []

        class counting_probes(nearest.tracer):
            def __call__(self, rays, active):
                psteps.append(active)
                return super().__call__(rays, active)

        pw = walk.run(pq, Pp, counting_probes(scene))
        cnt = pw.hit_count.cpu().numpy()
        live = np.arange(pw.max_hits)[:, None] < cnt[None, :]
        out["probes"] = {"rays": pq.count, "steps": psteps, "hits": int(cnt.sum()), "count": _fnv_bytes(cnt.tobytes()),
                         "P": _fnv(pw.hit_P.cpu().numpy()[:, live]), "N": _fnv(pw.hit_N.cpu().numpy()[:, live])}
        scene.close()
        return out
    finally:
        ctx.close()


@pytest.mark.parametrize("n,spp_n,max_steps", [(1000, 2, 8), (333, 3, 2)])
def test_nearest_example_matches_the_python_path(n, spp_n, max_steps):
    from rlshaders_amd import build
    exe = build.OBJDIR / "example_nearest"
    assert exe.exists(), f"{exe}: build it with rlshaders_amd.build.build_nearest_example()"
    p = subprocess.run([str(exe), str(n), str(spp_n), str(max_steps)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    want = _python_path(n, spp_n, max_steps)
    assert got["points"] == n and got["spp_n"] == spp_n and got["rays"] == want["rays"] > n
    assert got["triangles"] == want["triangles"] == 8 * 4 ** LEVEL + 2 and got["nodes"] == want["nodes"] and got["depth"] == want["depth"]
    assert got["steps"] == want["steps"] and 2 <= len(got["steps"]) <= max_steps
    assert got["black"] == want["black"] and got["black"] > 0
    for key in ("visibility", "direct_diffuse", "direct_specular"):
        assert got[key] == want[key], (key, got, want)
    assert 0.0 < got["mean_visibility"] < 1.0
    assert got["probes"] == want["probes"], (got["probes"], want["probes"])
    assert got["probes"]["rays"] == n * spp_n * spp_n and len(got["probes"]["steps"]) >= 2 and got["probes"]["hits"] > n
