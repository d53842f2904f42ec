"""GPU: the C++ mirror of the caller-traced rlDisney integrator (rlshaders_amd/host/rls_trace.hpp, emitDisney) end to end --
emit per lobe, a host-side "tracer" against an analytic sky, resolve -- gives the same ray counts and the same resolved bits
as the Python path (rlshaders_amd.trace.disney_rays) on the same inputs."""
import json
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 1234          # example_trace.cpp, kSeed
DIFFUSE, GLOSSY = 0x08, 0x10
# example_trace.cpp: the rlDisney closure's uniform parameters
PARAMS = dict(subsurface=0.1, metallic=0.2, specular=0.5, specular_tint=0.1, roughness=0.35, anisotropic=0.3, sheen=0.2,
              sheen_tint=0.5, clearcoat=0.3, clearcoat_gloss=0.6)


def _fnv(planes: np.ndarray) -> str:
    h = 1469598103934665603
    for byte in np.ascontiguousarray(planes, dtype=np.float32).tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _python_path(n, spp_n):
    import rlshaders_amd as R
    from rlshaders_amd import trace as T
    ctx = R.Context(0)
    try:
        wo, N, Tn = R.gen_frame(ctx, SEED, 0, n)
        s = R.DisneySampler(ctx, wo, N, Tn, base_color=(0.8, 0.5, 0.3), **PARAMS)
        got = {}
        for name, lobe in (("disney_diffuse", DIFFUSE), ("disney_glossy", GLOSSY)):
            q = T.disney_rays(s, lobe, spp_n, SEED)
            dz = q.dir[2].cpu().numpy()
            up = np.float32(0.25) + np.float32(0.75) * np.maximum(dz, np.float32(0.0))
            L = np.stack([up, up * np.float32(0.875), up * np.float32(0.75)]).astype(np.float32)
            res = q.resolve(torch.from_numpy(L).cuda()).cpu().numpy()
            got[name] = {"rays": q.count, "checksum": _fnv(res)}
        return got
    finally:
        ctx.close()


@pytest.mark.parametrize("n,spp_n", [(4096, 4), (777, 3)])
def test_trace_example_disney_matches_the_python_path(n, spp_n):
    from rlshaders_amd import build
    exe = build.build_trace_example()
    p = subprocess.run([str(exe), str(n), str(spp_n)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["points"] == n and got["spp_n"] == spp_n
    want = _python_path(n, spp_n)
    for name in ("disney_diffuse", "disney_glossy"):
        assert 0 < got[name]["rays"] <= n * spp_n * spp_n
        assert got[name]["rays"] == want[name]["rays"], name
        assert got[name]["checksum"] == want[name]["checksum"], name
