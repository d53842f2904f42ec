"""GPU: the C++ mirror of the caller-traced integrators (rlshaders_amd/host/rls_trace.hpp) end to end -- emit, a host-side
"tracer" against an analytic sky, resolve -- gives the same ray counts and the same resolved bits as the Python path
(rlshaders_amd/trace.py) on the same inputs."""
import json
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 1234          # example_trace.cpp, kSeed


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
        s = R.GgxSampler(ctx, wo, N, Tn, specColor=(0.9, 0.6, 0.3), roughness=0.4, ior=1.6, anisotropic=0.5)
        got = {}
        for name, emit in (("glossy", T.glossy_rays), ("refract", T.refract_rays)):
            q = emit(s, spp_n, SEED)
            dz = q.dir[2].cpu().numpy()
            up = np.float32(0.25) + np.float32(0.75) * np.maximum(dz, np.float32(0.0))
            L = np.stack([up, up * np.float32(0.875), up * np.float32(0.75)]).astype(np.float32)
            res = q.resolve(torch.from_numpy(L).cuda()).cpu().numpy()
            got[name] = {"rays": q.count, "checksum": _fnv(res)}
        return got
    finally:
        ctx.close()


@pytest.mark.parametrize("n,spp_n", [(4096, 4), (777, 3)])
def test_trace_example_matches_the_python_path(n, spp_n):
    from rlshaders_amd import build
    exe = build.build_trace_example()
    p = subprocess.run([str(exe), str(n), str(spp_n)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["points"] == n and got["spp_n"] == spp_n
    want = _python_path(n, spp_n)
    for name in ("glossy", "refract"):
        assert 0 < got[name]["rays"] <= n * spp_n * spp_n
        assert got[name]["rays"] == want[name]["rays"], name
        assert got[name]["checksum"] == want[name]["checksum"], name
