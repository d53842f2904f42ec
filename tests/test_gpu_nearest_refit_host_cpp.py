"""GPU: the C++ mirror of the refit (rlshaders_amd/host/rls_nearest_refit.hpp, rlsb::NearestRefit) end to end --
example_nearest_refit squashes and moves example_nearest's sphere over three frames, refits the one scene to each frame's device
vertices and normals, walks the light loop's shadow rays and rlSss's probe rays through it, and does the same on a fresh
rlsb::NearestScene per frame: the two sets of checksums must agree frame by frame, and the frames must differ from each other."""
import json
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_refit_example_matches_a_fresh_scene_every_frame():
    from rlshaders_amd import build
    exe = build.OBJDIR / "example_nearest_refit"
    assert exe.exists(), f"{exe}: build it with rlshaders_amd.build.build_nearest_refit_example()"
    n, spp_n = 700, 2
    p = subprocess.run([str(exe), str(n), str(spp_n), "8"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["points"] == n and got["triangles"] == 8 * 4 ** 3 + 2 and got["updates"] == 3 and got["levels"] >= 8
    frames = got["frames"]
    assert [f["frame"] for f in frames] == [0, 1, 2]
    for f in frames:
        assert f["refit"] == f["fresh"], f
        assert f["refit"]["rays"] > n and len(f["refit"]["steps"]) >= 2 and f["refit"]["black"] > 0
        assert f["refit"]["probes"]["hits"] > n and len(f["refit"]["probes"]["steps"]) >= 2
    # the sphere moved: what the rays meet changes from frame to frame
    for key in ("visibility", "direct_diffuse"):
        assert len({f["refit"][key] for f in frames}) == 3, key
    assert len({f["refit"]["probes"]["P"] for f in frames}) == 3
