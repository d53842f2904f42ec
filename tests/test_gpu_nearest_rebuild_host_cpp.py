"""-m gpu: rlshaders_amd/host/example_nearest_rebuild.cpp (rlsb::NearestRebuild over rlsb::NearestScene) -- a sphere twisted by 0,
0.5 and 2 radians, the tree of ONE scene rebuilt on the device each frame; the shadow walk's and the probe walk's checksums on the
rebuilt scene equal those on a fresh scene built from the frame's vertices, and so does the tree (links, leaf order, boxes by
value)."""
import json
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_example_rebuilds_and_matches_a_fresh_scene():
    from rlshaders_amd import build
    exe = build.OBJDIR / "example_nearest_rebuild"
    assert exe.exists(), f"{exe}: build it with rlshaders_amd.build.build_nearest_rebuild_example()"
    p = subprocess.run([str(exe), "1024", "2", "8"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["triangles"] == 514 and r["levels"] >= 8 and r["updates"] == 3 and r["device_bytes"] > 0
    assert [f["radians"] for f in r["frames"]] == [0.0, 0.5, 2.0]
    seen = set()
    for f in r["frames"]:
        assert f["tree"] is True, f["frame"]
        assert f["rebuilt"] == f["fresh"], f["frame"]
        assert f["rebuilt"]["rays"] > 0 and 0 < f["rebuilt"]["black"] < f["rebuilt"]["rays"] and f["rebuilt"]["probes"]["hits"] > 0
        seen.add((f["rebuilt"]["visibility"], f["rebuilt"]["probes"]["P"]))
    assert len(seen) == 3                                            # the frames differ: the sphere did move
