"""-m gpu: rlshaders_amd/host/example_nearest_group.cpp (rlsb::NearestGroup over rlsb::NearestScene) -- three instances of one
sphere, a shadow walk and a routed glossy queue through them, one instance moved by two matrices on the device; the checksums on the
group equal those on a fresh group made with the same matrices before and after the move, and the move changed them."""
import json
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_example_moves_an_instance_and_matches_a_fresh_group():
    from rlshaders_amd import build
    exe = build.OBJDIR / "example_nearest_group"
    assert exe.exists(), f"{exe}: build it with rlshaders_amd.build.build_nearest_group_example()"
    p = subprocess.run([str(exe), "1024", "2", "8"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["ok"] is True and r["triangles"] == 512 and r["instances"] == 3 and r["scenes"] == 1 and r["updates"] == 1
    seen = set()
    for f in r["frames"]:
        g = f["group"]
        assert g == f["fresh"], f["frame"]
        assert g["rays"] > 0 and 0 < g["black"] < g["rays"] and g["tinted"] > 0          # the opaque and the translucent instances
        assert len(g["steps"]) >= 2                                                       # a ray through both translucent ones walks on
        assert g["glossy"]["hits"] > 0 and sum(g["glossy"]["routed"]) + g["glossy"]["missed"] == g["glossy"]["rays"]
        assert sum(g["glossy"]["routed"]) == g["glossy"]["hits"] == sum(g["glossy"]["instances"])
        assert g["glossy"]["routed"][0] == sum(g["glossy"]["instances"][:2]) and g["glossy"]["routed"][1] == g["glossy"]["instances"][2]
        seen.add((g["visibility"], g["glossy"]["found"]))
    assert len(seen) == 2                                            # the move changed both queries
