"""-m gpu: rlshaders_amd/host/example_nearest_any.cpp (rlsb::NearestAny over rlsb::NearestScene and rlsb::ShadowWalk) -- a light
loop's shadow queue under an opaque occluder answered in one launch and resolved, beside the full walk with an all-ones table; and
under the mixed table through the two-phase route beside the full walk.  The program's own checks pass and its counts add up."""
import json
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_example_answers_the_shadow_queue_in_one_launch():
    from rlshaders_amd import build
    exe = build.OBJDIR / "example_nearest_any"
    assert exe.exists(), f"{exe}: build it with rlshaders_amd.build.build_nearest_any_example()"
    p = subprocess.run([str(exe), "1024", "2", "8"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["ok"] is True and r["triangles"] == 514 and r["rays"] > 0
    o, m = r["opaque"], r["mixed"]
    # every triangle opaque: no ray is veiled, the launch's visibility and AOVs are the full walk's
    assert o["veiled"] == 0 and o["differ"] == 0 and 0 < o["blocked"] and o["clear"] + o["blocked"] == r["rays"]
    assert o["visibility"] == o["walk_visibility"]
    assert o["direct_diffuse"] == o["walk_direct_diffuse"] and o["direct_specular"] == o["walk_direct_specular"]
    # the mixed table: the quad veils, the sphere blocks; only the veiled rays are walked, the full walk lists every ray in reach
    assert m["clear"] + m["blocked"] + m["veiled"] == r["rays"] and m["blocked"] > 0 and m["veiled"] > 0
    assert m["walked"] == m["veiled"] < m["walk_listed"] <= r["rays"]
    assert m["differ"] == 0 and m["blocked_not_zero"] == 0 and m["walk_blocked_not_zero"] * 100 <= m["blocked"]
    assert m["blocked"] <= o["blocked"] and m["blocked"] + m["veiled"] == o["blocked"]                # the same candidates, classed anew
