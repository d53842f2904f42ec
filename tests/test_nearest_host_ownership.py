"""CPU: rlsb::NearestScene and rlsb::NearestFound (host/rls_nearest.hpp) are the single owners of what they hold: they give back
every allocation, also when one of them fails.

tests/native/nearest_ownership.cpp is built as an integrator builds against the header (g++ -std=c++14 -Wall, here with the
address and undefined-behaviour sanitizers: a stand-alone host program) but links no library: it defines rls_device_alloc /
rls_device_free and the scene's create / destroy over the heap, counting live blocks and failing the k-th call.  Every form is
constructed once unhindered -- N allocations, none live after destruction -- and once per k in 1..N with the k-th failing -- an
rlsb::Error, none live (what leaks for real is the sanitizer's to report: the program's blocks are not freed behind its back)."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "native" / "nearest_ownership.cpp"
HEADER = ROOT / "rlshaders_amd" / "host" / "rls_nearest.hpp"


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = tmp_path_factory.mktemp("nearest_ownership") / "nearest_ownership"
    cmd = ["g++", "-std=c++14", "-Wall", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}",
           f"-I{ROOT / 'rlshaders_amd' / 'host'}", str(DRIVER), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    out = {}
    for line in p.stdout.splitlines():
        name, n, live, leaked, silent = line.split("\t")
        out[name] = dict(n=int(n), live=int(live), leaked=[int(k) for k in leaked.split(",") if k],
                         silent=[int(k) for k in silent.split(",") if k])
    return out


def test_every_form_is_constructed(rows):
    want = {"NearestScene": 1, "scene and found": 1 + 2 + 5 * 3 + 1 + 1}
    for r in (20, 0):
        # hit, t; five vectors of three planes; prim, surface, u, v; bin; last
        want[f"NearestFound all rays {r}"] = 2 + 15 + 4 + 1 + 1
        want[f"NearestFound walk rays {r}"] = 2 + 9 + 1 + 1
        want[f"NearestFound shadow rays {r}"] = 2 + 3 + 1 + 1
        want[f"NearestFound bare rays {r}"] = 2
    assert {k: v["n"] for k, v in rows.items()} == want


def test_nothing_is_live_after_destruction(rows):
    assert {k: r["live"] for k, r in rows.items() if r["live"]} == {}


def test_a_failing_allocation_throws_and_leaves_nothing_live(rows):
    assert {k: r["silent"] for k, r in rows.items() if r["silent"]} == {}
    assert {k: r["leaked"] for k, r in rows.items() if r["leaked"]} == {}


def test_one_owner_in_the_header():
    """the found planes go through the class's one DeviceBuffers member, the scene through its one pointer; the header frees and
    allocates nothing by itself, and neither class can be copied"""
    text = HEADER.read_text()
    assert not re.search(r"\brls_device_(alloc|free)\b", text)
    assert text.count("detail::DeviceBuffers bufs_;") == 1 and text.count("rls_nearest_scene_destroy(") == 1
    for cls in ("NearestScene", "NearestFound"):
        assert f"{cls}(const {cls} &) = delete;" in text and f"{cls} &operator=(const {cls} &) = delete;" in text
