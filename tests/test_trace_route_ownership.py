"""CPU: rlsb::HitRoutes (host/rls_trace.hpp) gives back every device allocation, also when one of them fails.

tests/native/trace_route_ownership.cpp is built as an integrator builds against the header (g++ -std=c++14 -Wall) but links
neither library (tests/test_trace_host_ownership.py): it constructs HitRoutes with and without slot, for 5 rays and for none:
once unhindered -- N allocations (offsets, order, the scratch; slot one more), none live after destruction -- and once per k in
1..N with the k-th allocation failing -- an rlsb::Error, none live."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "native" / "trace_route_ownership.cpp"


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = tmp_path_factory.mktemp("trace_route_ownership") / "trace_route_ownership"
    cmd = ["g++", "-std=c++14", "-Wall", f"-I{ROOT / 'include'}", f"-I{ROOT / 'rlshaders_amd' / 'host'}", str(DRIVER),
           "-o", str(exe)]
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


def test_the_allocations_of_every_form(rows):
    assert set(rows) == {f"HitRoutes rays {r} slot {s}" for r in (5, 0) for s in (0, 1)}
    for r in (5, 0):
        assert rows[f"HitRoutes rays {r} slot 0"]["n"] == 3 and rows[f"HitRoutes rays {r} slot 1"]["n"] == 4


def test_nothing_is_live_after_destruction(rows):
    assert {k: r["live"] for k, r in rows.items() if r["live"]} == {}


def test_a_failing_allocation_throws_and_leaves_nothing_live(rows):
    assert {k: r["silent"] for k, r in rows.items() if r["silent"]} == {}
    assert {k: r["leaked"] for k, r in rows.items() if r["leaked"]} == {}
