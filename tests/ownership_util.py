"""helpers of the host ownership tests (test_*_ownership.py): a program of tests/native/*_ownership.cpp is built as an integrator
builds against the headers (g++ -std=c++14 -Wall; with ``sanitize`` under the address and undefined-behaviour sanitizers: a
stand-alone host program), run, and its rows parsed; and the two tests every such module asks of its rows, which it imports
under their names.  pytest does not collect this module."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOST = ROOT / "rlshaders_amd" / "host"
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def rows_of(name, sanitize):
    """a module-scoped fixture ``rows``: case -> dict(n, live, leaked, silent) of tests/native/<name>.cpp (ownership_harness.hpp)"""
    @pytest.fixture(scope="module")
    def rows(tmp_path_factory):
        exe = tmp_path_factory.mktemp(name) / name
        cmd = ["g++", "-std=c++14", "-Wall", *(SANITIZE if sanitize else []), f"-I{ROOT / 'include'}", f"-I{HOST}",
               str(ROOT / "tests" / "native" / f"{name}.cpp"), "-o", str(exe)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        out = {}
        for line in p.stdout.splitlines():
            case, n, live, leaked, silent = line.split("\t")
            out[case] = dict(n=int(n), live=int(live), leaked=[int(k) for k in leaked.split(",") if k],
                             silent=[int(k) for k in silent.split(",") if k])
        return out
    return rows


def test_nothing_is_live_after_destruction(rows):
    assert {k: r["live"] for k, r in rows.items() if r["live"]} == {}


def test_a_failing_allocation_throws_and_leaves_nothing_live(rows):
    assert {k: r["silent"] for k, r in rows.items() if r["silent"]} == {}
    assert {k: r["leaked"] for k, r in rows.items() if r["leaked"]} == {}
