"""builds tests/native/nearest_host_check.cpp for test_nearest_bvh.py and test_nearest_host_traversal.py: a stand-alone host
program (g++, -ffp-contract=off, no HIP), plain or under the address and undefined-behaviour sanitizers.  pytest does not collect
this module."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "native" / "nearest_host_check.cpp"
FLAGS = ["-std=c++14", "-Wall", "-Werror", "-ffp-contract=off", "-pthread"]


def build(directory, sanitize=False):
    exe = Path(directory) / ("nearest_host_check_san" if sanitize else "nearest_host_check")
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    p = subprocess.run(["g++", *FLAGS, *extra, str(SOURCE), "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return exe


def run(exe, *args):
    p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    return p.stdout.splitlines()
