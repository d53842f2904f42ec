"""CPU: the argument checks of the five routing entry points (rls_trace_route_scratch_bytes, rls_trace_route_hits,
rls_trace_route_gather, rls_trace_route_scatter, rls_trace_route_fill; librls_trace.so).

tests/native/trace_route_checks.cpp runs them with a hand-built context, dummy planes and no GPU: the status, the message and
its entry-point prefix of every refusal the header lists, RLS_ERR_UNSUPPORTED past 2^32 - 1 rays, that a passing argument set
reaches the launch (RLS_ERR_HIP), and that an empty call succeeds without one while a bad argument beside it is still refused.
Like tests/test_trace_abi.py's native drivers it skips where torch sees a GPU."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "native" / "trace_route_checks.cpp"
ENTRY = dict(scratch_bytes="rls_trace_route_scratch_bytes", hits="rls_trace_route_hits", gather="rls_trace_route_gather",
             scatter="rls_trace_route_scatter", fill="rls_trace_route_fill")
OK, INVALID, HIP, UNSUPPORTED = 0, 1, 3, 5


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the driver hands dummy planes to the entry points")
    from rlshaders_amd import build
    build.build_trace_library()
    exe = tmp_path_factory.mktemp("trace_route_checks") / "trace_route_checks"
    cmd = [build._hipcc(), "-std=c++17", "-O1", "-x", "hip", "--offload-host-only", "-Wall", "-DRLS_FAST=0", str(DRIVER),
           "-o", str(exe), f"-L{build.LIBDIR}", "-lrls_trace", "-lrlshaders_amd", f"-Wl,-rpath,{build.LIBDIR}"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    rows = []
    for line in p.stdout.splitlines():
        verb, what, status, want, text, message = line.split("\t")
        rows.append(dict(verb=verb, what=what, status=int(status), want=int(want), text=text, message=message))
    return rows


def test_every_listed_refusal_is_exercised(cases):
    have = {v: {c["what"] for c in cases if c["verb"] == v} for v in ENTRY}
    assert have["scratch_bytes"] >= {"bytes NULL", "rays < 0", "rays = 2^32", "bins 0", "bins 17", "valid"}
    assert have["hits"] >= {"ctx NULL", "routes NULL", "rays < 0", "rays = 2^32", "bins 0", "bins 17", "offsets NULL", "bin NULL",
                            "order NULL", "scratch NULL", "scratch short", "slot NULL", "valid", "rays == 0"}
    for v in ("gather", "scatter"):
        assert have[v] >= {"ctx NULL", "m < 0", "planes NULL", "n_w32 25", "n_u8 9", "src_w32 NULL below the count",
                           "dst_u8 NULL below the count", "word dst == src", "byte dst == src", "index NULL", "valid", "m == 0",
                           "m == 0, planes NULL"}
    assert have["fill"] >= {"ctx NULL", "m < 0", "n_planes 0", "n_planes 25", "dst NULL", "value NULL",
                            "dst plane NULL below the count", "index NULL", "valid", "m == 0", "m == 0, n_planes 25"}
    statuses = {c["want"] for c in cases}
    assert statuses == {OK, INVALID, HIP, UNSUPPORTED}


def test_statuses_messages_and_prefixes(cases):
    wrong = []
    for c in cases:
        ok = c["status"] == c["want"]
        if ok and c["want"] in (INVALID, UNSUPPORTED):           # "<entry point>: <text>"
            prefix, _, text = c["message"].partition(": ")
            ok = prefix == ENTRY[c["verb"]] and text == c["text"]
        elif ok and c["want"] == HIP:                            # every check passed, the launch found no device
            ok = c["message"].startswith("HIP error ")
        if not ok:
            wrong.append(f'{c["verb"]} {c["what"]}: status {c["status"]} "{c["message"]}", want {c["want"]} "{c["text"]}"')
    assert not wrong, "\n".join(wrong)
