"""CPU: the command lines of rlshaders_amd/build.py, held to a recording (tests/golden/build_commands.json).

Every library is built for real first, so that no step below finds a prerequisite out of date; then ``build.subprocess.run`` is replaced by a recorder that
reports success, every ``build_*_library`` is forced and every example and tool is called with its output made stale, and the
argv lists -- the repository root replaced by a placeholder -- are compared with the recording: flags, ``-cuid``, ``-D``,
their order, object and output paths.  The recording was made from the build driver as it stood before its companion
libraries were described in one table; a change to it is a change to what is compiled, and is made on purpose:

    python tests/test_build_commands.py --record

Within one step the compile jobs run on a thread pool, so a step's commands are compared as a sorted list.  No real output is
touched: the recorder writes nothing, and the mtimes moved to make an output stale are put back."""
import json
import os
import sys
import threading
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "build_commands.json"
TRACE_EXAMPLES = ("example_trace", "example_trace_bounce", "example_trace_skin_bounce", "example_trace_shadow", "example_trace_path")
HOST_EXAMPLES = ("example_arnold_stub", "example_multi_gpu", "example_host_pipeline", "test_arnold_stub")


def steps(build):
    """name -> (the call, the outputs to make stale before it)"""
    out = {"build_library": (lambda: build.build_library(force=True), ())}
    for lib in ("rr", "trace", "walk", "shadow_walk", "nearest", "nearest_refit"):
        out[f"build_{lib}_library"] = (lambda f=getattr(build, f"build_{lib}_library"): f(force=True), ())
    for name in TRACE_EXAMPLES:
        out[f"build_trace_example:{name}"] = (lambda n=name: build.build_trace_example(name=n), (build.OBJDIR / name,))
    for ex in ("walk", "shadow_walk", "nearest", "nearest_refit"):
        out[f"build_{ex}_example"] = (getattr(build, f"build_{ex}_example"), (build.OBJDIR / f"example_{ex}",))
    out["build_nearest_stats"] = (build.build_nearest_stats, (build.OBJDIR / "nearest_stats",))
    out["build_libm_probe"] = (lambda: build.build_libm_probe(force=True), ())
    out["build_host_examples"] = (build.build_host_examples, tuple(build.OBJDIR / n for n in HOST_EXAMPLES))
    return out


def build_for_real(build):
    build.build_library()
    for lib in ("trace", "walk", "shadow_walk", "nearest", "nearest_refit"):
        getattr(build, f"build_{lib}_library")()


def record(build, patch):
    """the argv lists of every step; patch(obj, name, value) replaces an attribute until the caller undoes it"""
    calls, lock = [], threading.Lock()

    def run(cmd, **kwargs):
        with lock:
            calls.append([str(a) for a in cmd])
        return SimpleNamespace(returncode=0, stdout="", stderr="")

    patch(build.subprocess, "run", run)
    got = {}
    for name, (call, outputs) in steps(build).items():
        del calls[:]
        was = [(p, p.stat().st_mtime_ns) for p in outputs if p.exists()]
        try:
            for p, _ in was:
                os.utime(p, ns=(0, 0))
            call()
        finally:
            for p, t in was:
                os.utime(p, ns=(t, t))
        got[name] = sorted(portable(c) for c in calls)
    return got


def portable(cmd):
    head = "hipcc" if Path(cmd[0]).name == "hipcc" else cmd[0]
    return [head] + [a.replace(str(ROOT), "<ROOT>") for a in cmd[1:]]


def test_every_command_line_is_the_recorded_one(monkeypatch):
    from rlshaders_amd import build
    build_for_real(build)
    want = json.loads(GOLDEN.read_text())
    got = record(build, monkeypatch.setattr)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    assert all(got.values())                                        # every step ran something


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        raise SystemExit(__doc__)
    sys.path.insert(0, str(ROOT))
    from rlshaders_amd import build as _build
    build_for_real(_build)
    GOLDEN.write_text(json.dumps(record(_build, setattr), indent=1) + "\n")
