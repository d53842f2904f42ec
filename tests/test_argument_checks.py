"""CPU: the argument checks of every closure and loop entry point of librlshaders_amd.so and of the four calls of
librls_trace.so, in EXACT and FAST mode.

tests/native/argument_checks.cpp builds an rls_context by hand (device 0, no stream), hands each entry point a set of dummy
planes that passes every check, then breaks one argument at a time: a NULL required plane, a mixed-NULL rgb,
materials.count == 0, n < 0, spp_n 0 and 17, an unknown enum, n == 0 with and without a bad argument.  Arguments that pass
reach the launch, where hipSetDevice fails for want of a device (RLS_ERR_HIP): a check that goes missing shows up as a
wrong status.  That is only safe with no GPU visible -- the planes are dummies -- so the test skips where torch sees a
GPU, and the driver refuses to run where HIP reports a device."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "native" / "argument_checks.cpp"

ENTRY_POINTS = {
    "rls_ggx_sample", "rls_ggx_eval", "rls_ggx_pdf", "rls_ggx_sample_eval_pdf", "rls_ggx_refract_sample",
    "rls_ggx_reflect_refract", "rls_ggx_microfacet", "rls_ggx_ndf_pdf", "rls_ggx_integrate", "rls_ggx_integrate_refract",
    "rls_ggx_direct_lighting", "rls_ggx_shade",
    "rls_disney_sample", "rls_disney_eval", "rls_disney_pdf", "rls_disney_sample_eval_pdf", "rls_disney_alt_sample",
    "rls_disney_alt_pdf", "rls_disney_d_gtr2", "rls_disney_integrate", "rls_disney_integrate_chunked",
    "rls_disney_direct_lighting", "rls_disney_shade",
    "rls_gaussian_sample", "rls_libm_eval", "rls_sss_cavity_fade", "rls_sss_sample_diffuse_direction", "rls_util_directions",
    "rls_util_reflect_luminance",
    "rls_nd_sample", "rls_nd_pdf", "rls_nd_eval", "rls_sss_probe_ray", "rls_sss_mis_pdf", "rls_sss_integrate_scatter",
    "rls_skin_sample_eval_pdf", "rls_skin_integrate",
    "rls_trace_ggx_glossy_emit", "rls_trace_ggx_refract_emit", "rls_trace_ggx_glossy_resolve", "rls_trace_ggx_refract_resolve",
}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the driver hands dummy planes to the entry points")
    from rlshaders_amd import build
    build.build_trace_library()
    exe = tmp_path_factory.mktemp("argument_checks") / "argument_checks"
    cmd = [build._hipcc(), "-std=c++17", "-O1", "-x", "hip", "--offload-host-only", "-Wall", "-DRLS_FAST=0", str(DRIVER),
           "-o", str(exe), f"-L{build.LIBDIR}", "-lrls_trace", "-lrlshaders_amd", f"-Wl,-rpath,{build.LIBDIR}"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    rows = []
    for line in p.stdout.splitlines():
        entry, what, fast, status, want, prefix, text, message = line.split("\t")
        rows.append(dict(entry=entry, what=what, fast=int(fast), status=int(status), want=int(want), prefix=prefix,
                         text=text, message=message))
    return rows


def test_every_entry_point_in_both_modes(cases):
    assert {c["entry"] for c in cases} == ENTRY_POINTS
    for fast in (0, 1):
        assert {c["entry"] for c in cases if c["fast"] == fast} == ENTRY_POINTS
    assert len(cases) > 1000


def test_status_and_message_of_every_case(cases):
    wrong = []
    for c in cases:
        ok = c["status"] == c["want"]
        if ok and c["want"] in (1, 5):                      # RLS_ERR_INVALID_ARGUMENT, RLS_ERR_UNSUPPORTED: the text
            ok = c["message"].partition(": ")[2] == c["text"]
        elif ok and c["want"] == 3:                         # RLS_ERR_HIP: every check passed, the launch found no device
            ok = c["message"].startswith("HIP error ")
        if not ok:
            wrong.append(f'{c["entry"]} [{c["what"]}, fast={c["fast"]}]: status {c["status"]} "{c["message"]}", '
                         f'want {c["want"]} "{c["text"]}"')
    assert not wrong, "\n".join(wrong)


def test_messages_name_the_function_that_refused(cases):
    """the prefix of a refusal is the public entry point (copy_lights for the lights, emit / resolve for the trace calls)"""
    wrong = [f'{c["entry"]} [{c["what"]}]: "{c["message"]}"' for c in cases
             if c["want"] in (1, 5) and c["message"].partition(": ")[0] != c["prefix"]]
    assert not wrong, "\n".join(wrong)
