"""CPU: rls_trace_scratch_bytes and rls_trace_shadow_scratch_bytes return what they returned before the two emits' staging
got one carve helper (csrc_trace/trace.hip, staging): the values below were read from the library built at the commit before
that change.  No device needed."""
import ctypes as C

import pytest

RAY = {(0, 1): 256, (0, 4): 256, (0, 16): 256, (1, 1): 2048, (1, 4): 2048, (1, 16): 6912, (257, 1): 8704, (257, 4): 108544,
       (257, 16): 1710848, (1048576, 1): 27267072, (1048576, 4): 436211712, (1048576, 16): 6979325952}
SHADOW = {(0, 1, 1): 256, (0, 8, 1): 256, (0, 1, 4): 256, (0, 8, 4): 256, (0, 1, 16): 256, (0, 8, 16): 256, (1, 1, 1): 3072,
          (1, 8, 1): 3072, (1, 1, 4): 3072, (1, 8, 4): 17152, (1, 1, 16): 34048, (1, 8, 16): 270592, (257, 1, 1): 36864,
          (257, 8, 1): 273408, (257, 1, 4): 543744, (257, 8, 4): 4342528, (257, 1, 16): 8684800, (257, 8, 16): 69476608,
          (1048576, 1, 1): 138416128, (1048576, 8, 1): 1107300352, (1048576, 1, 4): 2214596608, (1048576, 8, 4): 17716744192,
          (1048576, 1, 16): 35433484288, (1048576, 8, 16): 283467845632}


@pytest.fixture(scope="module")
def lib():
    from rlshaders_amd import build, trace
    build.build_trace_library()
    return trace.load()


def test_scratch_bytes_of_the_sample_ray_emits(lib):
    b = C.c_size_t()
    for (n, spp_n), want in RAY.items():
        assert lib.rls_trace_scratch_bytes(n, spp_n, C.byref(b)) == 0
        assert b.value == want, (n, spp_n)


def test_scratch_bytes_of_the_light_loops(lib):
    b = C.c_size_t()
    for (n, nl, spp_n), want in SHADOW.items():
        assert lib.rls_trace_shadow_scratch_bytes(n, nl, spp_n, C.byref(b)) == 0
        assert b.value == want, (n, nl, spp_n)
