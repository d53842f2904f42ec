"""CPU: the oracle's sample loops and rlSkin's layering against the float64 twin (tests/twin64.py) -- the rows whose only
anchor was the oracle itself: rls_ggx_integrate (src/rlGgx.h:97-127, 172-184), integrateRefract (205-245), the explicit rlDisney
loop (src/rlDisney.cpp:299-312), the MIS pdf, the cavity fade and integrateScatter (src/rlSss.h:227-276, 288-357, 379-424) and
shader_evaluate of rlSkin (src/rlSkin.cpp:174-254).  The twin was written from those lines, the oracle from the same lines by
another route; a misreading would have to be made twice to pass.  Batches, gates and both sides: tests/twin_loops_util.py.
The gates were measured at N = 2^18 over three seeds; the tests run the cases.SEED_PARITY batch at 2^16 points, which keeps
them to seconds and can only lower a maximum."""
import numpy as np
import pytest

import cases
import oracle_lib as O
import twin_loops_util as U

N = 1 << 16
SEED = cases.SEED_PARITY


@pytest.fixture(scope="module")
def ggx():
    return U.ggx_case(SEED, N)


@pytest.mark.parametrize("spp_n", U.LOOP_SPP)
def test_ggx_integrate_against_the_float64_twin(ggx, spp_n):
    """the sum of evalBrdf / evalPdf and getAvgReflectWeight: the mean over the closure's own sample count"""
    U.check(f"ggx_integrate/{spp_n}/", U.oracle_ggx_integrate(ggx, spp_n), U.twin_ggx_integrate(ggx, spp_n))


@pytest.mark.parametrize("spp_n", U.LOOP_SPP)
def test_ggx_integrate_refract_traced_against_the_float64_twin(ggx, spp_n):
    """a third of the points leave the medium: their totally internally reflected samples are mirrored, not dropped"""
    got = U.oracle_ggx_refract(ggx, spp_n, True)
    assert got["tir#"][ggx["exiting"] == 1].mean() > 0.01
    U.check(f"ggx_refract/traced/{spp_n}/", got, U.twin_ggx_refract(ggx, spp_n, True))


def test_ggx_integrate_refract_untraced_against_the_float64_twin(ggx):
    U.check("ggx_refract/untraced/", U.oracle_ggx_refract(ggx, 1, False), U.twin_ggx_refract(ggx, 1, False))


@pytest.mark.parametrize("spp_n", U.LOOP_SPP)
def test_disney_integrate_against_the_float64_twin(spp_n):
    """both lobes on the oracle's own streamed directions; the batch has invalid samples, which must not be counted"""
    c = cases.disney_mixed(SEED, N)
    got, wi = U.oracle_disney_integrate(c, spp_n)
    twin = U.twin_disney_integrate(c, spp_n, wi)
    if spp_n > 1:                                                      # about 6 in 1e5 samples are invalid
        assert (twin["specular_count#"] < spp_n * spp_n).any()
    U.check(f"disney_integrate/{spp_n}/", got, twin)


def test_sss_mis_pdf_and_cavity_fade_against_the_float64_twin():
    s = cases.sss_mixed(SEED, N)
    v = U.cavity_case(SEED, N)
    U.check("sss_pointwise/", U.oracle_sss_pointwise(s, *v), U.twin_sss_pointwise(s, *v))


@pytest.mark.parametrize("spp_n", U.SCATTER_SPP)
@pytest.mark.parametrize("scene", list(U.SCENES))
def test_integrate_scatter_against_the_float64_twin(scene, spp_n):
    s = U.sss_case(SEED, N, U.scene_geometry(scene))
    sc = O.make_scene(**U.SCENES[scene])
    got = U.oracle_scatter(s, sc, spp_n)
    assert (got["result"] > 0).any(axis=0).mean() > 0.15              # the probe rays do find lit surface
    U.check(f"scatter/{scene}/{spp_n}/", got, U.twin_scatter(s, sc, spp_n))


def test_skin_one_sample_against_the_float64_twin():
    c = U.skin_case(SEED, N)
    xi = cases.xi(SEED, N, 6)
    U.check("skin/", U.oracle_skin(c, xi), U.twin_skin(c, xi))


@pytest.mark.parametrize("spp_n", U.LOOP_SPP)
def test_skin_integrate_against_the_float64_twin(spp_n):
    c = U.skin_case(SEED, N)
    sc = O.make_scene(**U.SCENES["sphere"])
    twin = U.twin_skin_integrate(c, sc, spp_n)
    at_eps = twin["sssWeight"].astype(np.float32) == np.float32(1e-4)
    assert at_eps.mean() > 0.01                                        # the boundary of src/rlSkin.cpp:244 is in the batch
    assert (twin["sss"][:, at_eps] > 0).any(axis=0).mean() > 0.15      # and `<` keeps its scatter term (one probe: 0.3 lit)
    U.check(f"skin_integrate/{spp_n}/", U.oracle_skin_integrate(c, sc, spp_n), twin)
