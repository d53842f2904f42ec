"""GPU: the EXACT-mode kernels of the sample loops and of rlSkin's layering against the float64 twin (tests/twin64.py)
directly -- not through the oracle -- under the gates of the CPU comparison (tests/twin_loops_util.py: measured oracle against
twin on the CPU; nothing the device returns sets a gate).  n = 4096 + 77: sixteen full 256-point tiles and a partial one."""
import numpy as np
import pytest

import cases
import rlshaders_amd as R
import twin_loops_util as U
from gpu_util import dev, disney_sampler, ggx_sampler, host

pytestmark = pytest.mark.gpu

N = 4096 + 77
SEED = cases.SEED_PARITY


@pytest.fixture(scope="module")
def ggx():
    return U.ggx_case(SEED, N)


def _scene(name):
    return R.make_scene(**U.SCENES[name])


def _sss(gpu, s):
    return R.SssSampler(gpu, dev(s["N"]), dev(s["T"]), dev(s["albedo"]), dev(s["dist"]))


def _skin(gpu, c):
    return R.SkinShader(gpu, dev(c["wo"]), dev(c["N"]), dev(c["T"]), **{k: dev(v) for k, v in c["params"].items()})


@pytest.mark.parametrize("spp_n", U.LOOP_SPP)
def test_ggx_integrate(gpu, oracle, ggx, spp_n):
    s, a = ggx_sampler(gpu, ggx, exiting=ggx["exiting"]).integrate(spp_n, U.SAMPLER_SEED, first_index=U.FIRST)
    U.check(f"ggx_integrate/{spp_n}/", {"sum": host(s), "fresnel_mean": host(a)}, U.twin_ggx_integrate(ggx, spp_n))


@pytest.mark.parametrize("spp_n", U.LOOP_SPP)
def test_ggx_integrate_refract_traced(gpu, oracle, ggx, spp_n):
    r, t = ggx_sampler(gpu, ggx, exiting=ggx["exiting"]).integrateRefract(spp_n, U.SAMPLER_SEED, traced=True, env=U.ENV,
                                                                        want_tir=True, first_index=U.FIRST)
    assert host(t)[ggx["exiting"] == 1].mean() > 0.01
    U.check(f"ggx_refract/traced/{spp_n}/", {"result": host(r), "tir#": host(t)}, U.twin_ggx_refract(ggx, spp_n, True))


def test_ggx_integrate_refract_untraced(gpu, oracle, ggx):
    r, t = ggx_sampler(gpu, ggx, exiting=ggx["exiting"]).integrateRefract(1, U.SAMPLER_SEED, traced=False, env=U.ENV,
                                                                        want_tir=True, first_index=U.FIRST)
    U.check("ggx_refract/untraced/", {"result": host(r), "tir#": host(t)}, U.twin_ggx_refract(ggx, 1, False))


@pytest.mark.parametrize("spp_n", U.LOOP_SPP)
def test_disney_integrate(gpu, oracle, spp_n):
    """reduced mode gives the sums and counts; streamed mode the directions the twin evaluates"""
    c = cases.disney_mixed(SEED, N)
    d = disney_sampler(gpu, c)
    o = d.integrate(spp_n, U.SAMPLER_SEED, first_index=U.FIRST)
    wi = host(d.integrate(spp_n, U.SAMPLER_SEED, streamed=True, first_index=U.FIRST)["wi"])
    got = {"diffuse_sum": host(o["diffuse_sum"]), "diffuse_count#": host(o["diffuse_count"]),
           "specular_sum": host(o["specular_sum"]), "specular_count#": host(o["specular_count"])}
    U.check(f"disney_integrate/{spp_n}/", got, U.twin_disney_integrate(c, spp_n, wi))


def test_sss_mis_pdf_and_cavity_fade(gpu, oracle):
    s = cases.sss_mixed(SEED, N)
    disp, sN, No = U.cavity_case(SEED, N)
    got = {"mis_pdf": host(_sss(gpu, s).misPdf(dev(disp), dev(sN))),
           "cavity_fade": host(R.SssSampler.cavityFade(gpu, dev(disp), dev(sN), dev(No)))}
    U.check("sss_pointwise/", got, U.twin_sss_pointwise(s, disp, sN, No))


@pytest.mark.parametrize("spp_n", U.SCATTER_SPP)
@pytest.mark.parametrize("scene", list(U.SCENES))
def test_integrate_scatter(gpu, oracle, scene, spp_n):
    s = U.sss_case(SEED, N, U.scene_geometry(scene))
    r, d = _sss(gpu, s).integrateScatter(dev(s["P"]), _scene(scene), spp_n, U.SAMPLER_SEED, want_depth=True, first_index=U.FIRST)
    got = {"result": host(r), "depth#": host(d)}
    assert (got["result"] > 0).any(axis=0).mean() > 0.15
    U.check(f"scatter/{scene}/{spp_n}/", got, U.twin_scatter(s, oracle.make_scene(**U.SCENES[scene]), spp_n))


def test_skin_sample_eval_pdf(gpu, oracle):
    c = U.skin_case(SEED, N)
    xi = cases.xi(SEED, N, 6)
    got = {k: host(v) for k, v in _skin(gpu, c).sampleEvalPdf(dev(xi)).items()}
    U.check("skin/", got, U.twin_skin(c, xi))


@pytest.mark.parametrize("spp_n", U.SCATTER_SPP)
def test_skin_integrate_without_lights(gpu, oracle, spp_n):
    c = U.skin_case(SEED, N)
    got = {k: host(v) for k, v in _skin(gpu, c).integrate(dev(c["N"]), _scene("sphere"), spp_n, U.SAMPLER_SEED, env=U.ENV,
                                                          first_index=U.FIRST).items()}
    twin = U.twin_skin_integrate(c, oracle.make_scene(**U.SCENES["sphere"]), spp_n)
    assert (twin["sssWeight"].astype(np.float32) == np.float32(1e-4)).mean() > 0.01      # the boundary of src/rlSkin.cpp:244
    U.check(f"skin_integrate/{spp_n}/", got, twin)
