"""CPU: the oracle (oracle/rls_oracle.c, our restatement) against the reference's own closure code (oracle/_ref, built
by build() from the reference checkout against the stand-in oracle/ref/ai.h), bit for bit.

Both sides are gcc, fp32, without contraction, on the same libm, so no tolerance applies: every output word must be
equal, NaNs and signed zeros included (cases.assert_same_bits).  Rows are SURVEY.md section 8(a)'s.  Inputs: the mixed
generators at 2^18 points, cases.ggx_edge with cases.xi_edge, the testsuite's ten parameter presets, and the named
adversarial sets below.  What the stand-in services decide (oracle/ref/ref_services.cpp) stays unpinned: DESIGN.md 3.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest

import cases
import oracle_lib as O
import ref_cases as RC
import ref_lib as R
from ref_lib import NTHREADS, ref  # noqa: F401  (session fixture)

N_MIXED = RC.N_MIXED
ONE_M, EPS = RC.ONE_M, RC.EPS
KAT = json.loads((Path(__file__).parent / "golden" / "survey_kat.json").read_text())

same = cases.assert_same_bits
f32 = np.float32


def _bits(what, a, b):
    same(a, b, what)


GGX_SETS = RC.ggx_sets()


def _ggx_pair(d):
    wo, N = d["wo"], d["N"]
    og = O.Ggx(wo, N, d["T"], KsColor=d["KsColor"], ior=d["ior"], roughness=d["roughness"],
               anisotropic=d["anisotropic"], exiting=RC.exiting(wo, N), nthreads=NTHREADS)
    return og, R.Ggx(og)


# ------------------------------------------------------------------------------------------------------ a2-a5
def test_util_a2_a5(ref):
    x = cases.xi(cases.SEED_PARITY, N_MIXED, 2)
    edge = np.float32([0.0, 2.0 ** -24, 0.5, ONE_M, 0.25, 0.75])
    a = np.concatenate([x[0], np.repeat(edge, edge.size)])
    b = np.concatenate([x[1], np.tile(edge, edge.size)])
    for nm, o, r in zip(("sphericalDirection", "concentricDiskSample"), O.util_directions(a, b), R.util_directions(a, b)):
        _bits(nm, o, r)
    d = cases.ggx_mixed(cases.SEED_PARITY, N_MIXED)
    for nm, o, r in zip(("reflectDirection", "colorToLuminance"),
                        O.reflect_luminance(d["wo"], d["N"], d["KsColor"]), R.reflect_luminance(d["wo"], d["N"], d["KsColor"])):
        _bits(nm, o, r)


# ----------------------------------------------------------------------------------------------- a6-a17 GGX
@pytest.mark.parametrize("name", list(GGX_SETS))
def test_ggx_a6_a17(ref, name):
    d, x = GGX_SETS[name]
    og, rg = _ggx_pair(d)
    o = og.sample_eval_pdf(x[0], x[1])
    r = rg.sample_eval_pdf(x[0], x[1])
    for nm, a, b in zip(("wi", "f", "pdf", "fresnel"), o, r):
        _bits(f"{name} fused {nm}", a, b)
    # decoupled: eval / pdf on the oracle's directions, and on the reference's (bit-equal above, kept distinct)
    for src, wi in (("oracle_wi", o[0]), ("reference_wi", r[0])):
        _bits(f"{name} eval on {src}", og.eval(wi), rg.eval(wi))
        _bits(f"{name} pdf on {src}", og.pdf(wi), rg.pdf(wi))
    for k, wi in RC.indir_sets(d["wo"], d["N"], og.n).items():
        _bits(f"{name} eval {k}", og.eval(wi), rg.eval(wi))
        _bits(f"{name} pdf {k}", og.pdf(wi), rg.pdf(wi))
    _bits(f"{name} VNDF microfacet", og.microfacet(x[0], x[1]), rg.microfacet(x[0], x[1]))


@pytest.mark.parametrize("name", ["mixed", "edge", "roughness=0", "anisotropic=1.0", "wo==N", "xi0=1-2^-24"])
def test_ggx_ndf_kernel_a10(ref, name):
    d, x = GGX_SETS[name]
    og, rg = _ggx_pair(d)
    _bits(f"{name} NDFKernel sample", og.microfacet(x[0], x[1], ndf_kernel=True),
          rg.microfacet(x[0], x[1], ndf_kernel=True))
    wi = og.sample_eval_pdf(x[0], x[1])[0]
    _bits(f"{name} NDFKernel pdf", og.ndf_pdf(wi), rg.ndf_pdf(wi))


@pytest.mark.parametrize("name", list(GGX_SETS))
def test_ggx_refract_a16(ref, name):
    """the per-sample body of integrateRefract, driven through the reference's loop (one sample, unit environment)"""
    d, x = GGX_SETS[name]
    og, rg = _ggx_pair(d)
    o, r = og.refract(x[0], x[1]), rg.refract(x[0], x[1])
    for nm, a, b in zip(("wt", "weight"), o[:2], r[:2]):
        _bits(f"{name} refract {nm}", a, b)
    assert np.array_equal(o[2], r[2]), (name, "TIR flags differ", int((o[2] != r[2]).sum()))


def test_ggx_survey_kat_reproduced(ref):
    """the reference build reproduces SURVEY.md 8(c)'s GGX known answers, to the bit of their 9-digit prints"""
    k = KAT["ggx"]
    one = lambda v: np.asarray(v, np.float32).reshape(3, 1)
    og = O.Ggx(one(k["wo"]), one(k["N"]), one(k["T"]), KsColor=k["KsColor"], ior=k["ior"],
               roughness=float(np.sqrt(np.float32(k["roughness_squared"]))), anisotropic=k["anisotropic"])
    wi, f, pdf, _ = R.Ggx(og).sample_eval_pdf(np.float32([k["xi"][0]]), np.float32([k["xi"][1]]))
    assert np.array_equal(wi[:, 0], np.float32(k["L"])), wi[:, 0]
    assert f[0, 0] == np.float32(k["f"]) and pdf[0] == np.float32(k["pdf"]), (f[:, 0], pdf)


# -------------------------------------------------------------------------------------------- a18-a28 Disney
DISNEY_SETS = RC.disney_sets()
LOBES = {"diffuse": O.RAY_DIFFUSE, "glossy": O.RAY_GLOSSY}


def _disney_pair(d):
    sc = {k: d[k] for k in O.DISNEY_SCALARS if k in d}
    od = O.Disney(d["wo"], d["N"], d["T"], base_color=d.get("base_color", (1, 1, 1)), nthreads=NTHREADS, **sc)
    return od, R.Disney(od)


@pytest.mark.parametrize("lobe", list(LOBES))
@pytest.mark.parametrize("name", list(DISNEY_SETS))
def test_disney_a18_a28(ref, name, lobe):
    d, x = DISNEY_SETS[name]
    od, rd = _disney_pair(d)
    lb = LOBES[lobe]
    o = od.sample_eval_pdf(lb, x[0], x[1])
    r = rd.sample_eval_pdf(lb, x[0], x[1])
    for nm, a, b in zip(("wi", "f", "pdf"), o, r):
        _bits(f"{name} {lobe} fused {nm}", a, b)
    dirs = {"oracle_wi": o[0], "reference_wi": r[0]}
    dirs.update(RC.indir_sets(d["wo"], d["N"], od.n))
    # the other lobe's directions reach the branches its own sampler avoids
    dirs["other_lobe_wi"] = od.sample(O.RAY_GLOSSY if lb == O.RAY_DIFFUSE else O.RAY_DIFFUSE, x[0], x[1])
    for src, wi in dirs.items():
        _bits(f"{name} {lobe} eval on {src}", od.eval(lb, wi), rd.eval(lb, wi))
        _bits(f"{name} {lobe} pdf on {src}", od.pdf(lb, wi), rd.pdf(lb, wi))


@pytest.mark.parametrize("name", ["mixed", "edge", "roughness=0", "roughness=1", "anisotropic=1.0", "xi0=1-2^-24",
                                  "xi1=1-2^-24"])
def test_disney_alternates_a27(ref, name):
    d, x = DISNEY_SETS[name]
    od, rd = _disney_pair(d)
    wi = od.sample(O.RAY_GLOSSY, x[0], x[1])
    _bits(f"{name} sampleGTR2AnisoDirection", od.alt(0, rx=x[0], ry=x[1]), rd.alt(0, rx=x[0], ry=x[1]))
    _bits(f"{name} sampleGTR2Direction", od.alt(1, rx=x[0], ry=x[1]), rd.alt(1, rx=x[0], ry=x[1]))
    _bits(f"{name} non-VNDF evalSpecularPdf", od.alt(2, v=wi), rd.alt(2, v=wi))
    _bits(f"{name} D_GTR2", od.alt(3, v=wi), rd.alt(3, v=wi))


# --------------------------------------------------------------------------------------- a29-a34, a37 SSS
SSS_SETS = RC.sss_sets()


def _sss_pair(d, has_dPdu=True):
    n = d["N"].shape[1]
    os_ = O.Sss(n, d["dist"], d["albedo"], multiplier=d.get("mult"), N=d["N"], T=d["T"], has_dPdu=has_dPdu,
                nthreads=NTHREADS)
    return os_, R.Sss(os_)


@pytest.mark.parametrize("name", list(SSS_SETS))
def test_nd_profile_a29_a32(ref, name):
    d, x = SSS_SETS[name]
    os_, rs = _sss_pair(d)
    o, r = os_.nd_sample(x[0]), rs.nd_sample(x[0])
    for nm, a, b in zip(("r", "pdf", "profile"), o, r):
        _bits(f"{name} ND {nm}", a, b)
    dist = np.asarray(d["dist"], np.float32)
    dist = dist if dist.ndim == 2 else np.repeat(dist[:, None], os_.n, axis=1)
    maxR = (dist.max(axis=0) * f32(3)).astype(np.float32)
    radii = {"r=0": np.zeros(os_.n, np.float32), "r=eps": np.full(os_.n, EPS, np.float32), "r=maxR": maxR,
             "r>maxR": (maxR * f32(4)).astype(np.float32), "r=sampled": o[0]}
    for k, rr in radii.items():
        _bits(f"{name} ND getPdf {k}", os_.nd_pdf(rr), rs.nd_pdf(rr))
        _bits(f"{name} ND evalProfile {k}", os_.nd_profile(rr), rs.nd_profile(rr))


def test_gaussian_profile(ref):
    """GaussianProfile (dead in the reference); Arnold's fast_exp is the stand-in expf on both sides"""
    x = cases.xi(cases.SEED_PARITY, N_MIXED, 2)
    dist = (f32(0.01) + f32(3) * x[1]).astype(np.float32)
    rx = np.concatenate([x[0][:-4], np.float32([0, 2.0 ** -24, 0.5, ONE_M])])
    for nm, a, b in zip(("r", "pdf", "profile"), O.gauss(dist, rx), R.gauss(dist, rx)):
        _bits(f"gauss {nm}", a, b)


@pytest.mark.parametrize("has_dPdu", [True, False], ids=["dPdu", "polar"])
@pytest.mark.parametrize("name", list(SSS_SETS))
def test_sss_probe_a33_a34(ref, name, has_dPdu):
    d, x = SSS_SETS[name]
    os_, rs = _sss_pair(d, has_dPdu)
    o, r = os_.probe(x[0], x[1]), rs.probe(x[0], x[1])
    for k in o:
        _bits(f"{name} probe {k}", o[k], r[k])


@pytest.mark.parametrize("name", ["mixed", "edge", "xi0=0", "xi0=1-2^-24", "xi0=0.5"])
def test_sss_sample_diffuse_a37(ref, name):
    d, x = SSS_SETS[name]
    _bits(f"{name} sampleDiffuseDirection", O.sample_diffuse_direction(d["N"], d["T"], x[0], x[1], nthreads=NTHREADS),
          R.sample_diffuse_direction(d["N"], d["T"], x[0], x[1]))


def test_nd_survey_kat_reproduced(ref):
    """SURVEY.md 8(c)'s ND known answers were printed from the double-overload build: the fp32 reference build agrees
    to the 1-2 last digits its provenance states"""
    k = KAT["nd"]
    rs = R.Sss(O.Sss(1, k["dist"], k["albedo"]))
    for xv, rv in k["radius"]:
        got = rs.nd_sample(np.float32([xv]))[0][0]
        assert abs(got - rv) <= 2e-6 * rv, (xv, got, rv)
    assert abs(rs.nd_pdf(np.float32([0.5]))[0] - k["pdf_at_0.5"]) <= 2e-7
    assert abs(rs.nd_profile(np.float32([0.5]))[0, 0] - k["profile_r_at_0.5"]) <= 2e-7
