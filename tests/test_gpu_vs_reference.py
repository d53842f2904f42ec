"""GPU: the EXACT kernels, through the C ABI, against the reference's own closure code (oracle/_ref/librls_ref.so,
built by build() from the reference checkout) -- with no restatement in between.

The same inputs as tests/test_oracle_vs_reference.py (tests/ref_cases.py), the mixed sets at 2^20 points.  Gates as the
kernel-vs-oracle tests: bits when cases.strict_parity(), cases.assert_tight otherwise; NaNs must sit in the same places
(their payloads are the device's own).  These add to the kernel-vs-oracle tests; they replace none of them.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import cases
import oracle_lib as O
import ref_cases as RC
import ref_lib as R
import rlshaders_amd as RL
from gpu_util import dev, disney_sampler, ggx_sampler, host
from ref_lib import NTHREADS, ref  # noqa: F401  (session fixture)

pytestmark = pytest.mark.gpu

N_MIXED = 1 << 20
GGX_SETS = RC.ggx_sets(N_MIXED)
DISNEY_SETS = RC.disney_sets(N_MIXED)
SSS_SETS = RC.sss_sets(N_MIXED)
LOBES = {"diffuse": RL.RLS_RAY_DIFFUSE, "glossy": RL.RLS_RAY_GLOSSY}


def gate(what, got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), (what, "NaN placement differs", int((ng != nw).sum()))
    g, w = got[~nw], want[~nw]
    if cases.strict_parity():
        d = g.view(np.uint32) != w.view(np.uint32)
        assert not d.any(), (what, "words differing", int(d.sum()), "of", d.size)
        return
    inf = np.isinf(w) | np.isinf(g)
    assert np.array_equal(g[inf], w[inf]), (what, "infinities differ")
    cases.assert_tight(cases.summarize(cases.rel_err(g[~inf], w[~inf])), what)


def _ggx(gpu, d):
    ex = RC.exiting(d["wo"], d["N"])
    og = O.Ggx(d["wo"], d["N"], d["T"], KsColor=d["KsColor"], ior=d["ior"], roughness=d["roughness"],
               anisotropic=d["anisotropic"], exiting=ex)
    return ggx_sampler(gpu, d, exiting=ex), R.Ggx(og)


@pytest.mark.parametrize("name", list(GGX_SETS))
def test_ggx_reflect_refract(gpu, ref, name):
    """GGX sample / eval / pdf / Fresnel and the refraction sample (reflect_refract) against the reference"""
    d, x = GGX_SETS[name]
    x2 = x[::-1].copy()                     # the refraction sample draws the other pairing
    s, rg = _ggx(gpu, d)
    got = [host(t) for t in s.reflectRefract(dev(x[0]), dev(x[1]), dev(x2[0]), dev(x2[1]))]
    want = list(rg.sample_eval_pdf(x[0], x[1])) + list(rg.refract(x2[0], x2[1])[:2])
    for nm, a, b in zip(("wi", "f", "pdf", "fresnel", "wt", "weight"), got, want):
        gate(f"{name} {nm}", a, b)
    # decoupled eval / pdf on the reference's directions and on the adversarial ones
    dirs = {"reference_wi": want[0]}
    dirs.update(RC.indir_sets(d["wo"], d["N"], rg.n))
    for k, wi in dirs.items():
        gate(f"{name} eval {k}", host(s.evalBrdf(dev(wi))), rg.eval(wi))
        gate(f"{name} pdf {k}", host(s.evalPdf(dev(wi))), rg.pdf(wi))


@pytest.mark.parametrize("lobe", list(LOBES))
@pytest.mark.parametrize("name", list(DISNEY_SETS))
def test_disney_triples(gpu, ref, name, lobe):
    d, x = DISNEY_SETS[name]
    sc = {k: d[k] for k in O.DISNEY_SCALARS if k in d}
    rd = R.Disney(O.Disney(d["wo"], d["N"], d["T"], base_color=d.get("base_color", (1, 1, 1)), **sc))
    s = disney_sampler(gpu, d)
    s.setSampleType(LOBES[lobe])
    got = [host(t) for t in s.sampleEvalPdf(dev(x[0]), dev(x[1]))]
    want = rd.sample_eval_pdf(LOBES[lobe], x[0], x[1])
    for nm, a, b in zip(("wi", "f", "pdf"), got, want):
        gate(f"{name} {lobe} {nm}", a, b)
    for k, wi in RC.indir_sets(d["wo"], d["N"], rd.n).items():
        gate(f"{name} {lobe} eval {k}", host(s.evalBrdf(dev(wi))), rd.eval(LOBES[lobe], wi))
        gate(f"{name} {lobe} pdf {k}", host(s.evalPdf(dev(wi))), rd.pdf(LOBES[lobe], wi))


def _sss_dist(d, n):
    dist = np.asarray(d["dist"], np.float32)
    return dist if dist.ndim == 2 else np.ascontiguousarray(np.repeat(dist[:, None], n, axis=1))


@pytest.mark.parametrize("name", list(SSS_SETS))
def test_nd_profile(gpu, ref, name):
    d, x = SSS_SETS[name]
    n = d["N"].shape[1]
    mult = d.get("mult", 1.0)
    rs = R.Sss(O.Sss(n, d["dist"], d["albedo"], multiplier=mult))
    p = RL.NDProfile(gpu, n, dev(_sss_dist(d, n)), dev(d["albedo"]), multiplier=mult)
    got = [host(t) for t in p.sample(dev(x[0]))]
    want = rs.nd_sample(x[0])
    for nm, a, b in zip(("r", "pdf", "profile"), got, want):
        gate(f"{name} ND {nm}", a, b)
    r = want[0]
    gate(f"{name} ND getPdf", host(p.getPdf(dev(r))), rs.nd_pdf(r))
    gate(f"{name} ND evalProfile", host(p.evalProfile(dev(r))), rs.nd_profile(r))


@pytest.mark.parametrize("has_dPdu", [True, False], ids=["dPdu", "polar"])
@pytest.mark.parametrize("name", list(SSS_SETS))
def test_sss_probe(gpu, ref, name, has_dPdu):
    d, x = SSS_SETS[name]
    n = d["N"].shape[1]
    mult = d.get("mult", 1.0)
    rs = R.Sss(O.Sss(n, d["dist"], d["albedo"], multiplier=mult, N=d["N"], T=d["T"], has_dPdu=has_dPdu))
    s = RL.SssSampler(gpu, dev(d["N"]), dev(d["T"]), dev(d["albedo"]), dev(_sss_dist(d, n)), multiplier=mult,
                      has_dPdu=has_dPdu)
    got = {k: host(v) for k, v in s.getProbeRay(dev(x[0]), dev(x[1])).items()}
    want = rs.probe(x[0], x[1])
    for k in ("r", "origin", "dir", "maxdist", "pdf", "profile"):
        gate(f"{name} probe {k}", got[k], want[k])
