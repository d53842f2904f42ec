"""numpy/ctypes front end of the reference build (oracle/_ref/librls_ref.so: the reference's own closure code
compiled by oracle/Makefile's `ref` target against the stand-in oracle/ref/ai.h).  TEST INFRASTRUCTURE ONLY.

Every entry point mirrors an oracle batch function and takes the oracle's SoA structs (oracle_lib), so one set
of input arrays feeds both sides.  Nothing here reads the reference checkout: only what build() produced.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np
import pytest

import oracle_lib as O
from oracle_lib import _p, _v, f32

ROOT = Path(__file__).resolve().parent.parent
LIB_PATH = ROOT / "oracle" / "_ref" / "librls_ref.so"
PROVENANCE = ROOT / "oracle" / "_ref" / "provenance.json"
NTHREADS = min(16, os.cpu_count() or 1)

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise FileNotFoundError(f"{LIB_PATH} is missing: run build() (oracle/Makefile target `ref`) where the "
                                    "reference checkout is present")
        _lib = C.CDLL(str(LIB_PATH))
    return _lib


@pytest.fixture(scope="session")
def ref():
    """the reference build; fails (never skips) when build() has not produced it"""
    try:
        return lib()
    except FileNotFoundError as e:
        pytest.fail(f"run build(): {e}")


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


class Ggx:
    """the reference's rls::GgxSampler over the same SoA as oracle_lib.Ggx (whose `exiting` plane it ignores:
    the closure decides from dot(N, -wo) itself)"""

    def __init__(self, og: O.Ggx):
        self.o, self.n = og, og.n

    def sample_eval_pdf(self, rx, ry):
        n = self.n
        rx, ry = f32(rx), f32(ry)
        wi, f = np.empty((3, n), np.float32), np.empty((3, n), np.float32)
        pdf, F = np.empty(n, np.float32), np.empty(n, np.float32)
        lib().ref_batch_ggx_sample_eval_pdf(C.c_int64(n), C.byref(self.o.soa), _p(rx), _p(ry), _v(wi), _v(f), _p(pdf),
                                            _p(F), NTHREADS)
        return wi, f, pdf, F

    def eval(self, wi):
        wi = f32(wi)
        f = np.empty((3, self.n), np.float32)
        lib().ref_batch_ggx_eval(C.c_int64(self.n), C.byref(self.o.soa), _v(wi), _v(f), NTHREADS)
        return f

    def pdf(self, wi):
        wi = f32(wi)
        pdf = np.empty(self.n, np.float32)
        lib().ref_batch_ggx_pdf(C.c_int64(self.n), C.byref(self.o.soa), _v(wi), _p(pdf), NTHREADS)
        return pdf

    def refract(self, rx, ry):
        n = self.n
        rx, ry = f32(rx), f32(ry)
        wt, w, flag = np.empty((3, n), np.float32), np.empty(n, np.float32), np.empty(n, np.uint8)
        lib().ref_batch_ggx_refract(C.c_int64(n), C.byref(self.o.soa), _p(rx), _p(ry), _v(wt), _p(w), _u8(flag),
                                    NTHREADS)
        return wt, w, flag

    def microfacet(self, rx, ry, ndf_kernel=False):
        rx, ry = f32(rx), f32(ry)
        m = np.empty((3, self.n), np.float32)
        lib().ref_batch_ggx_microfacet(C.c_int64(self.n), C.byref(self.o.soa), _p(rx), _p(ry), _v(m), int(ndf_kernel),
                                       NTHREADS)
        return m

    def ndf_pdf(self, wi):
        wi = f32(wi)
        pdf = np.empty(self.n, np.float32)
        lib().ref_batch_ggx_ndf_pdf(C.c_int64(self.n), C.byref(self.o.soa), _v(wi), _p(pdf), NTHREADS)
        return pdf


class Disney:
    """the reference's DisneySampler over the same SoA as oracle_lib.Disney"""

    def __init__(self, od: O.Disney):
        self.o, self.n = od, od.n

    def sample_eval_pdf(self, lobe, rx, ry):
        n = self.n
        rx, ry = f32(rx), f32(ry)
        wi, f, pdf = np.empty((3, n), np.float32), np.empty((3, n), np.float32), np.empty(n, np.float32)
        lib().ref_batch_disney_sample_eval_pdf(C.c_int64(n), C.byref(self.o.soa), lobe, _p(rx), _p(ry), _v(wi), _v(f),
                                               _p(pdf), NTHREADS)
        return wi, f, pdf

    def eval(self, lobe, wi):
        wi = f32(wi)
        f = np.empty((3, self.n), np.float32)
        lib().ref_batch_disney_eval(C.c_int64(self.n), C.byref(self.o.soa), lobe, _v(wi), _v(f), NTHREADS)
        return f

    def pdf(self, lobe, wi):
        wi = f32(wi)
        pdf = np.empty(self.n, np.float32)
        lib().ref_batch_disney_pdf(C.c_int64(self.n), C.byref(self.o.soa), lobe, _v(wi), _p(pdf), NTHREADS)
        return pdf

    def alt(self, kind, rx=None, ry=None, v=None):
        n = self.n
        out3, out1 = np.zeros((3, n), np.float32), np.zeros(n, np.float32)
        rx = f32(rx) if rx is not None else out1
        ry = f32(ry) if ry is not None else out1
        v = f32(v) if v is not None else out3
        lib().ref_batch_disney_alt(C.c_int64(n), C.byref(self.o.soa), int(kind), _p(rx), _p(ry), _v(v), _v(out3),
                                   _p(out1), NTHREADS)
        return out3 if kind < 2 else out1


class Sss:
    """the reference's NDProfile / SssSampler<NDProfile> over the same SoA as oracle_lib.Sss"""

    def __init__(self, os_: O.Sss):
        self.o, self.n = os_, os_.n

    def nd_sample(self, rx):
        n = self.n
        rx = f32(rx)
        r, pdf, prof = np.empty(n, np.float32), np.empty(n, np.float32), np.empty((3, n), np.float32)
        lib().ref_batch_nd_sample_pdf_profile(C.c_int64(n), C.byref(self.o.soa), _p(rx), _p(r), _p(pdf), _v(prof),
                                              NTHREADS)
        return r, pdf, prof

    def nd_pdf(self, r):
        r = f32(r)
        pdf = np.empty(self.n, np.float32)
        lib().ref_batch_nd_pdf(C.c_int64(self.n), C.byref(self.o.soa), _p(r), _p(pdf), NTHREADS)
        return pdf

    def nd_profile(self, r):
        r = f32(r)
        prof = np.empty((3, self.n), np.float32)
        lib().ref_batch_nd_profile(C.c_int64(self.n), C.byref(self.o.soa), _p(r), _v(prof), NTHREADS)
        return prof

    def probe(self, rx, ry):
        n = self.n
        rx, ry = f32(rx), f32(ry)
        out = dict(r=np.empty(n, np.float32), origin=np.empty((3, n), np.float32), dir=np.empty((3, n), np.float32),
                   maxdist=np.empty(n, np.float32), pdf=np.empty(n, np.float32), profile=np.empty((3, n), np.float32))
        lib().ref_batch_sss_probe(C.c_int64(n), C.byref(self.o.soa), self.o.has_dPdu, _p(rx), _p(ry), _p(out["r"]),
                                  _v(out["origin"]), _v(out["dir"]), _p(out["maxdist"]), _p(out["pdf"]),
                                  _v(out["profile"]), NTHREADS)
        return out


def sample_diffuse_direction(normal, T, rx, ry):
    normal, T, rx, ry = f32(normal), f32(T), f32(rx), f32(ry)
    wi = np.empty((3, normal.shape[1]), np.float32)
    lib().ref_batch_sss_sample_diffuse(C.c_int64(normal.shape[1]), _v(normal), _v(T), _p(rx), _p(ry), _v(wi), NTHREADS)
    return wi


def gauss(dist_x, rx):
    dist_x, rx = f32(dist_x), f32(rx)
    n = dist_x.shape[0]
    r, pdf, prof = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.float32)
    lib().ref_batch_gauss(C.c_int64(n), _p(dist_x), _p(rx), _p(r), _p(pdf), _p(prof), NTHREADS)
    return r, pdf, prof


def util_directions(a, b):
    a, b = f32(a), f32(b)
    n = a.shape[0]
    sph, disk = np.empty((3, n), np.float32), np.empty((3, n), np.float32)
    lib().ref_batch_util(C.c_int64(n), _p(a), _p(b), _v(sph), _v(disk), 1)
    return sph, disk


def reflect_luminance(i, nrm, color):
    i, nrm, color = f32(i), f32(nrm), f32(color)
    n = i.shape[1]
    refl, lum = np.empty((3, n), np.float32), np.empty(n, np.float32)
    lib().ref_batch_reflect_luminance(C.c_int64(n), _v(i), _v(nrm), _v(color), _v(refl), _p(lum))
    return refl, lum
