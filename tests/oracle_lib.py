"""numpy/ctypes front end of the CPU oracle (oracle/rls_oracle.c).  TEST INFRASTRUCTURE ONLY: used by
tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg as the checker / timed baseline.
Nothing under rlshaders_amd/ imports it.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
ORACLE_DIR = ROOT / "oracle"
LIB_PATH = ORACLE_DIR / "build" / "librls_oracle.so"

RAY_DIFFUSE = 0x08
RAY_GLOSSY = 0x10

DISNEY_SCALARS = ("subsurface", "metallic", "specular", "specular_tint", "roughness", "anisotropic",
                  "sheen", "sheen_tint", "clearcoat", "clearcoat_gloss")

# stream ids (oracle/rls_oracle.h)
S_N0, S_N1, S_T, S_WO0, S_WO1, S_ROUGH, S_IOR, S_ANISO, S_KS_R, S_KS_G, S_KS_B = range(11)
S_XI0 = 11
S_PARAM0 = 32
S_SCRAMBLE = 64

fp = C.POINTER(C.c_float)


class V3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class RGB(C.Structure):
    _fields_ = [("r", C.c_float), ("g", C.c_float), ("b", C.c_float)]


class CV3P(C.Structure):
    _fields_ = [("x", fp), ("y", fp), ("z", fp)]


class GgxSoa(C.Structure):
    _fields_ = [("wo", CV3P), ("N", CV3P), ("T", CV3P), ("KsColor", CV3P),
                ("specularRoughness", fp), ("ior", fp), ("anisotropic", fp), ("exiting", C.POINTER(C.c_uint8))]


class Light(C.Structure):
    """orc_light (same layout as rls_sphere_light)."""
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("radiance", C.c_float * 3), ("mis_mode", C.c_int)]


def make_light(center=(0, 0, 5), radius=1.0, radiance=(1, 1, 1), mis_mode=0) -> Light:
    lt = Light()
    lt.center[:] = center
    lt.radius = radius
    lt.radiance[:] = radiance
    lt.mis_mode = mis_mode
    return lt


def light_array(lights):
    """one Light, a sequence of them or None -> (ctypes array or None, count)"""
    if lights is None:
        return None, 0
    if isinstance(lights, Light):
        lights = [lights]
    lights = list(lights)
    if not lights:
        return None, 0
    return (Light * len(lights))(*lights), len(lights)


class GgxShaderSoa(C.Structure):
    _fields_ = [("Kd_color", CV3P), ("Kd", fp), ("Kd_roughness", fp), ("Ks", fp), ("Kt_color", CV3P), ("Kt", fp)]


class GgxShadeOutSoa(C.Structure):
    _fields_ = [(k, CV3P) for k in ("direct_diffuse", "direct_specular", "refraction", "indirect_diffuse", "indirect_specular", "out")]


class DisneyShadeOutSoa(C.Structure):
    _fields_ = [(k, CV3P) for k in ("direct_diffuse", "direct_specular", "indirect_diffuse", "indirect_specular", "out")]


class DisneySoa(C.Structure):
    _fields_ = [("wo", CV3P), ("N", CV3P), ("T", CV3P), ("base_color", CV3P), ("scalars", fp * 10)]


class SssSoa(C.Structure):
    _fields_ = [("sss_scatter_dist", CV3P), ("sss_dist_multiplier", fp), ("sss_color", CV3P),
                ("N", CV3P), ("T", CV3P)]


class SkinSoa(C.Structure):
    _fields_ = [("wo", CV3P), ("N", CV3P), ("T", CV3P),
                ("sss_color", CV3P), ("sss_weight", fp), ("sss_dist_multiplier", fp), ("sss_scatter_dist", CV3P),
                ("specular_color", CV3P), ("specular_weight", fp), ("specular_roughness", fp), ("specular_ior", fp),
                ("sheen_color", CV3P), ("sheen_weight", fp), ("sheen_roughness", fp), ("sheen_ior", fp),
                ("xi", fp * 6)]


class SkinOutSoa(C.Structure):
    _fields_ = [("sheen_wi", CV3P), ("sheen_f", CV3P), ("sheen_pdf", fp), ("sheen_fresnel", fp),
                ("spec_wi", CV3P), ("spec_f", CV3P), ("spec_pdf", fp), ("spec_fresnel", fp),
                ("r", fp), ("r_pdf", fp), ("profile", CV3P),
                ("sheenFresnel", fp), ("specularFresnel", fp), ("sssWeight", fp)]


_lib = None


def build(force: bool = False) -> Path:
    if force or not LIB_PATH.exists() or LIB_PATH.stat().st_mtime < max(
            (ORACLE_DIR / "rls_oracle.c").stat().st_mtime, (ORACLE_DIR / "rls_oracle.h").stat().st_mtime):
        p = subprocess.run(["make", "-C", str(ORACLE_DIR)], capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"oracle build failed:\n{p.stdout}\n{p.stderr}")
    return LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        build()
        _lib = C.CDLL(str(LIB_PATH))
        _lib.orc_hardware_threads.restype = C.c_int
        _lib.orc_hash_u32.restype = C.c_uint32
        _lib.orc_hash_u32.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32]
        _lib.orc_hash_u01.restype = C.c_float
        _lib.orc_hash_u01.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32]
    return _lib


def hardware_threads() -> int:
    return int(lib().orc_hardware_threads())


def set_closure_alloc(on: bool) -> None:
    """orc_set_closure_alloc: orc_ggx_init pays the reference's per-closure heap allocation (src/rlGgx.h:152) or not."""
    lib().orc_set_closure_alloc(1 if on else 0)


def f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"], (a.dtype, a.flags)
    return a.ctypes.data_as(fp)


def _v(a: np.ndarray) -> CV3P:
    """[3, n] float32 array -> struct of three plane pointers"""
    assert a.ndim == 2 and a.shape[0] == 3 and a.dtype == np.float32 and a.strides[1] == 4, (a.shape, a.dtype)
    return CV3P(_p(a[0]), _p(a[1]), _p(a[2]))


def _full(v, n) -> np.ndarray:
    """broadcast a python scalar / array to a contiguous [n] float32 plane"""
    a = np.asarray(v, dtype=np.float32)
    if a.ndim == 0:
        return np.full(n, a, dtype=np.float32)
    assert a.shape == (n,), a.shape
    return f32(a)


def _full3(v, n) -> np.ndarray:
    a = np.asarray(v, dtype=np.float32)
    if a.ndim == 1:
        assert a.shape == (3,)
        return np.ascontiguousarray(np.repeat(a[:, None], n, axis=1))
    assert a.shape == (3, n), a.shape
    return f32(a)


# ------------------------------------------------------------------------------------------------
class Ggx:
    """oracle-side batch of rls::GgxSampler closures"""

    def __init__(self, wo, N, T, KsColor=(1, 1, 1), ior=1.0, roughness=0.0, anisotropic=0.0, exiting=None,
                 nthreads: int = 1):
        self.n = n = wo.shape[1]
        self.arr = dict(wo=f32(wo), N=f32(N), T=f32(T), Ks=_full3(KsColor, n), rough=_full(roughness, n),
                        ior=_full(ior, n), aniso=_full(anisotropic, n))
        self.exiting = None if exiting is None else np.ascontiguousarray(exiting, dtype=np.uint8)
        a = self.arr
        self.soa = GgxSoa(_v(a["wo"]), _v(a["N"]), _v(a["T"]), _v(a["Ks"]), _p(a["rough"]), _p(a["ior"]),
                          _p(a["aniso"]),
                          self.exiting.ctypes.data_as(C.POINTER(C.c_uint8)) if self.exiting is not None else None)
        self.nthreads = nthreads
        # light loops: False = the oracle's canonical estimator (one running sum), True = its second form with one sum per
        # strategy, the order the device kernels produce (rls_oracle.c, ggx_light_loop); the GPU parity tests set True
        self.two_sums_default = False

    def sample_eval_pdf(self, rx, ry):
        n = self.n
        rx, ry = f32(rx), f32(ry)
        wi, f = np.empty((3, n), np.float32), np.empty((3, n), np.float32)
        pdf, F = np.empty(n, np.float32), np.empty(n, np.float32)
        lib().orc_batch_ggx_sample_eval_pdf(C.c_int64(n), C.byref(self.soa), _p(rx), _p(ry), _v(wi), _v(f), _p(pdf),
                                            _p(F), self.nthreads)
        return wi, f, pdf, F

    def sample(self, rx, ry):
        n = self.n
        rx, ry = f32(rx), f32(ry)
        wi, F = np.empty((3, n), np.float32), np.empty(n, np.float32)
        lib().orc_batch_ggx_sample(C.c_int64(n), C.byref(self.soa), _p(rx), _p(ry), _v(wi), _p(F), self.nthreads)
        return wi, F

    def eval(self, wi):
        n = self.n
        wi = f32(wi)
        f = np.empty((3, n), np.float32)
        lib().orc_batch_ggx_eval(C.c_int64(n), C.byref(self.soa), _v(wi), _v(f), self.nthreads)
        return f

    def pdf(self, wi):
        n = self.n
        wi = f32(wi)
        pdf = np.empty(n, np.float32)
        lib().orc_batch_ggx_pdf(C.c_int64(n), C.byref(self.soa), _v(wi), _p(pdf), self.nthreads)
        return pdf

    def refract(self, rx, ry):
        n = self.n
        rx, ry = f32(rx), f32(ry)
        wt, w = np.empty((3, n), np.float32), np.empty(n, np.float32)
        flag = np.empty(n, np.uint8)
        lib().orc_batch_ggx_refract(C.c_int64(n), C.byref(self.soa), _p(rx), _p(ry), _v(wt), _p(w),
                                    flag.ctypes.data_as(C.POINTER(C.c_uint8)), self.nthreads)
        return wt, w, flag

    def reflect_refract(self, rx, ry, rx2, ry2, out=None):
        n = self.n
        rx, ry, rx2, ry2 = f32(rx), f32(ry), f32(rx2), f32(ry2)
        if out is None:
            out = (np.empty((3, n), np.float32), np.empty((3, n), np.float32), np.empty(n, np.float32),
                   np.empty(n, np.float32), np.empty((3, n), np.float32), np.empty(n, np.float32))
        wi, f, pdf, F, wt, w = out
        lib().orc_batch_ggx_reflect_refract(C.c_int64(n), C.byref(self.soa), _p(rx), _p(ry), _p(rx2), _p(ry2),
                                            _v(wi), _v(f), _p(pdf), _p(F), _v(wt), _p(w), self.nthreads)
        return out

    def microfacet(self, rx, ry, ndf_kernel=False):
        n = self.n
        rx, ry = f32(rx), f32(ry)
        m = np.empty((3, n), np.float32)
        lib().orc_batch_ggx_microfacet(C.c_int64(n), C.byref(self.soa), _p(rx), _p(ry), _v(m), int(ndf_kernel),
                                       self.nthreads)
        return m

    def ndf_pdf(self, wi):
        n = self.n
        wi = f32(wi)
        pdf = np.empty(n, np.float32)
        lib().orc_batch_ggx_ndf_pdf(C.c_int64(n), C.byref(self.soa), _v(wi), _p(pdf), self.nthreads)
        return pdf

    def direct_lighting(self, P, light, spp_n, seed, Kd_color=(1, 1, 1), Kd=1.0, Kd_roughness=0.0, Ks=1.0,
                        first_index=0, two_sums=None):
        """orc_batch_ggx_direct_lighting (one Light or a sequence) -> (direct_diffuse [3,n], direct_specular [3,n]).
        two_sums: the estimator with one sum per strategy (the device kernels' order) instead of the canonical running sum"""
        n = self.n
        P = f32(P)
        kdc, kd, kdr, ks = _full3(Kd_color, n), _full(Kd, n), _full(Kd_roughness, n), _full(Ks, n)
        sh = GgxShaderSoa(_v(kdc), _p(kd), _p(kdr), _p(ks), CV3P(), None)
        dd, ds = np.empty((3, n), np.float32), np.empty((3, n), np.float32)
        la, nl = light_array(light)
        two_sums = self.two_sums_default if two_sums is None else two_sums
        fn = lib().orc_batch_ggx_direct_lighting_two_sums if two_sums else lib().orc_batch_ggx_direct_lighting
        fn(C.c_int64(n), C.byref(self.soa), C.byref(sh), _v(P), la, nl, int(spp_n), C.c_uint32(seed), C.c_uint64(first_index),
           _v(dd), _v(ds), self.nthreads)
        return dd, ds

    def shade(self, P, lights, spp_n, seed, Kd_color=(1, 1, 1), Kd=0.5, Kd_roughness=0.0, Ks=0.5, Kt_color=(1, 1, 1), Kt=0.0,
              env=(1.0, 1.0, 1.0), traced=True, first_index=0, two_sums=None) -> dict:
        """orc_batch_ggx_shade -> dict of the five AOVs and out, [3,n] each (two_sums: see direct_lighting)"""
        n = self.n
        P = f32(P)
        kdc, kd, kdr, ks = _full3(Kd_color, n), _full(Kd, n), _full(Kd_roughness, n), _full(Ks, n)
        ktc, kt = _full3(Kt_color, n), _full(Kt, n)
        sh = GgxShaderSoa(_v(kdc), _p(kd), _p(kdr), _p(ks), _v(ktc), _p(kt))
        keys = ("direct_diffuse", "direct_specular", "refraction", "indirect_diffuse", "indirect_specular", "out")
        out = {k: np.empty((3, n), np.float32) for k in keys}
        o = GgxShadeOutSoa(*[_v(out[k]) for k in keys])
        la, nl = light_array(lights)
        e = (C.c_float * 3)(*[float(v) for v in env])
        two_sums = self.two_sums_default if two_sums is None else two_sums
        fn = lib().orc_batch_ggx_shade_two_sums if two_sums else lib().orc_batch_ggx_shade
        fn(C.c_int64(n), C.byref(self.soa), C.byref(sh), _v(P), la, nl, e, 1 if traced else 0,
           int(spp_n), C.c_uint32(seed), C.c_uint64(first_index), C.byref(o), self.nthreads)
        return out

    def integrate_refract(self, spp_n, seed, traced=True, env=(1.0, 1.0, 1.0), first_index=0):
        """orc_batch_ggx_integrate_refract -> (result [3,n], tir_fraction [n])"""
        n = self.n
        res, tir = np.empty((3, n), np.float32), np.empty(n, np.float32)
        e = (C.c_float * 3)(*[float(v) for v in env])
        lib().orc_batch_ggx_integrate_refract(C.c_int64(n), C.byref(self.soa), 1 if traced else 0, e, int(spp_n),
                                              C.c_uint32(seed), C.c_uint64(first_index), _v(res), _p(tir), self.nthreads)
        return res, tir

    def integrate(self, spp_n, seed, first_index=0):
        n = self.n
        s, a = np.empty((3, n), np.float32), np.empty(n, np.float32)
        lib().orc_batch_ggx_integrate(C.c_int64(n), C.byref(self.soa), int(spp_n), C.c_uint32(seed),
                                      C.c_uint64(first_index), _v(s), _p(a), self.nthreads)
        return s, a


class Disney:
    def __init__(self, wo, N, T, base_color=(1, 1, 1), nthreads: int = 1, **scalars):
        self.n = n = wo.shape[1]
        self.arr = dict(wo=f32(wo), N=f32(N), T=f32(T), base=_full3(base_color, n))
        self.sc = [_full(scalars.get(k, 0.0), n) for k in DISNEY_SCALARS]
        a = self.arr
        self.soa = DisneySoa(_v(a["wo"]), _v(a["N"]), _v(a["T"]), _v(a["base"]), (fp * 10)(*[_p(s) for s in self.sc]))
        self.nthreads = nthreads
        self.two_sums_default = False           # see Ggx

    def sample(self, lobe, rx, ry):
        n = self.n
        rx, ry = f32(rx), f32(ry)
        wi = np.empty((3, n), np.float32)
        lib().orc_batch_disney_sample(C.c_int64(n), C.byref(self.soa), lobe, _p(rx), _p(ry), _v(wi), self.nthreads)
        return wi

    def eval(self, lobe, wi):
        n = self.n
        wi = f32(wi)
        f = np.empty((3, n), np.float32)
        lib().orc_batch_disney_eval(C.c_int64(n), C.byref(self.soa), lobe, _v(wi), _v(f), self.nthreads)
        return f

    def pdf(self, lobe, wi):
        n = self.n
        wi = f32(wi)
        pdf = np.empty(n, np.float32)
        lib().orc_batch_disney_pdf(C.c_int64(n), C.byref(self.soa), lobe, _v(wi), _p(pdf), self.nthreads)
        return pdf

    def sample_eval_pdf(self, lobe, rx, ry):
        n = self.n
        rx, ry = f32(rx), f32(ry)
        wi, f, pdf = np.empty((3, n), np.float32), np.empty((3, n), np.float32), np.empty(n, np.float32)
        lib().orc_batch_disney_sample_eval_pdf(C.c_int64(n), C.byref(self.soa), lobe, _p(rx), _p(ry), _v(wi), _v(f),
                                               _p(pdf), self.nthreads)
        return wi, f, pdf

    def alt(self, kind, rx=None, ry=None, v=None):
        """kind 0/1: alternate microfacet samplers -> [3,n]; 2: non-VNDF pdf(v); 3: D_GTR2(v) -> [n]"""
        n = self.n
        out3, out1 = np.zeros((3, n), np.float32), np.zeros(n, np.float32)
        rx = f32(rx) if rx is not None else out1
        ry = f32(ry) if ry is not None else out1
        v = f32(v) if v is not None else out3
        lib().orc_batch_disney_alt(C.c_int64(n), C.byref(self.soa), int(kind), _p(rx), _p(ry), _v(v), _v(out3),
                                   _p(out1), self.nthreads)
        return out3 if kind < 2 else out1

    def direct_lighting(self, P, light, spp_n, seed, first_index=0, two_sums=None):
        """orc_batch_disney_direct_lighting (one Light or a sequence) -> (direct_diffuse [3,n], direct_specular [3,n]).
        two_sums: the estimator with one sum per strategy (the device kernels' order) instead of the canonical running sum"""
        n = self.n
        P = f32(P)
        dd, ds = np.empty((3, n), np.float32), np.empty((3, n), np.float32)
        la, nl = light_array(light)
        two_sums = self.two_sums_default if two_sums is None else two_sums
        fn = lib().orc_batch_disney_direct_lighting_two_sums if two_sums else lib().orc_batch_disney_direct_lighting
        fn(C.c_int64(n), C.byref(self.soa), _v(P), la, nl, int(spp_n), C.c_uint32(seed), C.c_uint64(first_index), _v(dd), _v(ds),
           self.nthreads)
        return dd, ds

    def shade(self, P, lights, spp_n, seed, env=(1.0, 1.0, 1.0), first_index=0, two_sums=None) -> dict:
        """orc_batch_disney_shade -> dict of the four AOVs and out, [3,n] each (two_sums: see direct_lighting)"""
        n = self.n
        P = f32(P)
        keys = ("direct_diffuse", "direct_specular", "indirect_diffuse", "indirect_specular", "out")
        out = {k: np.empty((3, n), np.float32) for k in keys}
        o = DisneyShadeOutSoa(*[_v(out[k]) for k in keys])
        la, nl = light_array(lights)
        e = (C.c_float * 3)(*[float(v) for v in env])
        two_sums = self.two_sums_default if two_sums is None else two_sums
        fn = lib().orc_batch_disney_shade_two_sums if two_sums else lib().orc_batch_disney_shade
        fn(C.c_int64(n), C.byref(self.soa), _v(P), la, nl, e, int(spp_n), C.c_uint32(seed), C.c_uint64(first_index), C.byref(o),
           self.nthreads)
        return out

    def integrate(self, spp_n, seed, streamed=False, first_index=0):
        n = self.n
        spp = spp_n * spp_n
        out = dict(diffuse_sum=np.empty((3, n), np.float32), diffuse_count=np.empty(n, np.float32),
                   specular_sum=np.empty((3, n), np.float32), specular_count=np.empty(n, np.float32))
        if streamed:
            m = 2 * spp * n
            out.update(wi=np.empty((3, m), np.float32), f=np.empty((3, m), np.float32), pdf=np.empty(m, np.float32))
            swi, sf, spdf = _v(out["wi"]), _v(out["f"]), _p(out["pdf"])
        else:
            swi, sf, spdf = CV3P(), CV3P(), None
        lib().orc_batch_disney_integrate(C.c_int64(n), C.byref(self.soa), int(spp_n), C.c_uint32(seed),
                                         C.c_uint64(first_index), _v(out["diffuse_sum"]), _p(out["diffuse_count"]),
                                         _v(out["specular_sum"]), _p(out["specular_count"]), swi, sf, spdf,
                                         self.nthreads)
        return out


class Sss:
    def __init__(self, n, dist, albedo=(1, 1, 1), multiplier=None, N=None, T=None, has_dPdu=True, nthreads: int = 1):
        self.n = n
        self.dist = _full3(dist, n)
        self.albedo = _full3(albedo, n)
        self.mult = None if multiplier is None else _full(multiplier, n)
        self.N = None if N is None else f32(N)
        self.T = None if T is None else f32(T)
        self.has_dPdu = int(has_dPdu)
        self.soa = SssSoa(_v(self.dist), _p(self.mult) if self.mult is not None else None, _v(self.albedo),
                          _v(self.N) if self.N is not None else CV3P(), _v(self.T) if self.T is not None else CV3P())
        self.nthreads = nthreads

    def nd_sample(self, rx):
        n = self.n
        rx = f32(rx)
        r, pdf, prof = np.empty(n, np.float32), np.empty(n, np.float32), np.empty((3, n), np.float32)
        lib().orc_batch_nd_sample_pdf_profile(C.c_int64(n), C.byref(self.soa), _p(rx), _p(r), _p(pdf), _v(prof),
                                              self.nthreads)
        return r, pdf, prof

    def nd_pdf(self, r):
        n = self.n
        r = f32(r)
        pdf = np.empty(n, np.float32)
        lib().orc_batch_nd_pdf(C.c_int64(n), C.byref(self.soa), _p(r), _p(pdf), self.nthreads)
        return pdf

    def nd_profile(self, r):
        n = self.n
        r = f32(r)
        prof = np.empty((3, n), np.float32)
        lib().orc_batch_nd_profile(C.c_int64(n), C.byref(self.soa), _p(r), _v(prof), self.nthreads)
        return prof

    def probe(self, rx, ry):
        n = self.n
        rx, ry = f32(rx), f32(ry)
        out = dict(r=np.empty(n, np.float32), origin=np.empty((3, n), np.float32), dir=np.empty((3, n), np.float32),
                   maxdist=np.empty(n, np.float32), pdf=np.empty(n, np.float32), profile=np.empty((3, n), np.float32))
        lib().orc_batch_sss_probe(C.c_int64(n), C.byref(self.soa), self.has_dPdu, _p(rx), _p(ry), _p(out["r"]),
                                  _v(out["origin"]), _v(out["dir"]), _p(out["maxdist"]), _p(out["pdf"]),
                                  _v(out["profile"]), self.nthreads)
        return out

    def mis_pdf(self, disp, sampleN, literal=False):
        n = self.n
        disp, sampleN = f32(disp), f32(sampleN)
        pdf = np.empty(n, np.float32)
        lib().orc_batch_sss_mis_pdf(C.c_int64(n), C.byref(self.soa), self.has_dPdu, _v(disp), _v(sampleN),
                                    int(literal), _p(pdf), self.nthreads)
        return pdf


class Scene(C.Structure):
    """orc_scene (same layout as rls_sss_scene)."""
    _fields_ = [("geometry", C.c_int),
                ("plane_point", C.c_float * 3), ("plane_normal", C.c_float * 3),
                ("sphere_center", C.c_float * 3), ("sphere_radius", C.c_float),
                ("light_dir", C.c_float * 3), ("light_color", C.c_float * 3),
                ("has_gate", C.c_int),
                ("gate_point", C.c_float * 3), ("gate_normal", C.c_float * 3),
                ("use_cavity_fade", C.c_int), ("literal_matrix", C.c_int)]


def make_scene(geometry="plane", plane_point=(0, 0, 0), plane_normal=(0, 0, 1), sphere_center=(0, 0, 0),
               sphere_radius=1.0, light_dir=(0, 0, 1), light_color=(1, 1, 1), gate_point=None, gate_normal=(1, 0, 0),
               use_cavity_fade=False, literal_matrix=False) -> Scene:
    sc = Scene()
    sc.geometry = {"plane": 0, "sphere": 1}[geometry]
    sc.plane_point[:] = plane_point
    sc.plane_normal[:] = plane_normal
    sc.sphere_center[:] = sphere_center
    sc.sphere_radius = sphere_radius
    sc.light_dir[:] = light_dir
    sc.light_color[:] = light_color
    sc.has_gate = int(gate_point is not None)
    sc.gate_point[:] = gate_point if gate_point is not None else (0, 0, 0)
    sc.gate_normal[:] = gate_normal
    sc.use_cavity_fade = int(use_cavity_fade)
    sc.literal_matrix = int(literal_matrix)
    return sc


def scene_trace(scene: Scene, O, D, maxdist):
    """orc_scene_trace -> (count, t[2], hitP[2][3], hitN[2][3])"""
    t = (C.c_float * 2)()
    hp, hn = (V3 * 2)(), (V3 * 2)()
    fn = lib().orc_scene_trace
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(Scene), V3, V3, C.c_float, fp, C.POINTER(V3), C.POINTER(V3)]
    k = fn(C.byref(scene), V3(*map(float, O)), V3(*map(float, D)), float(maxdist), t, hp, hn)
    return k, [t[i] for i in range(k)], [(hp[i].x, hp[i].y, hp[i].z) for i in range(k)], \
        [(hn[i].x, hn[i].y, hn[i].z) for i in range(k)]


def integrate_scatter(sss: "Sss", P, scene: Scene, spp_n, seed, first_index=0):
    """orc_batch_sss_integrate_scatter -> (result [3,n], mean_depth [n])"""
    n = sss.n
    P = f32(P)
    result, depth = np.empty((3, n), np.float32), np.empty(n, np.float32)
    lib().orc_batch_sss_integrate_scatter(C.c_int64(n), C.byref(sss.soa), sss.has_dPdu, _v(P), C.byref(scene),
                                          int(spp_n), C.c_uint32(seed), C.c_uint64(first_index), _v(result), _p(depth),
                                          sss.nthreads)
    return result, depth


def cavity_fade(disp, sampleN, No, nthreads=1):
    disp, sampleN, No = f32(disp), f32(sampleN), f32(No)
    n = disp.shape[1]
    out = np.empty(n, np.float32)
    lib().orc_batch_sss_cavity_fade(C.c_int64(n), _v(disp), _v(sampleN), _v(No), _p(out), nthreads)
    return out


def sample_diffuse_direction(normal, T, rx, ry, nthreads=1):
    normal, T, rx, ry = f32(normal), f32(T), f32(rx), f32(ry)
    n = normal.shape[1]
    wi = np.empty((3, n), np.float32)
    lib().orc_batch_sss_sample_diffuse(C.c_int64(n), _v(normal), _v(T), _p(rx), _p(ry), _v(wi), nthreads)
    return wi


def reflect_luminance(i, nrm, color):
    n = i.shape[1]
    i, nrm, color = f32(i), f32(nrm), f32(color)
    r, lum = np.empty((3, n), np.float32), np.empty(n, np.float32)
    lib().orc_batch_reflect_luminance(C.c_int64(n), _v(i), _v(nrm), _v(color), _v(r), _p(lum))
    return r, lum


def util_directions(a, b, nthreads=1):
    a, b = f32(a), f32(b)
    n = a.shape[0]
    sph, disk = np.empty((3, n), np.float32), np.empty((3, n), np.float32)
    lib().orc_batch_util(C.c_int64(n), _p(a), _p(b), _v(sph), _v(disk), nthreads)
    return sph, disk


SKIN_VEC = ("sheen_wi", "sheen_f", "spec_wi", "spec_f", "profile")
SKIN_SCALAR = ("sheen_pdf", "sheen_fresnel", "spec_pdf", "spec_fresnel", "r", "r_pdf",
               "sheenFresnel", "specularFresnel", "sssWeight")


class SkinIntOutSoa(C.Structure):
    _fields_ = [("sheen", CV3P), ("specular", CV3P), ("sss", CV3P), ("out", CV3P),
                ("sheenFresnel", fp), ("specularFresnel", fp), ("sssWeight", fp)]


def _skin_soa(wo, N, T, params: dict, xi):
    n = wo.shape[1]
    a = dict(wo=f32(wo), N=f32(N), T=f32(T),
             sss_color=_full3(params["sss_color"], n), sss_weight=_full(params["sss_weight"], n),
             mult=_full(params["sss_dist_multiplier"], n), dist=_full3(params["sss_scatter_dist"], n),
             spec_color=_full3(params["specular_color"], n), spec_w=_full(params["specular_weight"], n),
             spec_r=_full(params["specular_roughness"], n), spec_i=_full(params["specular_ior"], n),
             sheen_color=_full3(params["sheen_color"], n), sheen_w=_full(params["sheen_weight"], n),
             sheen_r=_full(params["sheen_roughness"], n), sheen_i=_full(params["sheen_ior"], n))
    xs = [np.ascontiguousarray(f32(xi)[k]) for k in range(6)] if xi is not None else []
    soa = SkinSoa(_v(a["wo"]), _v(a["N"]), _v(a["T"]), _v(a["sss_color"]), _p(a["sss_weight"]), _p(a["mult"]),
                  _v(a["dist"]), _v(a["spec_color"]), _p(a["spec_w"]), _p(a["spec_r"]), _p(a["spec_i"]),
                  _v(a["sheen_color"]), _p(a["sheen_w"]), _p(a["sheen_r"]), _p(a["sheen_i"]),
                  (fp * 6)(*[_p(x) for x in xs]) if xs else (fp * 6)())
    return soa, (a, xs)


def skin_integrate(wo, N, T, params: dict, P, scene: "Scene", spp_n, seed, env=(1.0, 1.0, 1.0), first_index=0,
                   nthreads=1, lights=None) -> dict:
    """orc_batch_skin_integrate -> dict(sheen, specular, sss, out [3,n]; sheenFresnel, specularFresnel, sssWeight [n])"""
    n = wo.shape[1]
    soa, keep = _skin_soa(wo, N, T, params, None)
    P = f32(P)
    out = {k: np.empty((3, n), np.float32) for k in ("sheen", "specular", "sss", "out")}
    out.update({k: np.empty(n, np.float32) for k in ("sheenFresnel", "specularFresnel", "sssWeight")})
    o = SkinIntOutSoa(_v(out["sheen"]), _v(out["specular"]), _v(out["sss"]), _v(out["out"]),
                      _p(out["sheenFresnel"]), _p(out["specularFresnel"]), _p(out["sssWeight"]))
    e = (C.c_float * 3)(*[float(v) for v in env])
    la, nl = light_array(lights)
    lib().orc_batch_skin_integrate(C.c_int64(n), C.byref(soa), _v(P), C.byref(scene), e, la, nl, int(spp_n),
                                   C.c_uint32(seed), C.c_uint64(first_index), C.byref(o), nthreads)
    return out


def skin(wo, N, T, params: dict, xi, nthreads=1) -> dict:
    n = wo.shape[1]
    a = dict(wo=f32(wo), N=f32(N), T=f32(T),
             sss_color=_full3(params["sss_color"], n), sss_weight=_full(params["sss_weight"], n),
             mult=_full(params["sss_dist_multiplier"], n), dist=_full3(params["sss_scatter_dist"], n),
             spec_color=_full3(params["specular_color"], n), spec_w=_full(params["specular_weight"], n),
             spec_r=_full(params["specular_roughness"], n), spec_i=_full(params["specular_ior"], n),
             sheen_color=_full3(params["sheen_color"], n), sheen_w=_full(params["sheen_weight"], n),
             sheen_r=_full(params["sheen_roughness"], n), sheen_i=_full(params["sheen_ior"], n))
    xi = f32(xi)
    xs = [np.ascontiguousarray(xi[k]) for k in range(6)]
    soa = SkinSoa(_v(a["wo"]), _v(a["N"]), _v(a["T"]), _v(a["sss_color"]), _p(a["sss_weight"]), _p(a["mult"]),
                  _v(a["dist"]), _v(a["spec_color"]), _p(a["spec_w"]), _p(a["spec_r"]), _p(a["spec_i"]),
                  _v(a["sheen_color"]), _p(a["sheen_w"]), _p(a["sheen_r"]), _p(a["sheen_i"]),
                  (fp * 6)(*[_p(x) for x in xs]))
    out = {k: np.empty((3, n), np.float32) for k in SKIN_VEC}
    out.update({k: np.empty(n, np.float32) for k in SKIN_SCALAR})
    o = SkinOutSoa(_v(out["sheen_wi"]), _v(out["sheen_f"]), _p(out["sheen_pdf"]), _p(out["sheen_fresnel"]),
                   _v(out["spec_wi"]), _v(out["spec_f"]), _p(out["spec_pdf"]), _p(out["spec_fresnel"]),
                   _p(out["r"]), _p(out["r_pdf"]), _v(out["profile"]),
                   _p(out["sheenFresnel"]), _p(out["specularFresnel"]), _p(out["sssWeight"]))
    lib().orc_batch_skin(C.c_int64(n), C.byref(soa), C.byref(o), nthreads)
    return out


def sample_02(seed, index, dim_pair, s):
    """sample s of point `index`'s scrambled (0,2)-sequence (orc_sample_02) -> (rx, ry)"""
    rx, ry = C.c_float(), C.c_float()
    lib().orc_sample_02(C.c_uint32(seed), C.c_uint64(index), C.c_uint32(dim_pair), C.c_uint32(s), C.byref(rx), C.byref(ry))
    return rx.value, ry.value


def batch_sample_02(seed, first, n, dim_pair, s):
    """sample s of points first .. first + n - 1 (orc_batch_sample_02) -> (rx [n], ry [n])"""
    rx, ry = np.empty(n, np.float32), np.empty(n, np.float32)
    lib().orc_batch_sample_02(C.c_uint32(seed), C.c_uint64(first), C.c_int64(n), C.c_uint32(dim_pair), C.c_uint32(s),
                              _p(rx), _p(ry))
    return rx, ry


# ------------------------------------------------------------------------------------------------
def gen_frame(seed, first, n):
    wo, N, T = (np.empty((3, n), np.float32) for _ in range(3))
    lib().orc_gen_frame(C.c_uint32(seed), C.c_uint64(first), C.c_int64(n), _v(wo), _v(N), _v(T))
    return wo, N, T


def gen_uniform(seed, first, n, stream, lo=0.0, hi=1.0):
    out = np.empty(n, np.float32)
    lib().orc_gen_uniform(C.c_uint32(seed), C.c_uint64(first), C.c_int64(n), C.c_uint32(stream), C.c_float(lo),
                          C.c_float(hi), _p(out))
    return out


def gen_aniso(seed, first, n):
    out = np.empty(n, np.float32)
    lib().orc_gen_aniso(C.c_uint32(seed), C.c_uint64(first), C.c_int64(n), _p(out))
    return out


def gauss(dist_x, rx, nthreads=1):
    rx = f32(rx)
    n = rx.shape[0]
    d = _full(dist_x, n)
    r, pdf, prof = (np.empty(n, np.float32) for _ in range(3))
    lib().orc_batch_gauss(C.c_int64(n), _p(d), _p(rx), _p(r), _p(pdf), _p(prof), nthreads)
    return r, pdf, prof
