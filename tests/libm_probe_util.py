"""Argument sets, references and bindings for the libm tests that run on the closures' own ranges:

* tests/test_gpu_libm_primitives.py -- the DEVICE-only instruction sequences of csrc/rls_libm.hpp (rcp32_w, div32_m, div32_y,
  ...) through the test-only probe tests/native/libm_device_probe.hip, against IEEE arithmetic in numpy float32;
* tests/test_gpu_libm_domains.py -- the elementary functions through rls_libm_eval, on the ranges the closures use them on
  and beside every threshold of their range cases, against the two arms of tests/native/libm_host.cpp.

Everything here is deterministic: the sets are edges (the first and last 64 mantissas of every binade, the 64 bit-pattern
neighbours each side of every threshold) plus a jittered stride whose jitter comes from a generator seeded by the binade."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
CAP = 1 << 22          # arguments per primitive / per function, at most
PER_BINADE = 1 << 12   # arguments per binade, at least (binades that hold fewer values are taken whole)
EDGE = 64              # mantissas at each end of a binade; neighbours each side of a threshold
NAN = F(np.nan)
INF = F(np.inf)


# ---- bit-pattern helpers ---------------------------------------------------------------------------------------------------
def f32(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32)


def bits(x) -> np.ndarray:
    return f32(x).view(np.uint32)


def from_bits(u) -> np.ndarray:
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def ubits(v) -> int:
    """the bit pattern of one fp32 value"""
    return int(bits(v).reshape(-1)[0])


def pow2(e: int) -> np.float32:
    return F(np.ldexp(1.0, e))


def step(v, k: int) -> np.float32:
    """the value k bit patterns away from v in magnitude (k < 0: towards zero); the sign of v is kept"""
    v = F(v)
    u = ubits(np.abs(v)) + k
    assert 0 <= u <= 0x7F800000, (v, k)
    r = from_bits(np.uint32(u))[0]
    return -r if np.signbit(v) else r


def near(v, k: int = EDGE, below: bool = True, above: bool = True) -> np.ndarray:
    """v with its k bit-pattern neighbours each side in magnitude (towards zero: below), the sign of v kept; stops at 0 and inf"""
    v = F(v)
    u = ubits(np.abs(v))
    off = np.arange(-k if below else 0, (k if above else 0) + 1, dtype=np.int64)
    uu = np.unique(np.clip(u + off, 0, 0x7F800000)).astype(np.uint32)
    r = from_bits(uu)
    return f32(-r) if np.signbit(v) else r


def binade(e: int, per: int = PER_BINADE) -> np.ndarray:
    """[2^e, 2^(e+1)), e in [-149, 127]: the first and last 64 values and a jittered stride through the rest, `per` in all"""
    assert -149 <= e <= 127
    base, width = ((e + 127) << 23, 1 << 23) if e >= -126 else (1 << (e + 149), 1 << (e + 149))
    if width <= per:
        idx = np.arange(width, dtype=np.int64)
    else:
        m = per - 2 * EDGE
        span = width - 2 * EDGE
        stride = span // m
        jitter = np.random.default_rng(1000 + e).integers(0, stride, m)
        idx = np.concatenate([np.arange(EDGE), EDGE + np.arange(m, dtype=np.int64) * stride + jitter,
                              width - EDGE + np.arange(EDGE)])
    return from_bits((base + idx).astype(np.uint32))


def binades(e_lo: int, e_hi: int, per: int = PER_BINADE) -> np.ndarray:
    """every binade [2^e, 2^(e+1)) for e_lo <= e <= e_hi"""
    return np.concatenate([binade(e, per) for e in range(e_lo, e_hi + 1)])


def both_signs(x) -> np.ndarray:
    x = f32(x)
    return np.concatenate([x, -x])


def cat(*parts) -> np.ndarray:
    return f32(np.concatenate([np.atleast_1d(f32(p)) for p in parts]))


def same(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """bit for bit; a NaN equals a NaN; the sign of zero and of infinity counts"""
    a, b = f32(a), f32(b)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def ulp_key(a: np.ndarray) -> np.ndarray:
    i = f32(a).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def assert_same(got, ref, args, what) -> int:
    """every argument compared; -> the number compared"""
    got, ref = f32(got), f32(ref)
    assert got.shape == ref.shape
    bad = ~same(got, ref)
    if bad.any():
        k = np.flatnonzero(bad)[:4]
        shown = [tuple(hex(ubits(a[i])) for a in args if a is not None) + (hex(ubits(got[i])), hex(ubits(ref[i])))
                 for i in k]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} results differ; first (arguments..., device, IEEE): {shown}")
    return int(bad.size)


# ---- the IEEE references ---------------------------------------------------------------------------------------------------
def ieee_div(a, b) -> np.ndarray:
    """RN(a / b) in numpy float32, cross-checked in float64: for fp32 operands float32(float64(a) / float64(b)) is the
    correctly rounded quotient (53 >= 2 * 24 + 2)"""
    a, b = f32(a), f32(b)
    with np.errstate(all="ignore"):
        q = f32(a / b)
        q64 = (a.astype(np.float64) / b.astype(np.float64)).astype(np.float32)
    assert same(q, q64).all(), "numpy's float32 division is not IEEE here"
    return q


def ieee_sqrt(x) -> np.ndarray:
    x = f32(x)
    with np.errstate(all="ignore"):
        s = f32(np.sqrt(x))
        s64 = np.sqrt(x.astype(np.float64)).astype(np.float32)
    assert same(s, s64).all(), "numpy's float32 square root is not IEEE here"
    return s


def ieee_rcp(x) -> np.ndarray:
    x = f32(x)
    return ieee_div(np.ones_like(x), x)


# ---- the host arms: tests/native/libm_host.cpp (the header compiled for the host, and the host libm) ----------------------------
HOST_FN = dict(sqrtf=0, div=1, atan2f=2, acosf=3, tanf=4, sinf=5, cosf=6, expf=7, logf=8, powf=9,
               tanf_bounded=10, sinf_bounded=11, cosf_bounded=12)
_HOST = None


def host_threads() -> int:
    return min(16, len(os.sched_getaffinity(0)))


def host_lib() -> C.CDLL:
    global _HOST
    if _HOST is None:
        out = ROOT / "tests" / "native" / "build"
        out.mkdir(exist_ok=True)
        so, src = out / "liblibm_host.so", ROOT / "tests" / "native" / "libm_host.cpp"
        hdr = ROOT / "rlshaders_amd" / "csrc" / "rls_libm.hpp"
        if not so.exists() or so.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
            subprocess.run(["g++", "-O2", "-std=gnu++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                            f"-I{hdr.parent}", str(src), "-o", str(so), "-lm"], check=True)
        _HOST = C.CDLL(str(so))
        fp = C.POINTER(C.c_float)
        _HOST.libm_host_eval.argtypes = [C.c_int, C.c_int64, fp, fp, fp, fp, C.c_int]
        _HOST.libm_host_eval.restype = None
    return _HOST


def host_eval(fn: int, x, y=None):
    """-> (the same source on the host, the host libm)"""
    fp = C.POINTER(C.c_float)
    x = f32(x)
    y = None if y is None else f32(y)
    port, libm = np.empty(x.size, np.float32), np.empty(x.size, np.float32)
    host_lib().libm_host_eval(fn, x.size, x.ctypes.data_as(fp), None if y is None else y.ctypes.data_as(fp),
                              port.ctypes.data_as(fp), libm.ctypes.data_as(fp), host_threads())
    return port, libm


def libm_rule(name: str, got: np.ndarray, libm: np.ndarray, what: str) -> None:
    """against the host libm: no differing result where cases.strict_parity() holds; elsewhere what tests/test_gpu_libm.py
    allows sinf / cosf / expf / powf (glibc's other build rounds ~1e-8 of their arguments the other way): at most
    max(2, n * 1e-6) results off by one ulp, and none for the other functions"""
    import cases
    bad = ~same(got, libm)
    n_bad = int(bad.sum())
    if cases.strict_parity() or name.split("_")[0] not in ("sinf", "cosf", "expf", "powf"):
        assert n_bad == 0, (what, n_bad, "of", bad.size, hex(ubits(got[bad][0])), hex(ubits(libm[bad][0])))
        return
    assert n_bad <= max(2, bad.size * 1e-6), (what, n_bad, bad.size)
    if n_bad:
        assert np.isfinite(got[bad]).all() and np.isfinite(libm[bad]).all(), what
        assert int(np.abs(ulp_key(got[bad]) - ulp_key(libm[bad])).max()) <= 1, what


# ---- the device probe ------------------------------------------------------------------------------------------------------
PROBE_FN = dict(rcp32_w=0, rcp32=1, rcp32_hi=2, div32_m=3,
                div32_const_3=4, div32_const_03333=5, div32_const_1m06666=6, div32_const_06666m03333=7,
                div32_const_w_3=8, div32_const_w_03333=9, div32_const_w_1m06666=10, div32_const_w_06666m03333=11,
                div32_y=12, sqrt32_1p=13, sqrt32_1m=14, two_over=15, exp32_in_range=16, exp32_in_range_3=17,
                ratio_to_one_minus=18, slope_y_ratio=19)
# the four divisors the kernels use, formed in fp32 as the kernels' source forms them
DIV_CONSTANTS = {"3": F(3.0), "03333": F(0.3333) - F(0.0), "1m06666": F(1.0) - F(0.6666), "06666m03333": F(0.6666) - F(0.3333)}
_PROBE = None


def probe_lib() -> C.CDLL:
    """tests/native/build/librls_libm_probe.so (rlshaders_amd.build.build_libm_probe: the product's flags); RLS_LIBM_PROBE_LIB
    names another build of it (the probe against a mutated copy of the header, to see the tests fail)"""
    global _PROBE
    if _PROBE is None:
        path = Path(os.environ.get("RLS_LIBM_PROBE_LIB", str(ROOT / "tests" / "native" / "build" / "librls_libm_probe.so")))
        if not path.exists():          # a missing kernel is an error, and nothing is compiled behind a GPU test's back
            raise RuntimeError(f"the libm device probe is not built at {path}: rlshaders_amd.build.build_libm_probe() makes it")
        _PROBE = C.CDLL(str(path))
        _PROBE.rls_libm_probe.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _PROBE.rls_libm_probe.restype = C.c_int
    return _PROBE


def probe(name: str, a, b=None, c=None) -> np.ndarray:
    """one primitive on the device, one argument (pair, triple) per lane -> its results"""
    import torch
    ta = torch.from_numpy(f32(a)).cuda()
    tb = None if b is None else torch.from_numpy(f32(b)).cuda()
    tc = None if c is None else torch.from_numpy(f32(c)).cuda()
    assert all(t is None or t.numel() == ta.numel() for t in (tb, tc))
    out = torch.full((ta.numel(),), 12345.0, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    st = probe_lib().rls_libm_probe(PROBE_FN[name], ta.numel(), ta.data_ptr(), None if tb is None else tb.data_ptr(),
                                    None if tc is None else tc.data_ptr(), out.data_ptr(), None)
    assert st == 0, (name, "rls_libm_probe failed", st)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- argument sets of the primitives (part A) ---------------------------------------------------------------------------------
SPECIALS = f32([0.0, -0.0, np.inf, -np.inf, np.nan])
GUARDS = (-126, 126, -100, 100)        # the exponents of the guard constants of rcp32 / rcp32_hi / div32_const


def window(e_lo: int, e_hi: int) -> np.ndarray:
    """2^e_lo <= |x| <= 2^e_hi, both signs: every binade, and the upper end itself with its 64 inward neighbours"""
    return both_signs(cat(binades(e_lo, e_hi - 1), near(pow2(e_hi), above=False)))


def everything() -> np.ndarray:
    """any argument: every binade, subnormal ones included, both signs; 64 neighbours each side of every guard constant;
    +-0, +-inf, NaN"""
    return cat(both_signs(cat(binades(-149, 127), *[near(pow2(e)) for e in GUARDS])), SPECIALS)


def args_rcp32_w():
    return (cat(window(-126, 126), both_signs(near(pow2(-126), below=False)), SPECIALS),)


def args_rcp32():
    return (everything(),)


def args_rcp32_hi():
    x = everything()
    return (x[(x == 0) | np.isnan(x) | (np.abs(x) >= pow2(-126))],)      # its stated domain


def args_div32_const():
    return (everything(),)


def args_div32_const_w():
    return (cat(window(-100, 100), both_signs(near(pow2(-100), below=False))),)


def slope_y_operands(u):
    """num(u), den(u) of slope_y_ratio (csrc/rls_device.hpp), in the kernel's fp32 operation order"""
    u = f32(u)
    with np.errstate(all="ignore"):
        num = u * (u * (u * F(0.27385) - F(0.73369)) + F(0.46341))
        den = u * (u * (u * F(0.093073) + F(0.309420)) - F(1.0)) + F(0.597999)
    return f32(num), f32(den)


def set_rx_window() -> np.ndarray:
    """rx in [2^-60, 1): every binade; densely beside 2^-60, 0.5 and 1 - 2^-24"""
    lo, half, top = ubits(pow2(-60)), ubits(F(0.5)), ubits(F(1.0)) - 1
    dense = np.concatenate([lo + np.arange(1 << 12), half + np.arange(-(1 << 12), 1 << 12), top - np.arange(1 << 12)])
    return cat(binades(-60, -1), from_bits(dense.astype(np.uint32)))


def u_of_ry(ry) -> np.ndarray:
    """u = 2 |ry - 1/2| in the kernel's fp32 operation order (csrc/rls_device.hpp, vndf_slope_closed)"""
    ry = f32(ry)
    return f32(np.where(ry > F(0.5), F(2.0) * (ry - F(0.5)), F(2.0) * (F(0.5) - ry)))


U_MIN = -24     # the smallest positive u the call site forms is 2^-24 (below)


def set_u_window() -> np.ndarray:
    """The u the second slope divides for.  The call site forms u = 2 |ry - 1/2| from a random number ry in [0, 1]: both
    differences are exact multiples of 2^-25 (ulp(ry) >= 2^-25 on [1/4, 1]; below 1/4 the difference is rounded to that grid),
    so u is 0 or a multiple of 2^-24 in [2^-24, 1] -- never in (0, 2^-24).  The set: 0; every binade of [2^-24, 1] with
    arbitrary mantissas (a superset of what ry can produce); 1 with its inward neighbours; 2^18 evenly spaced values; and u
    of ry itself for ry over every binade of [0, 1], densely beside 1/2 and 1.
    (For 0 < u < 2^-113, which no ry produces, the numerator is below 2^-114 and the residuals of the short division are no
    longer representable: there it is NOT IEEE division -- measured on gfx950 over every binade of (0, 1), 2^12 arguments
    each: 4095 results off by one ulp, every one of them at u <= 1.65e-34, none above.)"""
    half = ubits(F(0.5))
    ry = cat(0.0, binades(-149, -1), 1.0, from_bits((half + np.arange(-(1 << 12), 1 << 12)).astype(np.uint32)),
             near(F(1.0), 1 << 12, above=False))
    return cat(0.0, binades(U_MIN, -1), near(F(1.0), above=False), np.linspace(0.0, 1.0, 1 << 18).astype(np.float32)[1:],
               u_of_ry(ry))


def args_div32_m():
    """the two uses csrc/rls_device.hpp makes of it: (rx, 1 - rx) and (num(u), den(u))"""
    rx = set_rx_window()
    num, den = slope_y_operands(set_u_window())
    return cat(rx, num), cat(F(1.0) - rx, den)


def args_ratio_to_one_minus():
    """inside the window, and both sides of the guard: below 2^-60 (zero and subnormals included), >= 1, negative, NaN"""
    out = cat(0.0, binades(-149, -61), near(pow2(-60)), near(F(1.0)), binades(0, 127), INF)
    return (cat(set_rx_window(), out, -out, NAN),)


def args_slope_y_ratio():
    """inside its window (set_u_window), and beyond its guard: u > 1 up to inf, NaN.  (Negative u pass the guard `u <= 1`
    and are not in the window: the call site forms an absolute value.)"""
    return (cat(set_u_window(), near(F(1.0), below=False), binades(0, 127), INF, NAN),)


def args_div32_y():
    """denominators over every binade of [2^-14, 2^14], numerators over [2^-75, 2^40], both signs of both, and exactly +0; the
    four corners of the window with their inward neighbours; a = s b and (s + 2^-23) b for small integers s"""
    b_all = window(-14, 14)
    a_all = window(-75, 40)
    rng = np.random.default_rng(4014)
    n = 1 << 21
    a = a_all[rng.permutation(np.arange(n) % a_all.size)]
    b = b_all[rng.permutation(np.arange(n) % b_all.size)]
    parts_a, parts_b = [a], [b]
    for ea, up_a in ((-75, True), (40, False)):
        for eb, up_b in ((-14, True), (14, False)):
            ca = near(pow2(ea), below=not up_a, above=up_a)
            cb = near(pow2(eb), below=not up_b, above=up_b)
            for sa in (1, -1):
                for sb in (1, -1):
                    parts_a.append(np.repeat(sa * ca, cb.size))
                    parts_b.append(np.tile(sb * cb, ca.size))
    bs = b_all[rng.permutation(b_all.size)[:1 << 14]]
    for s in range(1, 17):
        for sv in (F(s), step(F(s), 1)):       # s, and the next number above it (1 + 2^-23 for s = 1)
            parts_a.append(f32(sv * bs))
            parts_b.append(bs)
    zb = b_all[rng.permutation(b_all.size)[:1 << 14]]
    parts_a.append(np.zeros_like(zb))
    parts_b.append(zb)
    return cat(*parts_a), cat(*parts_b)


def args_div32_y_negative_zero():
    """a = -0 over denominators of the whole window.  The header excludes zero operands from the IEEE guarantee, and for -0
    it matters: -0 / b comes out as +0 for b > 0 (q0 = -0, the residual +0, their sum +0).  Every caller squares the
    quotient, feeds it to expf or subtracts 1 from it, so the tests hold it to "a zero", not to the sign."""
    b = window(-14, 14)
    return -np.zeros_like(b), b


def args_sqrt32_1p():
    """y over every binade of [-2, 2^127]; every y in (-1 - 2^-20, -1 + 2^-20) (1 + y tiny, zero or negative); 0, inf, NaN"""
    lo, hi = ubits(step(F(1.0) - pow2(-20), 1)), ubits(step(F(1.0) + pow2(-20), -1))
    beside = -from_bits(np.arange(lo, hi + 1, dtype=np.uint32))
    return (cat(binades(-149, 126), near(pow2(127), below=False, above=False), -binades(-149, 0), F(-2.0), beside, 0.0, -0.0,
                INF, NAN),)


def args_sqrt32_1m():
    """t over [0, 2.5] by binade; every t in (1 - 2^-12, 1 + 2^-12); anisotropic * 0.9f beside the value that makes it 1"""
    lo, hi = ubits(step(F(1.0) - pow2(-12), 1)), ubits(step(F(1.0) + pow2(-12), -1))
    top = binade(1)
    aniso = f32([0.0, 1.0, 1.111111, step(F(1.111111), 1), 1.2])
    return (cat(0.0, binades(-149, 0), top[top <= F(2.5)], near(F(2.5), above=False),
                from_bits(np.arange(lo, hi + 1, dtype=np.uint32)), aniso * F(0.9), NAN),)


def args_two_over():
    """B^2 of Smith's G1: 0, every binade up to 2^128, inf, NaN"""
    return (cat(0.0, binades(-149, 127), INF, NAN),)


def args_exp32_in_range():
    """|x| < 88: every binade down to the subnormals, both signs; 2^20 evenly spaced values of [-88, 0]; the 64 values
    below 88 and above -88; +-0; NaN"""
    top = binade(6)
    mag = cat(binades(-149, 5), top[top < F(88.0)], near(F(88.0), above=False)[:-1])
    dense = f32(np.linspace(-88.0, 0.0, 1 << 20).astype(np.float32))
    x = cat(both_signs(mag), dense[np.abs(dense) < F(88.0)], 0.0, -0.0)
    assert (np.abs(x) < F(88.0)).all()
    return (cat(x, NAN),)


def args_exp32_in_range_3():
    """triples around the bound: every combination of the special values, and ordinary values with one, two or three
    neighbours of +-88 among them"""
    sp = f32([0.0, -0.0, 1.0, -1.0, step(F(88.0), -1), 88.0, step(F(88.0), 1), -step(F(88.0), -1), -88.0, -step(F(88.0), 1),
              np.inf, -np.inf, np.nan, 1e-45, 3e38])
    g = np.stack(np.meshgrid(sp, sp, sp, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(88)
    n = 1 << 16
    edge = both_signs(near(F(88.0)))
    t = rng.uniform(-87.0, 87.0, (n, 3)).astype(np.float32)
    put = rng.integers(0, 2, (n, 3)).astype(bool)
    t[put] = edge[rng.integers(0, edge.size, int(put.sum()))]
    t = np.concatenate([g, t])
    return f32(t[:, 0]), f32(t[:, 1]), f32(t[:, 2])


def ref_exp32_in_range_3(a, b, c):
    """max(|a|, |b|, |c|) < 88 with NaNs ignored by the maximum, as csrc/rls_libm.hpp states it"""
    with np.errstate(all="ignore"):
        m = np.fmax(np.fmax(np.abs(a), np.abs(b)), np.abs(c))
        return f32(m < F(88.0))


# ---- the elementary functions on the closures' ranges (part B) ---------------------------------------------------------------
# Every threshold of a range case that the sets must straddle, once: (value, the line of csrc/rls_libm.hpp -- or of
# csrc/rls_device.hpp where said -- that it restates).  Multiples of pi are rounded to fp32 from the fp64 value.
PI = np.pi
# rls_libm.hpp:986-987 n = round(x * 2 / pi): the quadrant changes at the odd multiples of pi / 4 and the reduced argument
# passes through 0 at the even ones
SINCOS_STEP = PI / 4
THRESHOLDS = {
    "sincos": [(2.0 ** -12, "rls_libm.hpp:1023 |y| < 2^-12: sin = y, cos = 1"),
               (120.0, "rls_libm.hpp:981 |y| >= 120: reduce_large (outside the bounded forms)")],
    "tanf": [(float(from_bits(np.uint32(0x3F2CA140))[0]), "rls_libm.hpp:1117 |x| >= 0.67434: the reflected argument"),
             (float(from_bits(np.uint32(0x3F490FDA))[0]), "rls_libm.hpp:1109 |x| <= pi/4: no reduction"),
             (2.0 ** -13, "rls_libm.hpp:1124 reduced argument below 2^-13")],
    "acosf": [(0.5, "rls_libm.hpp:921 |x| < 0.5"), (1.0, "rls_libm.hpp:920 |x| >= 1 leaves acos32_q"),
              (2.0 ** -26, "rls_libm.hpp:929 z = (1 - |x|) / 2 >= 2^-26; as an argument: far inside |x| < 0.5"),
              (float(from_bits(np.uint32(0x23000000))[0]), "rls_libm.hpp:920 |x| <= 2^-57: pi/2"),
              (float(F(1.0) - F(1e-4)), "rls_device.hpp:301 v.z < 1 - 1e-4: the near-normal threshold")],
    "atan2f": [(7 / 16, "rls_libm.hpp:892 q < 7/16"), (11 / 16, "rls_libm.hpp:893"), (19 / 16, "rls_libm.hpp:893"),
               (39 / 16, "rls_libm.hpp:893"), (2.0 ** 25, "rls_libm.hpp:851 |x| >= 2^25: pi/2"),
               (2.0 ** -25, "rls_libm.hpp:887 exponents up to 27 apart stay in atan2_32_q"),
               (2.0 ** -28, "rls_libm.hpp:887 k + 27 < 0 leaves atan2_32_q"), (2.0 ** 24, "rls_libm.hpp:887 k > 23 leaves atan2_32_q"),
               (2.0 ** -29, "rls_libm.hpp:849 |x| < 2^-29: atanf returns its argument")],
    "expf": [(88.0, "rls_libm.hpp:582 |x| >= 88"), (-88.0, "rls_libm.hpp:582"),
             (float.fromhex("0x1.62e42ep6"), "rls_libm.hpp:585 overflow"), (-float.fromhex("0x1.9fe368p6"), "rls_libm.hpp:586 underflow"),
             (2.0 ** -54, "rls_device.hpp:1319 the smallest |q| of the NDProfile window")],
    "logf": [(1.0, "rls_libm.hpp:616 log(1) = +0"), (2.0 ** -126, "rls_libm.hpp:617 subnormal arguments are normalised")] +
            [(float(from_bits(np.uint32(0x3F330000 + (i << 19)))[0]), "rls_libm.hpp:624-625 table interval %d" % i) for i in range(17)],
    "powf": [(2.0 ** -25, "rls_libm.hpp:750 x < 2^-25 takes pow32"), (1.0, "rls_libm.hpp:750 x > 1 takes pow32")],
}


HALF_PI = float(step(F(PI / 2), EDGE))        # pi / 2 with its 64 neighbours above


def _multiples(step_, limit):
    k = np.arange(1, int(limit / step_) + 1)
    return f32((k * step_).astype(np.float32))


def _around(values) -> np.ndarray:
    return cat(*[near(v) for v in np.atleast_1d(values)])


def _clip(x, lo, hi, open_lo=False, open_hi=False):
    x = f32(x)
    keep = ((x > lo) if open_lo else (x >= lo)) & ((x < hi) if open_hi else (x <= hi))
    return f32(x[keep])


def _angles(limit: float, dense: int) -> np.ndarray:
    """[-limit, limit]: every binade, every multiple of pi/4 with its neighbours, the thresholds, evenly spaced values"""
    top_e = int(np.floor(np.log2(limit)))
    mag = cat(0.0, binades(-149, top_e), _around(_multiples(SINCOS_STEP, limit)), _around([v for v, _ in THRESHOLDS["sincos"]]))
    return cat(both_signs(mag), np.linspace(-limit, limit, dense).astype(np.float32))


def dom_sincos():
    lim = float(F(2 * PI))
    return (_clip(_angles(lim, 1 << 20), -lim, lim),)


def dom_sincos_bounded():
    return (_clip(_angles(120.0, 1 << 20), -120.0, 120.0, True, True),)


def _tan_extra(limit):
    odd = _multiples(PI / 2, limit)[::2]
    return cat(_around(odd), _around(_multiples(PI / 4, limit)), _around([v for v, _ in THRESHOLDS["tanf"]]))


def dom_tanf_first_quadrant() -> np.ndarray:
    lim = float(F(PI / 2))            # kHalfPi rounds to the same fp32
    x = cat(0.0, binades(-149, 0), _tan_extra(2.0), np.linspace(0.0, lim, 1 << 19).astype(np.float32))
    return _clip(x, 0.0, HALF_PI)


def dom_tanf():
    """the full-domain form: [0, pi / 2] (the closures' theta), then [-120, 120]"""
    return (cat(dom_tanf_first_quadrant(), dom_tanf_bounded()[0]),)


def dom_tanf_bounded():
    mag = cat(0.0, binades(-149, 6), _tan_extra(120.0), near(F(120.0), above=False))
    return (_clip(cat(both_signs(mag), np.linspace(-120, 120, 1 << 19).astype(np.float32)), -120.0, 120.0, True, True),)


def dom_acosf():
    mag = cat(0.0, binades(-149, -1), _around([v for v, _ in THRESHOLDS["acosf"]]))
    return (_clip(cat(both_signs(mag), np.linspace(-1, 1, 1 << 20).astype(np.float32)), -1.0, 1.0),)


def dom_atan2f():
    rng = np.random.default_rng(2002)
    xs = cat(1.0, f32(np.ldexp(rng.uniform(1.0, 2.0, 192), rng.integers(-20, 21, 192))))
    ys, xx = [], []
    for t, _ in THRESHOLDS["atan2f"]:
        for x in xs:
            y = near(F(t) * x)
            ys.append(y)
            xx.append(np.full(y.size, x, np.float32))
    y, x = cat(*ys), cat(*xx)
    # zeros against everything, equal magnitudes, and the unit square the closures' dot products live in
    m = cat(binades(-149, 127, 4 * EDGE), 1.0)
    z = np.zeros_like(m)
    sq = rng.uniform(-1.0, 1.0, (2, 1 << 18)).astype(np.float32)
    y = cat(y, z, m, z, m, sq[0])
    x = cat(x, m, z, z, m, sq[1])
    # both signs of both arguments
    return cat(y, -y, y, -y), cat(x, x, -x, -x)


def dom_expf():
    mag = cat(0.0, binades(-149, 6), _around([abs(v) for v, _ in THRESHOLDS["expf"]]))
    return (_clip(cat(both_signs(mag), np.linspace(-104, 89, 1 << 20).astype(np.float32)), -104.0, 89.0),)


def dom_logf():
    x = cat(binades(-149, 0), _around([v for v, _ in THRESHOLDS["logf"]]), 2.0, np.linspace(0, 2, 1 << 20).astype(np.float32))
    return (_clip(x, 0.0, 2.0, open_lo=True),)


def gtr1_a2(gloss) -> np.ndarray:
    """a2 of sampleGTR1Direction: lerp(clearcoat_gloss, 0.1, 0.001)^2 in the kernels' fp32 operation order"""
    g = f32(gloss)
    a = ((F(1.0) - g) * F(0.1)) + (F(0.001) * g)
    return f32(a * a)


def dom_powf():
    """y = 5 over [0, 1] (the Schlick weights); x in (0, 1] against y in [0, 1]: a2^(1 - xi) of GTR1 and every binade of x"""
    rng = np.random.default_rng(5005)
    x5 = _clip(cat(0.0, binades(-149, -1), _around([v for v, _ in THRESHOLDS["powf"]]),
                   np.linspace(0, 1, 1 << 19).astype(np.float32)), 0.0, 1.0)
    n = 1 << 19
    xi = cat(rng.uniform(0, 1, n - 4).astype(np.float32), 0.0, 1.0, pow2(-24), F(1.0) - pow2(-24))
    a2 = gtr1_a2(cat(rng.uniform(0, 1, n - 2).astype(np.float32), 0.0, 1.0))
    xb = cat(binades(-149, -1, 1 << 12), 1.0)
    yb = cat(rng.uniform(0, 1, xb.size - 2).astype(np.float32), 0.0, 1.0)
    return cat(x5, a2, xb), cat(np.full(x5.size, 5.0, np.float32), F(1.0) - xi, yb)


def _thr(key):
    return [v for v, _ in THRESHOLDS[key]]


# name -> (generator, lo, hi of the stated domain of the first argument (64 neighbours past an end where the issue lists the
# end itself as a threshold), whether the ends are excluded, the values the set must contain with their neighbours)
TWO_PI = float(F(2 * PI))
DOMAINS = {
    "sinf": (dom_sincos, -TWO_PI, TWO_PI, False, _thr("sincos") + list(_multiples(SINCOS_STEP, TWO_PI))),
    "cosf": (dom_sincos, -TWO_PI, TWO_PI, False, _thr("sincos") + list(_multiples(SINCOS_STEP, TWO_PI))),
    "sinf_bounded": (dom_sincos_bounded, -120.0, 120.0, True, _thr("sincos") + list(_multiples(SINCOS_STEP, 120.0))),
    "cosf_bounded": (dom_sincos_bounded, -120.0, 120.0, True, _thr("sincos") + list(_multiples(SINCOS_STEP, 120.0))),
    "tanf": (dom_tanf, -120.0, 120.0, True, _thr("tanf") + list(_multiples(PI / 2, 120.0)[::2])),
    "tanf_bounded": (dom_tanf_bounded, -120.0, 120.0, True, _thr("tanf") + list(_multiples(PI / 2, 120.0)[::2])),
    "acosf": (dom_acosf, -1.0, 1.0, False, _thr("acosf")),
    "atan2f": (dom_atan2f, -np.inf, np.inf, False, []),           # its thresholds are quotients: checked on the pairs with x = 1
    "expf": (dom_expf, -104.0, 89.0, False, _thr("expf")),
    "logf": (dom_logf, 0.0, 2.0, False, _thr("logf")),
    "powf": (dom_powf, 0.0, 1.0, False, _thr("powf")),          # on the y = 5 part
}
