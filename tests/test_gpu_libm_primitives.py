"""GPU: the device-only instruction sequences of csrc/rls_libm.hpp -- rcp32_w, rcp32, rcp32_hi, div32_m, div32_const(_w),
div32_y, the unguarded sqrt32 behind sqrt32_1p / sqrt32_1m, exp32_in_range, exp32_in_range_3 -- and the two guarded
divisions of csrc/rls_device.hpp (ratio_to_one_minus, slope_y_ratio), each run on the device through the test-only probe
(tests/native/libm_device_probe.hip) against the IEEE operation it replaces.

Compiled for the host every one of them IS that IEEE operation, so the host builds of the header (tests/test_libm_faithful.py,
the "same source on host" arm of tools/libm_exhaustive.py) say nothing about them.  The reference here is numpy float32
arithmetic, cross-checked in float64 (tests/libm_probe_util.py); comparison is bit for bit, a NaN equals a NaN, signs of
zero and infinity count, and every generated argument is compared.  The sets: tests/libm_probe_util.py, args_*."""
import numpy as np
import pytest

import libm_probe_util as U

F = np.float32
pytestmark = pytest.mark.gpu


def _check(name, args, ref):
    n = args[0].size
    assert 0 < n <= U.CAP, (name, n)
    got = U.probe(name, *args)
    assert U.assert_same(got, ref, args, name) == n            # every generated argument compared


@pytest.mark.parametrize("name", ["rcp32_w", "rcp32", "rcp32_hi"])
def test_reciprocal(gpu, name):
    """rcp32_w inside 2^-126 .. 2^126 and on +-0, +-inf, NaN; rcp32 on any argument; rcp32_hi on 0, NaN and |x| >= 2^-126"""
    args = getattr(U, "args_" + name)()
    _check(name, args, U.ieee_rcp(args[0]))


@pytest.mark.parametrize("const", list(U.DIV_CONSTANTS))
def test_div32_const(gpu, const):
    """x / C, guarded: any x -- the subnormal binades, both sides of 2^-100 and 2^100, +-0, +-inf, NaN"""
    args = U.args_div32_const()
    _check("div32_const_" + const, args, U.ieee_div(args[0], np.full_like(args[0], U.DIV_CONSTANTS[const])))


@pytest.mark.parametrize("const", list(U.DIV_CONSTANTS))
def test_div32_const_w(gpu, const):
    """x / C without the range test: 2^-100 <= |x| <= 2^100"""
    args = U.args_div32_const_w()
    _check("div32_const_w_" + const, args, U.ieee_div(args[0], np.full_like(args[0], U.DIV_CONSTANTS[const])))


def test_div32_m(gpu):
    """Markstein's short division on the operands of its two uses in csrc/rls_device.hpp: (rx, 1 - rx) for rx in [2^-60, 1) and
    (num(u), den(u)) for every u the second slope can form -- 0 and [2^-24, 1].  For 0 < u <= 1.65e-34, which no random number
    produces, it is one ulp off IEEE division on some arguments (tests/libm_probe_util.py, set_u_window, has the figures)."""
    a, b = U.args_div32_m()
    _check("div32_m", (a, b), U.ieee_div(a, b))


def test_div32_y(gpu):
    """a / b through the kept reciprocal, over its whole operand window"""
    a, b = U.args_div32_y()
    _check("div32_y", (a, b), U.ieee_div(a, b))


def test_div32_y_negative_zero_numerator(gpu):
    """-0 / b: outside the IEEE guarantee (the sign comes out as +0 for b > 0); it must still be a zero"""
    a, b = U.args_div32_y_negative_zero()
    got = U.probe("div32_y", a, b)
    assert got.size == a.size and (got == 0).all()
    assert (U.bits(got[b < 0]) == 0).all()                     # -0 / negative = +0, as IEEE has it


def test_ratio_to_one_minus(gpu):
    """rx / (1 - rx): inside [2^-60, 1), and the plain division beyond its guard"""
    (rx,) = U.args_ratio_to_one_minus()
    with np.errstate(all="ignore"):
        den = U.f32(F(1.0) - rx)
    _check("ratio_to_one_minus", (rx,), U.ieee_div(rx, den))


def test_slope_y_ratio(gpu):
    """num(u) / den(u): on every u its call site can form (tests/libm_probe_util.py, set_u_window: 0 and [2^-24, 1]), and the
    plain division beyond its guard"""
    (u,) = U.args_slope_y_ratio()
    _check("slope_y_ratio", (u,), U.ieee_div(*U.slope_y_operands(u)))


def test_sqrt32_1p(gpu):
    (y,) = U.args_sqrt32_1p()
    with np.errstate(all="ignore"):
        rad = U.f32(F(1.0) + y)
    _check("sqrt32_1p", (y,), U.ieee_sqrt(rad))


def test_sqrt32_1m(gpu):
    (t,) = U.args_sqrt32_1m()
    with np.errstate(all="ignore"):
        rad = U.f32(F(1.0) - t)
    _check("sqrt32_1m", (t,), U.ieee_sqrt(rad))


def test_two_over(gpu):
    """2 / (1 + sqrtf(1 + B^2)), Smith's G1, as 2 * rcp32_w(den)"""
    (b2,) = U.args_two_over()
    with np.errstate(all="ignore"):
        den = U.f32(F(1.0) + U.ieee_sqrt(U.f32(F(1.0) + b2)))
    _check("two_over", (b2,), U.ieee_div(np.full_like(den, 2.0), den))


def test_exp32_in_range(gpu):
    """expf without its range tests, |x| < 88 and NaN: the host's expf (and the header's own host build)"""
    import cases
    (x,) = U.args_exp32_in_range()
    assert 0 < x.size <= U.CAP
    got = U.probe("exp32_in_range", x)
    port, libm = U.host_eval(U.HOST_FN["expf"], x)
    assert U.assert_same(got, port, (x,), "exp32_in_range against the same source on the host") == x.size
    assert np.isnan(got[np.isnan(x)]).all()
    if cases.strict_parity():
        assert U.assert_same(got, libm, (x,), "exp32_in_range against the host's expf") == x.size
    else:
        U.libm_rule("expf", got, libm, "exp32_in_range against the host's expf")


def test_exp32_in_range_3(gpu):
    a, b, c = U.args_exp32_in_range_3()
    _check("exp32_in_range_3", (a, b, c), U.ref_exp32_in_range_3(a, b, c))
