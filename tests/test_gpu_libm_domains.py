"""The elementary functions of csrc/rls_libm.hpp on the argument ranges the closures use them on, and beside every threshold
of their range cases (tests/libm_probe_util.py, THRESHOLDS / DOMAINS).  tests/test_gpu_libm.py strides through the 2^32 bit
patterns in chunks that start at k * 2^28: acosf never sees 7e-10 < |x| < 1 there, sinf / cosf one quadrant each side of zero,
expf [2, 3) and [-3, -2], logf nothing in (0.5, 1].

GPU (marked): rls_libm_eval against the two arms of tests/native/libm_host.cpp -- the same source compiled for the host: no
differing word, ever; the host libm: none where cases.strict_parity() holds, elsewhere the allowance tests/test_gpu_libm.py
gives sinf / cosf / expf / powf.
CPU (not marked): the generators alone -- inside their domains, every threshold present with its neighbours, within the
size cap -- and the host build of the header against the host libm on the same sets."""
import numpy as np
import pytest

import libm_probe_util as U

F = np.float32
NAMES = list(U.DOMAINS)
_SETS = {}


def _set(name):
    """the argument set of a function, generated once (sinf / cosf and their bounded forms share theirs)"""
    gen = U.DOMAINS[name][0]
    if gen not in _SETS:
        _SETS[gen] = gen()
    a = _SETS[gen]
    return a[0], (a[1] if len(a) > 1 else None)


def _host(name):
    key = ("host", name)
    if key not in _SETS:
        x, y = _set(name)
        _SETS[key] = U.host_eval(U.HOST_FN[name], x, y)
    return _SETS[key]


@pytest.mark.parametrize("name", NAMES)
def test_argument_sets(name):
    _, lo, hi, open_ends, must = U.DOMAINS[name]
    x, y = _set(name)
    assert 0 < x.size <= U.CAP and (y is None or y.size == x.size)
    assert not np.isnan(x).any() and (y is None or not np.isnan(y).any())
    assert ((x > lo) & (x < hi) if open_ends else (x >= lo) & (x <= hi)).all(), (name, float(x.min()), float(x.max()))
    if name == "logf":
        assert (x > 0).all()
    pool = x[y == F(5.0)] if name == "powf" else x
    if name == "powf":
        rest = y != F(5.0)
        assert (x[rest] > 0).all() and (x[rest] <= 1).all() and (y[rest] >= 0).all() and (y[rest] <= 1).all()
        a2 = U.gtr1_a2(np.array([0.0, 1.0], np.float32))
        assert np.isin(a2, x[rest]).all()
    present = set(U.bits(pool).tolist())
    for t in must:
        for v in ((t, -t) if lo < 0 else (t,)):
            nb = U.near(F(v))
            nb = nb[(nb > lo) & (nb < hi) if open_ends else (nb >= lo) & (nb <= hi)]
            if name == "logf":
                nb = nb[nb > 0]
            assert set(U.bits(nb).tolist()) <= present, (name, "threshold without its neighbours", v)
    if name == "atan2f":
        ratio_at_one = set(U.bits(np.abs(x[y == F(1.0)])).tolist())          # x here is atan2f's y: the quotient itself
        for t, _ in U.THRESHOLDS["atan2f"]:
            assert set(U.bits(U.near(F(t))).tolist()) <= ratio_at_one, t
        z = (x == 0) | (y == 0)
        assert z.any() and ((x == 0) & (y == 0)).any() and (np.abs(x) == np.abs(y)).any()
        for sx in (False, True):
            for sy in (False, True):
                assert ((np.signbit(x) == sx) & (np.signbit(y) == sy) & z).any()
    # every binade of the domain holds at least 2^12 arguments (or all it has)
    if name not in ("atan2f",):
        e_top = int(np.floor(np.log2(max(abs(lo), abs(hi))))) - 1
        expo = (U.bits(np.abs(pool)) >> 23).astype(np.int64) - 127
        for e in range(-126, e_top + 1):
            assert int((expo == e).sum()) >= U.PER_BINADE, (name, e)


@pytest.mark.parametrize("name", NAMES)
def test_host_build_matches_host_libm(name):
    """the header compiled for the host against the host libm, on the closures' ranges (tests/test_libm_faithful.py draws at random)"""
    x, _ = _set(name)
    port, libm = _host(name)
    assert port.size == x.size
    U.libm_rule(name, port, libm, f"{name}: host build of the header against the host libm")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_on_the_closures_ranges(gpu, name):
    import torch
    import rlshaders_amd as R
    x, y = _set(name)
    tx = torch.from_numpy(x).cuda()
    ty = None if y is None else torch.from_numpy(y).cuda()
    out = torch.full((x.size,), 12345.0, device="cuda", dtype=torch.float32)
    R._capi.check(gpu.lib.rls_libm_eval(gpu.handle, U.HOST_FN[name], x.size, tx.data_ptr(), None if ty is None else ty.data_ptr(),
                                        out.data_ptr()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    port, libm = _host(name)
    assert U.assert_same(got, port, (x, y), f"{name}: device against the same source on the host") == x.size
    U.libm_rule(name, got, libm, f"{name}: device against the host libm")
