"""helpers of the any-hit library's tests (test_nearest_any_statement.py, test_gpu_nearest_any*.py): any_np, the float32 numpy
statement of rls_nearest_any_hits (include/rlshaders_amd_nearest_any.h) -- every triangle against every ray through
nearest_util._candidate, no tree, two existence statements --, and the derived planes in float32 numpy.  The meshes and the ray
streams are nearest_util's.  pytest does not collect this module."""
from types import SimpleNamespace

import numpy as np

from nearest_util import F, NO_PRIM, _candidate, _ray_args

CLEAR, BLOCKED, VEILED = 0, 1, 2


def opaque_of(mesh, flags):
    """a triangle's class, bool [nt]: 1 without a table, else flags[min(surface_i, len - 1)] != 0, surface_i = 0 without surfaces"""
    if flags is None:
        return np.ones(mesh.nt, bool)
    flags = np.asarray(flags)
    s = np.zeros(mesh.nt, np.int64) if mesh.surface is None else mesh.surface.astype(np.int64)
    return flags[np.minimum(s, len(flags) - 1)] != 0


def flags_np(table):
    """rls_nearest_any_opaque: table float32 [3, surfaces] -> uint8 [surfaces], every channel exactly 1 (a NaN gives 0)"""
    t = np.asarray(table, F)
    return ((t[0] == F(1)) & (t[1] == F(1)) & (t[2] == F(1))).astype(np.uint8)


def any_np(mesh, o, d, m=None, skip=None, flags=None, base=None, ray=None, ids=None):
    """The statement: o, d float32 [3, M]; m float32 [M] or None (+inf); skip uint32 [M] or None (nothing): the skip OF EACH ENTRY
    (the caller has read `last` through the ids); flags uint8 [table] or None (every triangle opaque).  -> state uint8 [M] by
    entry, and by ray id (ray int [M] or None: the entry; ids: the planes' width, default M) visibility float32 [3, ids] and reach
    float32 [ids] with `written` bool [ids]: the ids of the entries; unwritten entries hold base (1) and 0."""
    o, d, M, m, skip = _ray_args(o, d, m, skip)
    opaque = opaque_of(mesh, flags)
    blocked, veiled = np.zeros(M, bool), np.zeros(M, bool)
    V = mesh.V
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(F)
        sign = np.signbit(inv)
        for i in range(mesh.nt):
            v0, v1, v2 = (V[int(k)] for k in mesh.tri[i])
            box, tri_hit, t, _, _ = _candidate(v0, v1, v2, o, d, inv, sign)
            cand = (skip != i) & box & tri_hit & (t > 0) & (t <= m)
            flag = bool(opaque[i])
            blocked |= cand & flag
            veiled |= cand & (not flag)
    state = np.where(blocked, BLOCKED, np.where(veiled, VEILED, CLEAR)).astype(np.uint8)
    return derived(state, m, base, ray, ids)


def derived(state, m, base=None, ray=None, ids=None):
    """the derived planes of given states: visibility_c[id] = b_c * 0 where state is 1, else b_c; reach[id] = m where state is 2,
    else +0 -- float32 numpy operations"""
    M = state.shape[0]
    ray = np.arange(M, dtype=np.int64) if ray is None else np.asarray(ray).astype(np.int64)
    ids = M if ids is None else int(ids)
    b = np.ones((3, ids), F) if base is None else np.array(base, F)[:, :ids]
    vis, reach, written = b.copy(), np.zeros(ids, F), np.zeros(ids, bool)
    with np.errstate(all="ignore"):
        bk = b[:, ray]
        vis[:, ray] = np.where(state == BLOCKED, (bk * F(0)).astype(F), bk)
    reach[ray] = np.where(state == VEILED, np.asarray(m, F), F(0))
    written[ray] = True
    return SimpleNamespace(state=state, visibility=vis, reach=reach, written=written)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
