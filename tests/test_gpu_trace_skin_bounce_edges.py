"""GPU: the rlSkin bounce calls (rls_trace_skin_bounce_emit / _resolve) where their kernels' loops and tiles end, as
tests/test_gpu_trace_bounce_edges.py and tests/test_gpu_trace_node_edges.py hold the other nodes there.

  A. on a context of one workgroup per CU, n = 2.5 x compute_units x kBlock points (+ a ragged tail) give every new emit kernel (one
     lane per point) and the resolve (kBlock points a workgroup) two and a half grid rounds: the bits are the default context's;
  B. diffuse_shadow across the scan's and the compaction's tile edges, n = 2047, 2048, 2049, 3 x 2048 + 5, against chunked emits;
  C. every spp_n 1 .. 16 at n = P + 1 of skin_diffuse_emit_kernel's tile of P = kBlock points: rls_trace_ggx_direct_emit's rays;
  D. diffuse rays' points only at a tile's last lane, and only in one lane group of a wavefront;
  E. every written plane and scratch of exactly the documented size as views inside sentinel-filled buffers;
  F. hostile per-point inputs (tests/test_gpu_trace_node_edges.py, _poison_case): the queues are still the node emit's filtered
     and rls_trace_ggx_direct_emit's on the same planes, or both NaN;
  G. state bytes of 255."""
import numpy as np
import pytest
import torch

import trace_sss_util as U
from gpu_util import dev, host
from test_gpu_trace_node_edges import Padded, _poison_case, _rehouse, _with_group, one_block_per_cu  # noqa: F401
from test_gpu_trace_skin import ENVS, KBLOCK, KEYS, MIXED3, T, _mk_lights, _resolve  # noqa: F401
from test_gpu_trace_skin_bounce import (CAM, DIF, GLS, NS, Planned, _assert_diffuse_shadow, _assert_node_queues_filtered, _bounce,
                                        _node_hosts, _plan, _same_hosts, _shadow_host, _state, _unit)

pytestmark = pytest.mark.gpu

LIGHTS2 = MIXED3[:2]


def _hosts(q):
    h = _node_hosts(q)
    h["diffuse_shadow"] = _shadow_host(q.diffuse_shadow, specular=False)
    return h


def _nan_same(got, want, what):
    assert got.keys() == want.keys(), what
    for name in want:
        for plane, v in want[name].items():
            if v.dtype == np.float32:
                U.same_bits_or_both_nan(got[name][plane], v, (what, name, plane))
            else:
                assert got[name][plane].tobytes() == v.tobytes(), (what, name, plane)


# ---- A ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
def test_two_and_a_half_grid_rounds_of_every_skin_bounce_kernel(gpu, oracle, T, one_block_per_cu, fast):
    ctx = one_block_per_cu
    rnd = ctx.device_info()["compute_units"] * KBLOCK
    n, spp_n = 2 * rnd + rnd // 2 + 37, 2
    for c in (gpu, ctx):
        c.set_math_mode(fast)
    try:
        w1 = _with_group(1, lambda: Planned(T, ctx, oracle, n, LIGHTS2, spp_n))
        w0 = _with_group(1, lambda: Planned(T, gpu, oracle, n, LIGHTS2, spp_n))
        h1 = _hosts(w1.q)
        _same_hosts(h1, _hosts(w0.q), "emit vs the default context")
        assert h1["diffuse_shadow"]["offsets"][-1] > n // NS and h1["sheen_glossy"]["offsets"][-1] > n // NS
        cnt, tr, dvis = _unit(w0, ENVS[1])
        hits = w0.b.hits(w0.q)
        a = _resolve(w1.b, w1.q, tr, hits, diffuse_visibility=dvis)
        b = _resolve(w0.b, w0.q, tr, hits, diffuse_visibility=dvis)
        for k in KEYS:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert (b["sss"][:, w0.k == 4] > 0).mean() > 0.5
    finally:
        for c in (gpu, ctx):
            c.set_math_mode(False)


# ---- B ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2047, 2048, 2049, 3 * 2048 + 5])
def test_diffuse_shadow_across_scan_and_compaction_tile_edges(gpu, oracle, T, n):
    spp_n, first = 2, (1 << 36) + 5
    st = _plan(n)[1]
    st[:, 0::2] = np.array([[DIF], [1], [1], [0], [0]], np.uint8)            # every other point a diffuse ray's: many rays a tile
    whole = Planned(T, gpu, oracle, n, LIGHTS2, spp_n, first=first, st=st)
    hw = _shadow_host(whole.q.diffuse_shadow, specular=False)
    assert hw["offsets"][-1] > n
    cut = 1000
    parts = []
    for a, m in ((0, cut), (cut, n - cut)):
        case = dict(wo=whole.b.frame[0][:, a:a + m].copy(), N=whole.b.frame[1][:, a:a + m].copy(), T=whole.b.frame[2][:, a:a + m].copy(),
                    P=whole.b.Ph[:, a:a + m].copy(), params={k: np.ascontiguousarray(v[..., a:a + m]) for k, v in whole.b.p.items()})
        w = Planned(T, gpu, oracle, m, LIGHTS2, spp_n, first=first + a, st=st[:, a:a + m], case=case)
        parts.append(_shadow_host(w.q.diffuse_shadow, specular=False))
    for plane in ("dir", "maxdist", "weight", "kind", "sample"):
        assert hw[plane].tobytes() == np.concatenate([p[plane] for p in parts], axis=-1).tobytes(), plane
    assert np.array_equal(hw["point"], np.concatenate([parts[0]["point"], parts[1]["point"] + cut]))
    assert np.array_equal(hw["offsets"], np.concatenate([parts[0]["offsets"], parts[1]["offsets"][1:] + parts[0]["offsets"][-1]]))


# ---- C ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp_n", range(1, 17))
def test_diffuse_emit_at_every_spp_n_a_point_past_its_tile(gpu, oracle, T, spp_n):
    n = KBLOCK + 1
    st = _plan(n)[1]
    st[:, -1] = (DIF, 1, 1, 0, 0)                                             # the one point of the second tile
    w = _with_group(1, lambda: Planned(T, gpu, oracle, n, LIGHTS2, spp_n, st=st))
    got, on = _assert_diffuse_shadow(w)
    assert on[-1] and np.diff(got["offsets"])[-1] > 0


# ---- D ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,at", [(1, [KBLOCK - 1]), (1, [63, KBLOCK + 63]), (4, [17]), (16, [2]), (16, [KBLOCK // 16 - 1]), (64, [5])])
def test_diffuse_points_at_a_tiles_last_lane_and_in_one_lane_group(gpu, oracle, T, g, at):
    """all camera rays but the points `at`: at g = 1 the last lane of a wavefront or of a tile, at g = 4, 16 one lane group of a
    wavefront whose other groups skip the light loop's stores but run its ballots"""
    n, spp_n = 2 * KBLOCK + 3, 4
    st = np.zeros((5, n), np.uint8)
    st[0] = CAM
    for i in at:
        st[:, i] = (DIF, 1, 1, 0, 0)
    w = _with_group(g, lambda: Planned(T, gpu, oracle, n, MIXED3, spp_n, st=st))
    got, on = _assert_diffuse_shadow(w)
    cnt = np.diff(got["offsets"])
    assert on[at].all() and on.sum() == len(at) and (cnt[at] > 0).all() and cnt.sum() == cnt[at].sum()
    _assert_node_queues_filtered(w)


# ---- E ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nl,spp_n", [(1001, 2, 3), (5, 3, 16)])
def test_nothing_is_written_outside_what_the_caller_handed_over(gpu, oracle, T, n, nl, spp_n):
    specs = MIXED3[:nl]
    plain = Planned(T, gpu, oracle, n, specs, spp_n)
    cnt, tr, dvis = _unit(plain, ENVS[1])
    hits = plain.b.hits(plain.q)
    want = _resolve(plain.b, plain.q, tr, hits, diffuse_visibility=dvis)
    for share in (False, True):
        pad = Padded()
        E = T.SkinBounceQueues(gpu, n, nl, spp_n, share)
        shared = None
        if share:
            assert E.scratch.numel() == T.node_scratch_bytes(n, nl, spp_n)
            shared = E.scratch = pad.like(E.scratch, 67 * 256)
        for name in ("sheen_shadow", "specular_shadow", "sheen_glossy", "specular_glossy", "probes"):
            q = getattr(E, name)
            if not share and name != "probes":
                assert q._scratch.numel() == (T.shadow_scratch_bytes(n, nl, spp_n) if "shadow" in name else T.scratch_bytes(n, spp_n))
            _rehouse(T, q, pad, shared)
        d = E.diffuse_shadow                                     # weight_diffuse.r alone: no weight_specular planes to house
        assert d.capacity == n * nl * 2 * spp_n * spp_n and d._ws.numel() == 0
        assert share or d._scratch.numel() == T.shadow_scratch_bytes(n, nl, spp_n)
        d.offsets, d._dir, d._maxdist, d._wd, d._kind, d._point, d._sample = (pad.like(t) for t in (
            d.offsets, d._dir, d._maxdist, d._wd, d._kind, d._point, d._sample))
        d._scratch = pad.like(d._scratch, 67 * 256) if shared is None else shared
        c = d.q
        c.offsets, c.maxdist, c.kind, c.point, c.sample = (t.data_ptr() for t in (d.offsets, d._maxdist, d._kind, d._point, d._sample))
        c.dir = T.capi.Vec3(*[d._dir[k].data_ptr() for k in range(3)])
        c.weight_diffuse = T.capi.Rgb(d._wd[0].data_ptr(), None, None)
        c.scratch, c.scratch_bytes = d._scratch.data_ptr(), d._scratch.numel()
        E.sheenFresnel, E.specularFresnel, E.sssWeight = (pad.like(t) for t in (E.sheenFresnel, E.specularFresnel, E.sssWeight))
        out = {k: pad.empty((3, n), gpu.torch_device) for k in ("sheen", "specular", "sss", "out")}
        out.update({k: pad.empty((n,), gpu.torch_device) for k in ("sheenFresnel", "specularFresnel", "sssWeight")})
        E = _bounce(T, plain.b, plain.lights, spp_n, plain.state, queues=E, share=share)
        got = _resolve(plain.b, E, tr, hits, diffuse_visibility=dvis, out=out)
        torch.cuda.synchronize()
        pad.check((n, nl, spp_n, share))
        _same_hosts(_hosts(E), _hosts(plain.q), (share, "in padded buffers"))
        for k in KEYS:
            assert got[k].tobytes() == want[k].tobytes(), (share, k)


# ---- F ---------------------------------------------------------------------------------------------------------------------------
def test_hostile_per_point_inputs(gpu, oracle, T):
    n, spp_n = 40 * NS, 3
    clean = Planned(T, gpu, oracle, n, MIXED3, spp_n)
    case, dirty = _poison_case(dict(wo=clean.b.frame[0], N=clean.b.frame[1], T=clean.b.frame[2], P=clean.b.Ph, params=clean.b.p),
                               np.random.default_rng(3), n)
    assert 0.2 < dirty.mean() < 0.9
    for g in (1, 16):
        w = _with_group(g, lambda: Planned(T, gpu, oracle, n, MIXED3, spp_n, case=case))
        _assert_node_queues_filtered(w, same=_nan_same)
        got, on = _assert_diffuse_shadow(w, same=_nan_same)
        assert got["offsets"][-1] > 0
        # the clean points keep the clean batch's bytes
        hq, hc = _hosts(w.q), _hosts(clean.q)
        for k in ("sheenFresnel", "specularFresnel", "sssWeight"):
            assert hq["scalars"][k][~dirty].tobytes() == hc["scalars"][k][~dirty].tobytes(), k
        cnt, tr, dvis = _unit(w, ENVS[1])
        out = _resolve(w.b, w.q, tr, clean.b.hits(clean.q), diffuse_visibility=dvis)
        _, ctr, cdvis = _unit(clean, ENVS[1])
        ref = _resolve(clean.b, clean.q, ctr, clean.b.hits(clean.q), diffuse_visibility=cdvis)
        for k in KEYS:                                           # (the probe walk of a clean point reads clean hits)
            assert out[k][..., ~dirty].tobytes() == ref[k][..., ~dirty].tobytes(), k


# ---- G ---------------------------------------------------------------------------------------------------------------------------
def test_state_bytes_of_255(gpu, oracle, T):
    n, spp_n = 5 * NS, 2
    k = np.arange(n) % 5
    st = np.full((5, n), 255, np.uint8)
    st[0] = np.array([255, CAM, GLS, DIF, 0xFD], np.uint8)[k]    # every bit: a shadow ray; 0xFD: every bit but the shadow bit
    w = Planned(T, gpu, oracle, n, MIXED3, spp_n, st=st)
    hn, hq, walk = _assert_node_queues_filtered(w)
    got, on = _assert_diffuse_shadow(w)
    lit = k != 0
    assert not hq["sheen_shadow"]["offsets"].any() and not hq["specular_glossy"]["offsets"].any()      # Rr_gloss 255 > the depth
    assert np.array_equal(on, (k == 3) | (k == 4)) and (np.diff(got["offsets"])[on] > 0).all()
    assert hq["scalars"]["sssWeight"][lit].tobytes() == (np.asarray(w.b.p["sss_weight"], np.float32) * np.ones(n, np.float32))[lit].tobytes()
    assert not hq["scalars"]["sssWeight"][~lit].view(np.uint32).any()
    child = T.advance_state(gpu, w.q.diffuse_shadow, w.state, DIF)
    assert (host(child.Rr) == 255).all() and (host(child.Rr_diff) == 255).all()      # the counters saturate
