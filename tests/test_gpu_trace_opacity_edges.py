"""GPU: the four shadow-hit kernels (csrc_trace/rls_trace_opacity.hpp: ggx_opacity_kernel, disney_opacity_kernel,
skin_opacity_kernel, shadow_visibility_kernel) past one round of their grid-stride loops: on a context capped at one workgroup
per CU (tests/test_gpu_trace_node_edges.py, one_block_per_cu) 2.5 x compute_units x kBlock + 37 points / rays take two full rounds
and a partial third.  Held to the default context's bytes, whole, and to the numpy restatement (tests/trace_opacity_util.py) on
windows of 512 around every round boundary and the tail."""
import numpy as np
import pytest

import trace_opacity_util as U
from gpu_util import dev, host
from test_gpu_trace_node_edges import KBLOCK, T, one_block_per_cu  # noqa: F401

pytestmark = pytest.mark.gpu

TABLE, MAX_HITS = 37, 4


def _size(ctx):
    cu = ctx.device_info()["compute_units"]
    round_ = cu * KBLOCK                                          # one round of the capped grid (a multiple of 8 workgroups)
    return 5 * round_ // 2 + 37, round_


def _windows(n, round_):
    """512 points around each round boundary below n, and the last 512"""
    edges = [k * round_ for k in range(1, n // round_ + 1)]
    w = [(max(e - 256, 0), min(e + 256, n)) for e in edges] + [(max(n - 512, 0), n)]
    assert len(w) >= 3
    return w


def _inputs(n):
    rt = U.ray_types(5, n, "mix")
    ids = np.random.default_rng(6).integers(0, TABLE + 5, n).astype(np.int32)
    col = lambda k, *lead: U.values(40 + k, *lead, TABLE, hostile=True)
    pln = lambda k, *lead: U.values(50 + k, *lead, n, hostile=True)
    return rt, ids, col, pln


@pytest.mark.parametrize("verb", ["ggx", "disney", "skin"])
def test_the_opacity_kernels_over_several_rounds(gpu, one_block_per_cu, T, verb):
    n, round_ = _size(gpu)
    rt, ids, col, pln = _inputs(n)
    for form in ("planes", "materials"):
        v = pln if form == "planes" else col
        p = dict(ggx=dict(opacity=v(0), opacity_color=v(1, 3), KtColor=v(2, 3), Kt=v(3)), disney=dict(opacity=v(0, 3)),
                 skin=dict(opacity=v(0), opacity_color=v(1, 3)))[verb]
        incoming = pln(7, 3) if verb == "skin" else None
        got = []
        for ctx in (gpu, one_block_per_cu):
            kw = dict(ray_type=dev(rt), materials=(dev(ids), TABLE) if form == "materials" else None)
            if verb == "skin":
                kw["incoming"] = dev(incoming)
            got.append(host(getattr(T, verb + "_opacity")(ctx, n, **{k: dev(a) for k, a in p.items()}, **kw)))
        assert U.same_bits(got[1], got[0], nan_bits=True), (verb, form)
        for a, e in _windows(n, round_):
            sl = lambda x: x if form == "materials" else np.ascontiguousarray(x[..., a:e])
            kw = dict(ray_type=rt[a:e], ids=ids[a:e] if form == "materials" else None, count=TABLE)
            q = {k: sl(x) for k, x in p.items()}
            if verb == "ggx":
                want = U.ggx_opacity(e - a, q["opacity"], q["opacity_color"], q["KtColor"], q["Kt"], **kw)
            elif verb == "disney":
                want = U.disney_opacity(e - a, q["opacity"], **kw)
            else:
                want = U.skin_opacity(e - a, q["opacity"], q["opacity_color"], incoming=incoming[:, a:e], **kw)
            assert U.same_bits(got[1][:, a:e], want), (verb, form, a, e)


@pytest.mark.parametrize("indexed", [False, True], ids=["direct", "indexed"])
def test_the_fold_kernel_over_several_rounds(gpu, one_block_per_cu, T, indexed):
    rays, round_ = _size(gpu)
    stride = rays + 3
    count = U.counts(9, rays, MAX_HITS)
    base = U.values(10, 3, rays)
    if indexed:
        opacity = U.values(11, 3, TABLE, hostile=True)
        index = np.random.default_rng(12).integers(0, TABLE + 5, MAX_HITS * stride).astype(np.int32)
    else:
        opacity, index = U.values(11, 3, MAX_HITS * stride, hostile=True), None
    got = []
    for ctx in (gpu, one_block_per_cu):
        hits = T.ShadowHits(dev(count), dev(opacity), MAX_HITS, stride=stride, index=None if index is None else dev(index))
        got.append(host(T.shadow_visibility(ctx, rays, hits, base=dev(base))))
    assert U.same_bits(got[1], got[0], nan_bits=True)
    for a, e in _windows(rays, round_):
        # ray j of the window is ray a + j of the batch: its elements are k * stride + a + j
        sel = (np.arange(MAX_HITS)[:, None] * stride + np.arange(a, e)[None, :]).reshape(-1)
        want = U.fold(e - a, count[a:e], opacity if indexed else opacity[:, sel], MAX_HITS, e - a,
                      index=index[sel] if indexed else None, base=base[:, a:e])
        assert U.same_bits(got[1][:, a:e], want), (indexed, a, e)
