"""What the routing tests share (tests/test_gpu_trace_route*.py): the numpy restatement of rls_trace_route_hits, raw calls of the
five entry points over sentinel-guarded buffers, bin mixes, and the two-bounce path of host/example_trace_path.cpp through
rlshaders_amd.trace -- routed (route_hits / gather / scatter / fill_misses) or by torch indexing."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
_SRC = (ROOT / "rlshaders_amd" / "csrc_trace" / "rls_trace_route.hpp").read_text() + \
    (ROOT / "rlshaders_amd" / "csrc" / "rls_internal.hpp").read_text()
KBLOCK = int(re.search(r"#define RLS_BLOCK (\d+)", _SRC).group(1))
TILE = KBLOCK * int(re.search(r"constexpr int kRoutePer = (\d+);", _SRC).group(1))        # the partition tile, kRouteTile
assert (KBLOCK, TILE) == (256, 2048)
SIZES = (0, 1, 63, 64, 65, KBLOCK - 1, KBLOCK, KBLOCK + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
GUARD, FILL = 256, 0xA5
MIXES = ("one", "miss", "miss_values", "alternate", "last_lane", "every_second_tile", "runs", "uniform", "rare")


def reference(bin_, bins):
    """(order, offsets [bins + 2], slot) of rls_trace_route_hits, by numpy"""
    key = np.where(bin_ < bins, bin_, bins).astype(np.int64)
    order = np.argsort(key, kind="stable").astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=bins + 1))]).astype(np.int64)
    slot = np.empty(len(bin_), np.uint32)
    slot[order] = np.arange(len(bin_), dtype=np.uint32)
    return order, offsets, slot


def mix(name, rays, bins, seed=0):
    """uint8 [rays]: the bin of every ray under one of MIXES"""
    rng = np.random.default_rng([seed, rays, bins, MIXES.index(name)])
    k = np.arange(rays)
    last = bins - 1
    if name == "one":
        return np.full(rays, last, np.uint8)
    if name == "miss":
        return np.full(rays, 255, np.uint8)
    if name == "miss_values":                                       # every miss value beside the bins
        return rng.choice(np.array(list(range(bins)) + [bins, 17, 254, 255], np.uint8), rays)
    if name == "alternate":                                         # ray by ray through the bins and a miss
        return np.where(k % (bins + 1) == bins, 255, k % (bins + 1)).astype(np.uint8)
    if name == "last_lane":                                         # a bin whose only ray is a wavefront's last lane
        b = np.full(rays, 255 if bins == 1 else 0, np.uint8)
        if rays >= 64:
            b[64 * (rays // 64 // 2) + 63] = last
        return b
    if name == "every_second_tile":                                 # the last bin absent from the odd tiles
        b = rng.integers(0, bins + 1, rays)
        odd = (k // TILE) % 2 == 1
        b[odd & (b == last)] = bins
        return np.where(b == bins, 255, b).astype(np.uint8)
    if name == "runs":                                              # runs longer than a tile
        b = (k // (TILE + 300)) % (bins + 1)
        return np.where(b == bins, 255, b).astype(np.uint8)
    if name == "uniform":
        b = rng.integers(0, bins + 1, rays)
        return np.where(b == bins, 255, b).astype(np.uint8)
    assert name == "rare"                                           # 1 % in the last bin
    b = rng.integers(0, bins, rays) if bins > 1 else np.full(rays, 255)
    if bins > 1:
        b[b == last] = bins
        b = np.where(b == bins, 255, b)
    b[rng.random(rays) < 0.01] = last
    return b.astype(np.uint8)


class Guarded:
    """`count` elements of `dtype` on the device inside GUARD bytes of FILL on both sides, themselves filled with FILL"""

    def __init__(self, count, dtype):
        self.bytes = int(count) * np.dtype(dtype).itemsize
        self.dtype = dtype
        self.buf = torch.full((self.bytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD

    def get(self):
        """the elements; asserts that nothing was written outside them"""
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == FILL).all() and (h[GUARD + self.bytes:] == FILL).all(), "written outside the buffer"
        return h[GUARD:GUARD + self.bytes].copy().view(self.dtype)


def raw_route(T, ctx, bin_, bins, slot=True, scratch_extra=0):
    """rls_trace_route_hits over guarded buffers of exactly the sizes the header names -> (order, offsets, slot or None)"""
    rays = len(bin_)
    order, offsets = Guarded(rays, np.uint32), Guarded(bins + 2, np.int64)
    slots = Guarded(rays, np.uint32) if slot else None
    scratch = Guarded(T.route_scratch_bytes(rays, bins) + scratch_extra, np.uint8)
    dbin = torch.from_numpy(np.ascontiguousarray(bin_)).cuda() if rays else None
    r = T.HitRoutes_(bins, offsets.ptr, order.ptr, slots.ptr if slot else None, scratch.ptr, scratch.bytes)
    st = T.load().rls_trace_route_hits(ctx.handle, rays, dbin.data_ptr() if rays else None, C.byref(r))
    assert st == 0, (st, rays, bins)
    torch.cuda.synchronize()
    scratch.get()
    return order.get(), offsets.get(), slots.get() if slot else None


def hostile_words(seed, planes, count):
    """uint32 [planes, count]: random bit patterns with NaN payloads, -0, denormals and infinities among them"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 32, (planes, count), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000], np.uint32)
    at = rng.random((planes, count)) < 0.25
    w[at] = rng.choice(special, int(at.sum()))
    return w


# ---- host/example_trace_path.cpp through rlshaders_amd.trace ----------------------------------------------------------------------
SEED, HIT_SEED = 1234, 4321
LIGHTS = (dict(center=(-4.0, 2.0, 3.0), radius=1.0, radiance=(3.0, 2.0, 1.0)),
          dict(center=(6.0, 1.0, 2.0), radius=1.0, radiance=(1.0, 4.0, 2.0)))
SHADER = dict(KdColor=(0.7, 0.5, 0.2), Kd=0.8, diffuseRoughness=0.3, Ks=0.6, KtColor=(0.2, 0.9, 0.7), Kt=0.5)
GGX = dict(specColor=(0.9, 0.6, 0.3), roughness=0.4, ior=1.6, anisotropic=0.5)
DISNEY = dict(base_color=(0.8, 0.5, 0.3), subsurface=0.1, metallic=0.2, specular=0.5, specular_tint=0.1, roughness=0.35,
              anisotropic=0.3, sheen=0.2, sheen_tint=0.5, clearcoat=0.3, clearcoat_gloss=0.6)
DEPTHS = dict(total=4, diffuse=1, glossy=1, refraction=2)
ENV, DEEP = (0.25, 0.3, 0.4), (0.5, 0.4, 0.3)


def example_bins(rays):
    """example_trace_path.cpp, hit_bin"""
    h = ((np.arange(rays, dtype=np.uint64) * 2654435761) & 0xFFFFFFFF) >> 29
    return np.where(h < 3, 0, np.where(h < 6, 1, 255)).astype(np.uint8)


def two_bounces(ctx, n, spp_n, bins_of, via):
    """The camera batch, its glossy queue's hits split between an rlGgx and an rlDisney surface and the misses, each bin shaded
    under the advanced state, the camera batch resolved with the children's out in its glossy radiance.  via "route": the
    library's routing; "torch": boolean masks, x[:, idx] and index_copy_.  -> dict of numpy arrays"""
    import rlshaders_amd as R
    from rlshaders_amd import trace as T
    from rlshaders_amd.closures import make_light
    dev = ctx.torch_device
    lights = [make_light(**kw) for kw in LIGHTS]
    uniform = lambda v, count: torch.tensor(v, dtype=torch.float32, device=dev)[:, None].repeat(1, max(int(count), 1)).contiguous()
    wo, N, Tn = R.gen_frame(ctx, SEED, 0, n)
    g = R.GgxSampler(ctx, wo, N, Tn, **GGX)
    camera = T.RayState.camera(ctx, n)
    nq = T.ggx_bounce_rays(g, T.ggx_shader(g, **SHADER), torch.zeros(3, n, device=dev), lights, spp_n, SEED, camera, DEPTHS)
    rays = nq.glossy.count
    hits = T.advance_state(ctx, nq.glossy, camera, T.RLS_RT_GLOSSY)
    bin_ = torch.from_numpy(bins_of(rays)).to(dev)
    frame = list(R.gen_frame(ctx, HIT_SEED, 0, rays)) + [torch.zeros(3, rays, device=dev)]          # wo, N, T, P per ray
    L = torch.zeros(3, nq.glossy.capacity, device=dev)
    got = {"rays": rays}

    def shade(b, wo_b, N_b, T_b, P_b, state):
        m = wo_b.shape[1]
        if b == 0:
            s = R.GgxSampler(ctx, wo_b, N_b, T_b, **GGX)
            q = T.ggx_bounce_rays(s, T.ggx_shader(s, **SHADER), P_b, lights, spp_n, SEED, state, DEPTHS, first_index=n)
        else:
            s = R.DisneySampler(ctx, wo_b, N_b, T_b, **DISNEY)
            q = T.disney_bounce_rays(s, P_b, lights, spp_n, SEED, state, DEPTHS, first_index=n, indirectDiffuseScale=0.5,
                                     indirectSpecularScale=0.25)
        assert q.n == m
        out = q.resolve(uniform((1.0, 1.0, 1.0), q.shadow.count), *[uniform(DEEP, getattr(q, r).count) for r in q.RAYS])
        for k in s.SHADE_AOVS:
            got[f"bin{b}_{k}"] = out[k].cpu().numpy()
        return out["out"]

    if via == "route":
        r = T.route_hits(ctx, bin_, 2)
        got["sizes"] = r.sizes()
        for b in (0, 1):
            out = shade(b, *r.gather(b, *frame), r.gather_state(b, hits))
            got[f"out{b}"] = out.cpu().numpy()
            r.scatter(b, out, L)
        r.fill_misses(ENV, L)
    else:
        key = torch.where(bin_ < 2, bin_, torch.full_like(bin_, 2))
        idx = [torch.nonzero(key == b).flatten() for b in range(3)]
        got["sizes"] = [int(i.shape[0]) for i in idx]
        for b in (0, 1):
            state = T.RayState(*[getattr(hits, k)[idx[b]].contiguous() for k in T.RayState.PLANES])
            out = shade(b, *[x[:, idx[b]].contiguous() for x in frame], state)
            got[f"out{b}"] = out.cpu().numpy()
            L.index_copy_(1, idx[b], out)
        L.index_copy_(1, idx[2], uniform(ENV, idx[2].shape[0])[:, :idx[2].shape[0]])
    got["radiance"] = L.cpu().numpy()
    out = nq.resolve(uniform((1.0, 1.0, 1.0), nq.shadow.count), L, uniform(DEEP, nq.refract.count), uniform(DEEP, nq.diffuse.count))
    for k in g.SHADE_AOVS + ("out",):
        got[k] = out[k].cpu().numpy()
    return got
