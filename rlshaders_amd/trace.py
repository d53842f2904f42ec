"""Caller-traced rlGgx, rlDisney and rlSss integrators: emit the sample rays of integrateGlossy / integrateRefract (rlGgx)
or of one rlDisney lobe, trace them with your own tracer, resolve the radiance; or emit integrateScatter's probe rays
(rlSss), walk them through the object, resolve the hits (include/rlshaders_amd_trace.h, companion library
``librls_trace.so``).

    q = trace.glossy_rays(sampler, spp_n=4, seed=7)          # RayQueue: q.dir [3, count], q.weight [3, count], ...
    L = my_tracer(origins[q.point], q.dir)                   # [3, count] radiance, one per ray
    s = q.resolve(L)                                         # [3, n]: sum of L x f/pdf per point (rls_ggx_integrate's sum)

    d = trace.disney_rays(disney, RLS_RAY_DIFFUSE, 8, seed)  # one lobe per queue; q.resolve: rls_disney_integrate's
                                                             # diffuse_sum, d.valid_count its diffuse_count

    p = trace.sss_probe_rays(sss, P, spp_n=4, seed=7)        # ProbeQueue: p.origin, p.dir [3, rays], p.maxdist [rays]
    cnt, hP, hN, E = my_probe_walk(p.origin, p.dir, p.maxdist)   # hits [3, max_hits, rays], E before profile and fade
    res = p.resolve(cnt, hP, hN, E)                          # [3, n]: integrateScatter's result

    s = trace.ggx_shadow_rays(sampler, shader, P, lights, 4, 7)  # ShadowQueue: s.dir, s.maxdist, s.weight_specular, s.kind, ...
    vis = my_shadow_tracer(P[:, s.point], s.dir, s.maxdist)      # [3, count]: 1 unoccluded, 0 blocked
    dd, ds = s.resolve(vis)                                      # [3, n] each: rls_ggx_direct_lighting's AOVs, shadowed

    nq = trace.ggx_node_rays(sampler, shader, P, lights, 4, 7)   # GgxNodeQueues: the whole node's rays, nq.shadow, nq.glossy,
    aov = nq.resolve(vis, Lg, Lt, Ld)                            # nq.refract, nq.diffuse -> rls_ggx_shade's dict, traced

    hq = trace.sss_hit_rays(sss, P, p, cnt, hP, hN, lights, 2, 7, trace_diffuse=True)   # HitQueues: the shaded hits' shadow
    E = hq.resolve(vis, Ld)                                      # rays and diffuse ray -> the E of p.resolve, traced

    sq = trace.skin_node_rays(skin, P, lights, 4, 7)             # SkinNodeQueues: sheen_shadow, specular_shadow, sheen_glossy,
    aov = sq.resolve(vis_a, vis_b, La, Lb, cnt, hP, hN, E)       # specular_glossy, probes -> SkinShader.integrate's dict, traced

    st = trace.RayState.camera(ctx, n)                           # sg->Rt and the sg->Rr* counters per point
    bq = trace.ggx_bounce_rays(sampler, shader, P, lights, 4, 7, st, depths=(8, 2, 2, 4))   # the node under that state
    hits = trace.advance_state(ctx, bq.glossy, st, trace.RLS_RT_GLOSSY)                     # the state of those rays' hits
    kq = trace.skin_bounce_rays(skin, P, lights, 4, 7, st, depths=(8, 2, 2, 4))             # SkinBounceQueues: + diffuse_shadow
    aov = kq.resolve(vis_a, vis_b, La, Lb, cnt, hP, hN, E, diffuse_visibility=vis_d)        # rlSkin under that state

    o = trace.ggx_opacity(ctx, m, KtColor=tint, Kt=0.5, ray_type=hit_state)                 # sg->out_opacity at shadow rays' hits
    vis = trace.shadow_visibility(ctx, s.count, trace.ShadowHits(cnt, o, max_hits, index=hit_surface))   # -> s.resolve(vis)

    r = trace.route_hits(ctx, hit_bin, bins=2)                   # HitRoutes: the queue's rays split by the node they hit
    hP, hN, ids = r.gather(0, P_hit, N_hit, material_id)         # bin 0's hit data as a dense batch; r.gather_state(0, hits)
    r.scatter(0, child["out"], L); r.fill_misses(env, L)         # the children's out and the environment, back in ray order

``count`` is read from the device once (it synchronises); everything else stays asynchronous on the context's stream, so
``glossy_rays(..., queue=q)`` / ``q.resolve(L, out=...)`` with preallocated tensors can be recorded by ``ctx.capture()``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _capi as capi
from ._capi import RLS_RAY_DIFFUSE, RLS_RAY_GLOSSY, check
from .closures import (DisneySampler, GgxSampler, SssSampler, cvec3, light_array, material_index, param, param_rgb, plane,
                       rgb)

TRACE_LIB_PATH = capi._PKG / "lib" / "librls_trace.so"

RLS_RAY_TRANSMITTED = 0
RLS_RAY_TIR_MIRROR = 1


class RayQueue_(C.Structure):
    """rls_ray_queue"""
    _fields_ = [("capacity", C.c_int64), ("offsets", C.c_void_p), ("dir", capi.Vec3), ("weight", capi.Rgb),
                ("point", C.c_void_p), ("sample", C.c_void_p), ("kind", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


class ProbeQueue_(C.Structure):
    """rls_probe_queue"""
    _fields_ = [("capacity", C.c_int64), ("offsets", C.c_void_p), ("origin", capi.Vec3), ("dir", capi.Vec3),
                ("maxdist", C.c_void_p), ("point", C.c_void_p), ("sample", C.c_void_p)]


class ProbeHits_(C.Structure):
    """rls_probe_hits"""
    _fields_ = [("max_hits", C.c_int), ("stride", C.c_int64), ("count", C.c_void_p), ("P", capi.CVec3), ("N", capi.CVec3),
                ("irradiance", capi.CRgb)]


class ShadowQueue_(C.Structure):
    """rls_shadow_queue"""
    _fields_ = [("capacity", C.c_int64), ("offsets", C.c_void_p), ("dir", capi.Vec3), ("maxdist", C.c_void_p),
                ("weight_specular", capi.Rgb), ("weight_diffuse", capi.Rgb), ("kind", C.c_void_p), ("point", C.c_void_p),
                ("sample", C.c_void_p), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


class HitQueues_(C.Structure):
    """rls_hit_queues"""
    _fields_ = [("hit_capacity", C.c_int64), ("hit_count", C.c_void_p), ("hit_element", C.c_void_p), ("shadow", ShadowQueue_),
                ("diffuse", RayQueue_), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


RLS_MAX_PROBE_HITS = 12

# rls_shadow_queue.kind
RLS_SHADOW_LIGHT_MASK = 0x07
RLS_SHADOW_BSDF = 0x08
RLS_SHADOW_SPECULAR = 0x10
RLS_SHADOW_DIFFUSE = 0x20

_ctx, _i64, _vp = C.c_void_p, C.c_int64, C.c_void_p
_q = C.POINTER(RayQueue_)
_pq = C.POINTER(ProbeQueue_)
_sq = C.POINTER(ShadowQueue_)
_lights = C.POINTER(capi.SphereLight)


class GgxNodeQueues_(C.Structure):
    """rls_ggx_node_queues"""
    _fields_ = [("shadow", _sq), ("glossy", _q), ("refract", _q), ("diffuse", _q)]


class GgxNodeTraced_(C.Structure):
    """rls_ggx_node_traced"""
    _fields_ = [("visibility", capi.CRgb), ("glossy", capi.CRgb), ("refract", capi.CRgb), ("diffuse", capi.CRgb)]


class DisneyNodeQueues_(C.Structure):
    """rls_disney_node_queues"""
    _fields_ = [("shadow", _sq), ("diffuse", _q), ("specular", _q)]


class DisneyNodeTraced_(C.Structure):
    """rls_disney_node_traced"""
    _fields_ = [("visibility", capi.CRgb), ("diffuse", capi.CRgb), ("specular", capi.CRgb)]


class SkinNodeQueues_(C.Structure):
    """rls_skin_node_queues"""
    _fields_ = [("sheen_shadow", _sq), ("specular_shadow", _sq), ("sheen_glossy", _q), ("specular_glossy", _q), ("probes", _pq),
                ("sheenFresnel", C.c_void_p), ("specularFresnel", C.c_void_p), ("sssWeight", C.c_void_p)]


class SkinNodeTraced_(C.Structure):
    """rls_skin_node_traced"""
    _fields_ = [("sheen_visibility", capi.CRgb), ("specular_visibility", capi.CRgb), ("sheen_glossy", capi.CRgb),
                ("specular_glossy", capi.CRgb), ("hits", C.POINTER(ProbeHits_))]


# rls_ray_state.ray_type: sg->Rt
RLS_RT_CAMERA = 0x01
RLS_RT_SHADOW = 0x02
RLS_RT_REFLECTED = 0x04
RLS_RT_REFRACTED = 0x08
RLS_RT_DIFFUSE = 0x20
RLS_RT_GLOSSY = 0x40


class GiDepths_(C.Structure):
    """rls_gi_depths"""
    _fields_ = [("total", C.c_int), ("diffuse", C.c_int), ("glossy", C.c_int), ("refraction", C.c_int)]


class RayState_(C.Structure):
    """rls_ray_state"""
    _fields_ = [("ray_type", C.c_void_p), ("Rr", C.c_void_p), ("Rr_diff", C.c_void_p), ("Rr_gloss", C.c_void_p),
                ("Rr_refr", C.c_void_p)]


_state, _depths = C.POINTER(RayState_), C.POINTER(GiDepths_)

# rls_trace_skin_bounce_emit: the seed of integrateScatter's light loop at diffuse rays' points is seed ^ this
RLS_SKIN_DIFFUSE_SEED = 0x9E3779B9


class SkinBounceQueues_(C.Structure):
    """rls_skin_bounce_queues"""
    _fields_ = [("node", SkinNodeQueues_), ("diffuse_shadow", _sq)]


class SkinBounceTraced_(C.Structure):
    """rls_skin_bounce_traced"""
    _fields_ = [("node", SkinNodeTraced_), ("diffuse_visibility", capi.CRgb)]


class GgxOpacity_(C.Structure):
    """rls_ggx_opacity"""
    _fields_ = [("opacity", capi.Param), ("opacity_color", capi.ParamRgb), ("KtColor", capi.ParamRgb), ("Kt", capi.Param),
                ("materials", capi.MaterialIndex)]


class DisneyOpacity_(C.Structure):
    """rls_disney_opacity"""
    _fields_ = [("opacity", capi.ParamRgb), ("materials", capi.MaterialIndex)]


class SkinOpacity_(C.Structure):
    """rls_skin_opacity"""
    _fields_ = [("opacity", capi.Param), ("opacity_color", capi.ParamRgb), ("materials", capi.MaterialIndex)]


class ShadowHits_(C.Structure):
    """rls_shadow_hits"""
    _fields_ = [("max_hits", C.c_int), ("stride", C.c_int64), ("count", C.c_void_p), ("opacity", capi.CRgb),
                ("index", C.c_void_p), ("table_count", C.c_uint32)]


RLS_ROUTE_MAX_BINS, RLS_ROUTE_MAX_W32, RLS_ROUTE_MAX_U8 = 16, 24, 8


class HitRoutes_(C.Structure):
    """rls_hit_routes"""
    _fields_ = [("bins", C.c_int), ("offsets", C.c_void_p), ("order", C.c_void_p), ("slot", C.c_void_p),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


class RoutePlanes_(C.Structure):
    """rls_route_planes"""
    _fields_ = [("n_w32", C.c_int), ("n_u8", C.c_int), ("src_w32", C.c_void_p * RLS_ROUTE_MAX_W32),
                ("dst_w32", C.c_void_p * RLS_ROUTE_MAX_W32), ("src_u8", C.c_void_p * RLS_ROUTE_MAX_U8),
                ("dst_u8", C.c_void_p * RLS_ROUTE_MAX_U8)]


PROTOTYPES = {
    "rls_trace_scratch_bytes": (C.c_int, [_i64, C.c_int, C.POINTER(C.c_size_t)]),
    "rls_trace_ggx_glossy_emit": (C.c_int, [_ctx, _i64, C.POINTER(capi.GgxClosure), C.c_int, C.c_uint32, C.c_uint64, _q, _vp]),
    "rls_trace_ggx_refract_emit": (C.c_int, [_ctx, _i64, C.POINTER(capi.GgxClosure), C.c_int, C.c_uint32, C.c_uint64, _q, _vp]),
    "rls_trace_disney_emit": (C.c_int, [_ctx, _i64, C.POINTER(capi.DisneyClosure), C.c_int, C.c_int, C.c_uint32, C.c_uint64,
                                        _q, _vp]),
    "rls_trace_ggx_glossy_resolve": (C.c_int, [_ctx, _i64, _q, capi.CRgb, capi.Rgb]),
    "rls_trace_ggx_refract_resolve": (C.c_int, [_ctx, _i64, _q, C.c_int, capi.CRgb, capi.Rgb]),
    "rls_trace_sss_probe_emit": (C.c_int, [_ctx, _i64, C.POINTER(capi.SssClosure), capi.CVec3, C.c_int, C.c_uint32, C.c_uint64,
                                           _pq]),
    "rls_trace_sss_scatter_resolve": (C.c_int, [_ctx, _i64, C.POINTER(capi.SssClosure), capi.CVec3, C.c_int, _pq,
                                                C.POINTER(ProbeHits_), C.c_int, C.c_int, capi.Rgb, _vp]),
    "rls_trace_sss_hits_scratch_bytes": (C.c_int, [_i64, C.c_int, C.c_int, _i64, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "rls_trace_sss_hits_emit": (C.c_int, [_ctx, _i64, C.POINTER(capi.SssClosure), capi.CVec3, C.c_int, _pq,
                                          C.POINTER(ProbeHits_), capi.CVec3, C.c_int, _lights, C.c_int, C.c_int, C.c_int,
                                          C.c_uint32, C.c_uint64, C.POINTER(HitQueues_)]),
    "rls_trace_sss_hits_resolve": (C.c_int, [_ctx, C.POINTER(ProbeHits_), _lights, C.c_int, C.c_int, C.c_int,
                                             C.POINTER(HitQueues_), capi.CRgb, capi.CRgb, capi.Rgb]),
    "rls_trace_shadow_scratch_bytes": (C.c_int, [_i64, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "rls_trace_ggx_direct_emit": (C.c_int, [_ctx, _i64, C.POINTER(capi.GgxClosure), C.POINTER(capi.GgxShader), capi.CVec3,
                                            _lights, C.c_int, C.c_int, C.c_uint32, C.c_uint64, _sq]),
    "rls_trace_disney_direct_emit": (C.c_int, [_ctx, _i64, C.POINTER(capi.DisneyClosure), capi.CVec3, _lights, C.c_int,
                                               C.c_int, C.c_uint32, C.c_uint64, _sq]),
    "rls_trace_ggx_direct_resolve": (C.c_int, [_ctx, _i64, C.POINTER(capi.GgxClosure), C.POINTER(capi.GgxShader), _lights,
                                               C.c_int, C.c_int, _sq, capi.CRgb, capi.Rgb, capi.Rgb]),
    "rls_trace_disney_direct_resolve": (C.c_int, [_ctx, _i64, _lights, C.c_int, C.c_int, _sq, capi.CRgb, capi.Rgb, capi.Rgb]),
    "rls_trace_ggx_shade_emit": (C.c_int, [_ctx, _i64, C.POINTER(capi.GgxClosure), C.POINTER(capi.GgxShader), capi.CVec3,
                                           _lights, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint64,
                                           C.POINTER(GgxNodeQueues_)]),
    "rls_trace_ggx_shade_resolve": (C.c_int, [_ctx, _i64, C.POINTER(capi.GgxClosure), C.POINTER(capi.GgxShader), _lights,
                                              C.c_int, C.c_int, C.c_int, C.POINTER(GgxNodeQueues_),
                                              C.POINTER(GgxNodeTraced_), C.POINTER(capi.GgxShadeOut)]),
    "rls_trace_disney_shade_emit": (C.c_int, [_ctx, _i64, C.POINTER(capi.DisneyClosure), capi.CVec3, _lights, C.c_int,
                                              C.c_int, C.c_uint32, C.c_uint64, C.POINTER(DisneyNodeQueues_)]),
    "rls_trace_disney_shade_resolve": (C.c_int, [_ctx, _i64, _lights, C.c_int, C.c_int, C.POINTER(DisneyNodeQueues_),
                                                 C.POINTER(DisneyNodeTraced_), C.POINTER(capi.DisneyShadeOut)]),
    "rls_trace_ggx_bounce_emit": (C.c_int, [_ctx, _i64, C.POINTER(capi.GgxClosure), C.POINTER(capi.GgxShader), capi.CVec3,
                                            _lights, C.c_int, C.c_int, C.c_uint32, C.c_uint64, _state, _depths,
                                            C.POINTER(GgxNodeQueues_)]),
    "rls_trace_ggx_bounce_resolve": (C.c_int, [_ctx, _i64, C.POINTER(capi.GgxClosure), C.POINTER(capi.GgxShader), _lights,
                                               C.c_int, C.c_int, _state, _depths, C.POINTER(GgxNodeQueues_),
                                               C.POINTER(GgxNodeTraced_), C.POINTER(capi.GgxShadeOut)]),
    "rls_trace_disney_bounce_emit": (C.c_int, [_ctx, _i64, C.POINTER(capi.DisneyClosure), capi.CVec3, _lights, C.c_int,
                                               C.c_int, C.c_uint32, C.c_uint64, _state, _depths,
                                               C.POINTER(DisneyNodeQueues_)]),
    "rls_trace_disney_bounce_resolve": (C.c_int, [_ctx, _i64, C.POINTER(capi.DisneyClosure), capi.Param, capi.Param, _lights,
                                                  C.c_int, C.c_int, _state, _depths, C.POINTER(DisneyNodeQueues_),
                                                  C.POINTER(DisneyNodeTraced_), C.POINTER(capi.DisneyShadeOut)]),
    "rls_trace_ray_state_advance": (C.c_int, [_ctx, _i64, _vp, _state, C.c_int, _state]),
    "rls_trace_skin_emit": (C.c_int, [_ctx, _i64, C.POINTER(capi.SkinClosure), capi.CVec3, _lights, C.c_int, C.c_int, C.c_uint32,
                                      C.c_uint64, C.POINTER(SkinNodeQueues_)]),
    "rls_trace_skin_resolve": (C.c_int, [_ctx, _i64, C.POINTER(capi.SkinClosure), capi.CVec3, _lights, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.POINTER(SkinNodeQueues_), C.POINTER(SkinNodeTraced_),
                                         C.POINTER(capi.SkinIntegrateOut)]),
    "rls_trace_skin_bounce_emit": (C.c_int, [_ctx, _i64, C.POINTER(capi.SkinClosure), capi.CVec3, _lights, C.c_int, C.c_int,
                                             C.c_uint32, C.c_uint64, _state, _depths, C.POINTER(SkinBounceQueues_)]),
    "rls_trace_skin_bounce_resolve": (C.c_int, [_ctx, _i64, C.POINTER(capi.SkinClosure), capi.CVec3, _lights, C.c_int, C.c_int,
                                                C.c_int, C.c_int, _state, _depths, C.POINTER(SkinBounceQueues_),
                                                C.POINTER(SkinBounceTraced_), C.POINTER(capi.SkinIntegrateOut)]),
    "rls_trace_ggx_opacity": (C.c_int, [_ctx, _i64, C.POINTER(GgxOpacity_), _vp, capi.Rgb]),
    "rls_trace_disney_opacity": (C.c_int, [_ctx, _i64, C.POINTER(DisneyOpacity_), _vp, capi.Rgb]),
    "rls_trace_skin_opacity": (C.c_int, [_ctx, _i64, C.POINTER(SkinOpacity_), _vp, capi.CRgb, capi.Rgb]),
    "rls_trace_shadow_visibility": (C.c_int, [_ctx, _i64, C.POINTER(ShadowHits_), capi.CRgb, capi.Rgb]),
    "rls_trace_route_scratch_bytes": (C.c_int, [_i64, C.c_int, C.POINTER(C.c_size_t)]),
    "rls_trace_route_hits": (C.c_int, [_ctx, _i64, _vp, C.POINTER(HitRoutes_)]),
    "rls_trace_route_gather": (C.c_int, [_ctx, _i64, _vp, C.POINTER(RoutePlanes_)]),
    "rls_trace_route_scatter": (C.c_int, [_ctx, _i64, _vp, C.POINTER(RoutePlanes_)]),
    "rls_trace_route_fill": (C.c_int, [_ctx, _i64, _vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_float)]),
}

_lib = None


def load() -> C.CDLL:
    """Load (once) and prototype the companion library; RLSHADERS_AMD_TRACE_LIB overrides its path.  The product library is
    loaded first (the companion takes its contexts and error state from it)."""
    global _lib
    if _lib is None:
        _lib = capi.load_companion("rlshaders_amd.trace", TRACE_LIB_PATH, "RLSHADERS_AMD_TRACE_LIB", PROTOTYPES,
                                   "build_trace_library", first=(capi.load,))
    return _lib


def _radiance(t: torch.Tensor, count: int, what: str) -> "capi.CRgb":
    """one traced value per ray and channel: radiance, or a shadow ray's visibility"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.shape[0] != 3 or \
            t.shape[1] < count or t.stride(1) != 1:
        raise ValueError(f"{what}: expected a float32 CUDA tensor [3, >= {count}] with unit inner stride")
    return capi.CRgb(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())


def _points(P: torch.Tensor, n: int) -> "capi.CVec3":
    """sg->P per point; an empty batch reads none"""
    return cvec3(P, n, "P") if n > 0 else capi.CVec3(None, None, None)


def scratch_bytes(n: int, spp_n: int) -> int:
    b = C.c_size_t()
    check(load().rls_trace_scratch_bytes(int(n), int(spp_n), C.byref(b)))
    return int(b.value)


class RayQueue:
    """The sample rays of one emit over n points at spp_n^2 samples, point-major (CSR: point i's rays are
    [offsets[i], offsets[i+1])).  Planes are allocated for the full capacity n * spp_n^2; the properties below view the
    first ``count`` rays.  ``lobe`` (RLS_RAY_DIFFUSE / RLS_RAY_GLOSSY) makes it a queue of that rlDisney lobe; without it
    the queue is rlGgx's, glossy or (``refract``) refraction."""

    def __init__(self, ctx, n: int, spp_n: int, refract: bool = False, want_kind: bool = True, *, lobe: Optional[int] = None,
                 scratch: Optional[torch.Tensor] = None, planes: Optional[int] = None):
        if lobe is not None and (lobe not in (RLS_RAY_DIFFUSE, RLS_RAY_GLOSSY) or refract):
            raise ValueError("lobe must be RLS_RAY_DIFFUSE or RLS_RAY_GLOSSY, on a queue without refract")
        if planes not in (None, 1) or (planes == 1 and (refract or lobe is not None)):
            raise ValueError("planes: 1 (a scalar weight, as the rlGgx node's Oren-Nayar queue), on a queue that is neither "
                             "refract nor an rlDisney lobe's")
        self.ctx, self.n, self.spp_n, self.refract = ctx, int(n), int(spp_n), bool(refract)
        self.lobe = lobe
        # one weight plane: refraction (with a kind plane) or planes=1 (without); its resolve is the mean over the spp_n^2
        # samples, rls_trace_ggx_refract_resolve
        self.scalar = self.refract or planes == 1
        scalar = self.scalar
        dev = ctx.torch_device
        cap = self.n * self.spp_n * self.spp_n
        self.capacity = cap
        self.offsets = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
        self._dir = torch.empty(3, cap, dtype=torch.float32, device=dev)
        self._weight = torch.empty(1 if scalar else 3, cap, dtype=torch.float32, device=dev)
        self._point = torch.empty(cap, dtype=torch.int32, device=dev)          # uint32 on the device; n < 2^31 here
        self._sample = torch.empty(cap, dtype=torch.uint8, device=dev)
        self._kind = torch.empty(cap, dtype=torch.uint8, device=dev) if refract and want_kind else None
        # (``scratch``: a uint8 block to use instead of one of its own -- the queues of one node emit may share one)
        self._scratch = scratch if scratch is not None else \
            torch.empty(max(scratch_bytes(self.n, self.spp_n), 1), dtype=torch.uint8, device=dev)
        # per point: getAvgReflectWeight (glossy) / the fraction of totally internally reflected samples (refraction) /
        # the valid samples (rlDisney)
        self.side = torch.empty(self.n, dtype=torch.float32, device=dev)
        w = self._weight
        q = RayQueue_()
        q.capacity = cap
        q.offsets = self.offsets.data_ptr()
        q.dir = capi.Vec3(*[self._dir[k].data_ptr() for k in range(3)])
        q.weight = capi.Rgb(w[0].data_ptr(), None if scalar else w[1].data_ptr(), None if scalar else w[2].data_ptr())
        q.point, q.sample = self._point.data_ptr(), self._sample.data_ptr()
        q.kind = self._kind.data_ptr() if self._kind is not None else None
        q.scratch, q.scratch_bytes = self._scratch.data_ptr(), self._scratch.numel()
        self.q = q

    @property
    def count(self) -> int:
        """offsets[n]: the number of rays (reads the device: synchronises)"""
        return int(self.offsets[self.n].item())

    @property
    def dir(self) -> torch.Tensor:
        return self._dir[:, :self.count]

    @property
    def weight(self) -> torch.Tensor:
        """[3, count] f/pdf (glossy) or [1, count] getSampleWeight (refraction)"""
        return self._weight[:, :self.count]

    @property
    def point(self) -> torch.Tensor:
        return self._point[:self.count]

    @property
    def sample(self) -> torch.Tensor:
        return self._sample[:self.count]

    @property
    def kind(self) -> Optional[torch.Tensor]:
        return None if self._kind is None else self._kind[:self.count]

    @property
    def avg_reflect_weight(self) -> torch.Tensor:
        if self.lobe is not None:
            raise AttributeError("an rlDisney queue has valid_count, not avg_reflect_weight")
        if self.refract:
            raise AttributeError("a refraction queue has tir_fraction, not avg_reflect_weight")
        return self.side

    @property
    def tir_fraction(self) -> torch.Tensor:
        if self.lobe is not None:
            raise AttributeError("an rlDisney queue has valid_count, not tir_fraction")
        if not self.refract:
            raise AttributeError("a glossy queue has avg_reflect_weight, not tir_fraction")
        return self.side

    @property
    def valid_count(self) -> torch.Tensor:
        """[n] the lobe's valid samples per point: rls_disney_integrate's diffuse_count / specular_count"""
        if self.lobe is None:
            raise AttributeError("an rlGgx queue has avg_reflect_weight / tir_fraction, not valid_count")
        return self.side

    def resolve(self, radiance: torch.Tensor, out: Optional[torch.Tensor] = None, count: Optional[int] = None) -> torch.Tensor:
        """radiance [3, >= count] float32, one per ray -> [3, n]: glossy and rlDisney the sum of radiance x f/pdf per point
        (the convention of rls_ggx_integrate's sum and rls_disney_integrate's diffuse_sum / specular_sum), refraction and
        planes=1 queues the mean of radiance x weight over the spp_n^2 samples.
        ``count``: the ray count when the caller knows it (skips the read of offsets[n], e.g. while recording a graph)."""
        ctx, n = self.ctx, self.n
        count = self.count if count is None else int(count)
        L = _radiance(radiance, count, "radiance")
        res = ctx.empty(3, n) if out is None else out
        lib = load()
        if self.scalar:
            check(lib.rls_trace_ggx_refract_resolve(ctx.handle, n, C.byref(self.q), self.spp_n, L, rgb(res, n, "result")))
        else:
            check(lib.rls_trace_ggx_glossy_resolve(ctx.handle, n, C.byref(self.q), L, rgb(res, n, "sum")))
        return res


def _emit(sampler: GgxSampler, spp_n: int, seed: int, first_index: int, queue: Optional[RayQueue], refract: bool) -> RayQueue:
    ctx, n = sampler.ctx, sampler.n
    q = RayQueue(ctx, n, spp_n, refract) if queue is None else queue
    if q.n != n or q.spp_n != int(spp_n) or q.refract != refract or q.lobe is not None:
        raise ValueError("queue: allocated for another batch size, spp_n or integrator")
    lib = load()
    fn = lib.rls_trace_ggx_refract_emit if refract else lib.rls_trace_ggx_glossy_emit
    check(fn(ctx.handle, n, C.byref(sampler.c), int(spp_n), int(seed) & 0xFFFFFFFF, int(first_index), C.byref(q.q),
             plane(q.side, n, "side") if n > 0 else None))
    return q


def glossy_rays(sampler: GgxSampler, spp_n: int, seed: int, first_index: int = 0, queue: Optional[RayQueue] = None) -> RayQueue:
    """integrateGlossy's sample rays (src/rlGgx.h:172-179): the samples rls_ggx_integrate draws, those with f/pdf != 0 queued
    with their direction and f/pdf; ``queue.avg_reflect_weight`` as rls_ggx_integrate writes it."""
    return _emit(sampler, spp_n, seed, first_index, queue, False)


def refract_rays(sampler: GgxSampler, spp_n: int, seed: int, first_index: int = 0, queue: Optional[RayQueue] = None) -> RayQueue:
    """integrateRefract's sample rays (src/rlGgx.h:228-241): the samples rls_ggx_integrate_refract(traced=1) draws, those with
    a non-zero weight queued with their direction, weight and kind (RLS_RAY_TRANSMITTED / RLS_RAY_TIR_MIRROR);
    ``queue.tir_fraction`` as rls_ggx_integrate_refract writes it."""
    return _emit(sampler, spp_n, seed, first_index, queue, True)


def disney_rays(sampler: DisneySampler, lobe: int, spp_n: int, seed: int, first_index: int = 0,
                queue: Optional[RayQueue] = None) -> RayQueue:
    """The sample rays of one rlDisney lobe (integrateDiffuse / integrateGlossy, src/rlDisney.cpp:240-243, 279-283; lobe
    RLS_RAY_DIFFUSE or RLS_RAY_GLOSSY): the samples rls_disney_integrate draws for that lobe, the valid ones (pdf > 1e-4)
    with f/pdf != 0 queued with their direction and f/pdf; ``queue.valid_count`` is the lobe's count as rls_disney_integrate
    writes it.  ``queue.resolve`` with radiance 1 is rls_disney_integrate's sum for the lobe."""
    ctx, n = sampler.ctx, sampler.n
    q = RayQueue(ctx, n, spp_n, lobe=lobe) if queue is None else queue
    if q.n != n or q.spp_n != int(spp_n) or q.lobe != lobe:
        raise ValueError("queue: allocated for another batch size, spp_n, integrator or lobe")
    check(load().rls_trace_disney_emit(ctx.handle, n, C.byref(sampler.c), int(lobe), int(spp_n), int(seed) & 0xFFFFFFFF,
                                       int(first_index), C.byref(q.q), plane(q.side, n, "valid_count") if n > 0 else None))
    return q


def _probe_hits(count, P, N, irradiance, rays: int) -> ProbeHits_:
    """The caller's hits of `rays` probe rays, validated, as rls_probe_hits (``ProbeQueue.resolve`` describes them).  The struct
    holds pointers only: the tensors stay the caller's.  irradiance None (the hits emit reads none): its planes stay NULL."""
    if not isinstance(count, torch.Tensor) or count.dtype != torch.uint8 or not count.is_cuda or count.dim() != 1 or \
            count.shape[0] < rays or not count.is_contiguous():
        raise ValueError(f"count: expected a contiguous uint8 CUDA tensor [>= {rays}]")
    shape = None
    for what, t in (("P", P), ("N", N), ("irradiance", irradiance)):
        if t is None and what == "irradiance":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 3 or \
                t.shape[0] != 3 or not 1 <= t.shape[1] <= RLS_MAX_PROBE_HITS or t.shape[2] < rays or \
                t.stride(2) != 1 or t.stride(1) != t.shape[2]:
            raise ValueError(f"{what}: expected a float32 CUDA tensor [3, 1..{RLS_MAX_PROBE_HITS}, >= {rays}] whose "
                             f"planes are contiguous")
        if shape is not None and t.shape != shape:
            raise ValueError(f"{what}: shape {tuple(t.shape)} differs from P's {tuple(shape)}")
        shape = t.shape
    h = ProbeHits_()
    h.max_hits, h.stride, h.count = int(shape[1]), int(shape[2]), count.data_ptr()
    h.P = capi.CVec3(*[P[k].data_ptr() for k in range(3)])
    h.N = capi.CVec3(*[N[k].data_ptr() for k in range(3)])
    if irradiance is not None:
        h.irradiance = capi.CRgb(*[irradiance[k].data_ptr() for k in range(3)])
    return h


class ProbeQueue:
    """integrateScatter's probe rays over n points at spp_n^2 samples: dense, point-major (ray j = i * spp_n^2 + s is sample s
    of point i; offsets[i] = i * spp_n^2).  ``count`` is known without reading the device."""

    def __init__(self, ctx, n: int, spp_n: int):
        self.ctx, self.n, self.spp_n = ctx, int(n), int(spp_n)
        dev = ctx.torch_device
        cap = self.n * self.spp_n * self.spp_n
        self.capacity = self.count = cap
        self.offsets = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
        self.origin = torch.empty(3, cap, dtype=torch.float32, device=dev)
        self.dir = torch.empty(3, cap, dtype=torch.float32, device=dev)
        self.maxdist = torch.empty(cap, dtype=torch.float32, device=dev)
        self.point = torch.empty(cap, dtype=torch.int32, device=dev)           # uint32 on the device; n < 2^31 here
        self.sample = torch.empty(cap, dtype=torch.uint8, device=dev)
        q = ProbeQueue_()
        q.capacity = cap
        q.offsets = self.offsets.data_ptr()
        q.origin = capi.Vec3(*[self.origin[k].data_ptr() for k in range(3)])
        q.dir = capi.Vec3(*[self.dir[k].data_ptr() for k in range(3)])
        q.maxdist, q.point, q.sample = self.maxdist.data_ptr(), self.point.data_ptr(), self.sample.data_ptr()
        self.q = q
        self.sampler: Optional[SssSampler] = None        # the closure and shading points of the last emit
        self.P: Optional[torch.Tensor] = None

    def resolve(self, count: torch.Tensor, P: torch.Tensor, N: torch.Tensor, irradiance: torch.Tensor,
                use_cavity_fade: bool = False, literal_matrix: bool = False, want_depth: bool = False,
                out: Optional[torch.Tensor] = None, depth_out: Optional[torch.Tensor] = None):
        """integrateScatter's combination of the caller's hits (rls_trace_sss_scatter_resolve) -> result [3, n] (and the
        mean number of shaded hits per probe ray [n] with ``want_depth``).
        count: uint8 [>= rays], the hits of every ray (values above max_hits read as max_hits); P, N, irradiance: float32
        [3, max_hits, stride] with stride >= rays: hit k of ray j at [:, k, j] -- positions in ascending t, sg->Ns aligned to
        sg->N, E before evalProfile and the cavity fade (include/rlshaders_amd_trace.h)."""
        if self.sampler is None:
            raise RuntimeError("resolve: no emit has filled this queue (trace.sss_probe_rays)")
        ctx, n = self.ctx, self.n
        h = _probe_hits(count, P, N, irradiance, self.count)
        res = ctx.empty(3, n) if out is None else out
        depth = (ctx.empty(n) if depth_out is None else depth_out) if want_depth else None
        s = self.sampler
        check(load().rls_trace_sss_scatter_resolve(
            ctx.handle, n, C.byref(s.c), _points(self.P, n), self.spp_n, C.byref(self.q), C.byref(h),
            1 if use_cavity_fade else 0, 1 if literal_matrix else 0, rgb(res, n, "result"),
            plane(depth, n, "mean_depth") if want_depth else None))
        return (res, depth) if want_depth else res


def sss_probe_rays(sampler: SssSampler, P: torch.Tensor, spp_n: int, seed: int, first_index: int = 0,
                   queue: Optional[ProbeQueue] = None) -> ProbeQueue:
    """integrateScatter's probe rays (getProbeRay, src/rlSss.h:224-228): the samples rls_sss_integrate_scatter draws, one ray
    each, origin sg->P + the probe offset (P: [3, n] float32, sg->P per point)."""
    ctx, n = sampler.ctx, sampler.n
    q = ProbeQueue(ctx, n, spp_n) if queue is None else queue
    if q.n != n or q.spp_n != int(spp_n):
        raise ValueError("queue: allocated for another batch size or spp_n")
    check(load().rls_trace_sss_probe_emit(ctx.handle, n, C.byref(sampler.c), _points(P, n), int(spp_n), int(seed) & 0xFFFFFFFF,
                                          int(first_index), C.byref(q.q)))
    q.sampler, q.P = sampler, P
    return q


def sss_hits_scratch_bytes(n: int, spp_n: int, max_hits: int, hit_capacity: int, n_lights: int, hit_spp_n: int) -> int:
    b = C.c_size_t()
    check(load().rls_trace_sss_hits_scratch_bytes(int(n), int(spp_n), int(max_hits), int(hit_capacity), int(n_lights),
                                                  int(hit_spp_n), C.byref(b)))
    return int(b.value)


class HitQueues:
    """The shaded probe hits of one ``sss_hit_rays`` call and the rays leaving them (rls_hit_queues): ``hit_element`` [listed]
    int64, the listed hits' elements k * stride + j of the hit planes, ray-major; ``hit_count`` the TRUE number of shaded hits
    (``listed`` = min(hit_count, hit_capacity)); ``shadow`` a light-loop queue over the LIST (dir, maxdist, weight_diffuse [1, .],
    kind, point = list index, sample; no weight_specular), ``diffuse`` integrateDiffuse's rays (dir, weight [1, .], point), at
    most one per listed hit.  ``hit_count`` and the views read the device once each (they synchronise)."""

    def __init__(self, ctx, n: int, spp_n: int, max_hits: int, stride: int, hit_capacity: int, n_lights: int, hit_spp_n: int,
                 trace_diffuse: bool = False, scratch: Optional[torch.Tensor] = None):
        self.ctx, self.n, self.spp_n, self.max_hits, self.stride = ctx, int(n), int(spp_n), int(max_hits), int(stride)
        self.hit_capacity, self.n_lights, self.hit_spp_n = int(hit_capacity), int(n_lights), int(hit_spp_n)
        self.trace_diffuse = bool(trace_diffuse)
        dev, cap = ctx.torch_device, self.hit_capacity
        i64 = dict(dtype=torch.int64, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self._hit_count = torch.zeros(1, **i64)
        self._hit_element = torch.empty(cap, **i64)
        self.shadow_capacity = scap = cap * self.n_lights * 2 * self.hit_spp_n * self.hit_spp_n
        self.shadow_offsets = torch.zeros(cap + 1, **i64)
        self._sdir, self._smaxdist, self._swd = torch.empty(3, scap, **f32), torch.empty(scap, **f32), torch.empty(1, scap, **f32)
        self._skind = torch.empty(scap, dtype=torch.uint8, device=dev)
        self._spoint = torch.empty(scap, dtype=torch.int32, device=dev)         # uint32 on the device
        self._ssample = torch.empty(scap, dtype=torch.uint8, device=dev)
        dcap = cap if self.trace_diffuse else 0
        self.diffuse_offsets = torch.zeros(cap + 1, **i64)
        self._ddir, self._dw = torch.empty(3, dcap, **f32), torch.empty(1, dcap, **f32)
        self._dpoint = torch.empty(dcap, dtype=torch.int32, device=dev)
        self._scratch = scratch if scratch is not None else torch.empty(
            max(sss_hits_scratch_bytes(self.n, self.spp_n, self.max_hits, cap, self.n_lights, self.hit_spp_n), 1),
            dtype=torch.uint8, device=dev)
        q = HitQueues_()
        q.hit_capacity, q.hit_count, q.hit_element = cap, self._hit_count.data_ptr(), self._hit_element.data_ptr()
        q.shadow.capacity, q.shadow.offsets = scap, self.shadow_offsets.data_ptr()
        q.shadow.dir = capi.Vec3(*[self._sdir[k].data_ptr() for k in range(3)])
        q.shadow.maxdist = self._smaxdist.data_ptr()
        q.shadow.weight_diffuse = capi.Rgb(self._swd[0].data_ptr(), None, None)
        q.shadow.kind, q.shadow.point, q.shadow.sample = self._skind.data_ptr(), self._spoint.data_ptr(), self._ssample.data_ptr()
        q.diffuse.capacity, q.diffuse.offsets = dcap, self.diffuse_offsets.data_ptr()
        q.diffuse.dir = capi.Vec3(*[self._ddir[k].data_ptr() for k in range(3)])
        q.diffuse.weight = capi.Rgb(self._dw[0].data_ptr(), None, None)
        q.diffuse.point = self._dpoint.data_ptr()
        q.scratch, q.scratch_bytes = self._scratch.data_ptr(), self._scratch.numel()
        self.q = q
        self.lights = None       # what the last emit took and the resolve takes again
        self.hits = None

    @property
    def hit_count(self) -> int:
        return int(self._hit_count.item())

    @property
    def listed(self) -> int:
        return min(self.hit_count, self.hit_capacity)

    @property
    def hit_element(self) -> torch.Tensor:
        return self._hit_element[:self.listed]

    @property
    def shadow_count(self) -> int:
        return int(self.shadow_offsets[self.hit_capacity].item()) if self.n_lights > 0 else 0

    @property
    def diffuse_count(self) -> int:
        return int(self.diffuse_offsets[self.hit_capacity].item()) if self.trace_diffuse else 0

    @property
    def shadow(self) -> dict:
        """the shadow rays' planes, the first ``shadow_count`` of each"""
        c = self.shadow_count
        return {"dir": self._sdir[:, :c], "maxdist": self._smaxdist[:c], "weight_diffuse": self._swd[:, :c],
                "kind": self._skind[:c], "point": self._spoint[:c], "sample": self._ssample[:c]}

    @property
    def diffuse(self) -> dict:
        c = self.diffuse_count
        return {"dir": self._ddir[:, :c], "weight": self._dw[:, :c], "point": self._dpoint[:c]}

    def resolve(self, visibility: Optional[torch.Tensor], radiance: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, counts: Optional[tuple] = None) -> torch.Tensor:
        """visibility [3, >= shadow_count] (None without lights), radiance [3, >= diffuse_count] (with trace_diffuse) -> E
        [3, max_hits, stride], the layout of the hits' irradiance: exactly 0 at every hit that is not listed.  ``counts``:
        (shadow_count, diffuse_count) where the caller knows them (skips the reads of the offsets)."""
        if self.hits is None:
            raise RuntimeError("resolve: no emit has filled these queues (trace.sss_hit_rays)")
        ctx = self.ctx
        sc, dc = counts if counts is not None else (self.shadow_count, self.diffuse_count)
        vis = _radiance(visibility, sc, "visibility") if self.n_lights > 0 else capi.CRgb(None, None, None)
        rad = _radiance(radiance, dc, "radiance") if self.trace_diffuse else capi.CRgb(None, None, None)
        E = ctx.empty(3, self.max_hits, self.stride) if out is None else out
        if E.dtype != torch.float32 or not E.is_cuda or E.shape != (3, self.max_hits, self.stride) or not E.is_contiguous():
            raise ValueError(f"out: expected a contiguous float32 CUDA tensor [3, {self.max_hits}, {self.stride}]")
        la, nl = self.lights
        check(load().rls_trace_sss_hits_resolve(ctx.handle, C.byref(self.hits), la, nl, self.hit_spp_n,
                                                1 if self.trace_diffuse else 0, C.byref(self.q), vis, rad,
                                                capi.Rgb(*[E[k].data_ptr() for k in range(3)])))
        return E


def sss_hit_rays(sampler: SssSampler, P: torch.Tensor, probe_queue: ProbeQueue, count: torch.Tensor, hitP: torch.Tensor,
                 hitN: torch.Tensor, lights, hit_spp_n: int, seed: int, *, hitT: Optional[torch.Tensor] = None,
                 use_cavity_fade: bool = False, trace_diffuse: bool = False, hit_capacity: Optional[int] = None,
                 hit_first_index: int = 0, queues: Optional[HitQueues] = None) -> HitQueues:
    """shadeProbeSample's shading of the probe hits (src/rlSss.h:415-418) up to its traces: lists the hits the scatter resolve
    counts as shaded and emits evalLightSample's shadow rays (an Oren-Nayar MIS light loop at roughness 0, hit_spp_n^2 samples a
    light) and, with ``trace_diffuse``, integrateDiffuse's one ray at each.  sampler, P, probe_queue: those of the probe emit
    (``sss_probe_rays``, or the ``probes`` of ``skin_node_rays`` with an SssSampler of the node's scatter parameters); count,
    hitP, hitN: the hits as ``ProbeQueue.resolve`` takes them; hitT: the tangents at the hits in hitP's layout (None: the
    library's own); lights: None, one ``make_light`` or a sequence; hit_capacity: the hits the list holds (default: every slot,
    max_hits * rays).  The hit with element e samples from hash(seed, hit_first_index + e).  ``HitQueues.resolve`` turns the traced
    visibility and radiance into the E planes of ``ProbeQueue.resolve`` / ``SkinNodeQueues.resolve``."""
    ctx, n = sampler.ctx, sampler.n
    if probe_queue.n != n:
        raise ValueError("probe_queue: emitted for another batch size")
    rays = probe_queue.count
    hits = _probe_hits(count, hitP, hitN, None, rays)
    T = capi.CVec3(None, None, None)
    if hitT is not None:
        if not isinstance(hitT, torch.Tensor) or hitT.dtype != torch.float32 or not hitT.is_cuda or hitT.shape != hitP.shape or \
                not hitT.is_contiguous():
            raise ValueError("hitT: expected a contiguous float32 CUDA tensor of hitP's shape")
        T = capi.CVec3(*[hitT[k].data_ptr() for k in range(3)])
    la, nl = light_array(lights)
    cap = hits.max_hits * rays if hit_capacity is None else int(hit_capacity)
    q = HitQueues(ctx, n, probe_queue.spp_n, hits.max_hits, hits.stride, cap, nl, hit_spp_n, trace_diffuse) \
        if queues is None else queues
    if (q.n, q.spp_n, q.max_hits, q.stride, q.n_lights, q.hit_spp_n, q.trace_diffuse) != \
            (n, probe_queue.spp_n, hits.max_hits, hits.stride, nl, int(hit_spp_n), bool(trace_diffuse)) or \
            (hit_capacity is not None and q.hit_capacity != cap):
        raise ValueError("queues: allocated for another batch, hit layout, light count, hit_spp_n or trace_diffuse")
    check(load().rls_trace_sss_hits_emit(ctx.handle, n, C.byref(sampler.c), _points(P, n), probe_queue.spp_n,
                                         C.byref(probe_queue.q), C.byref(hits), T, 1 if use_cavity_fade else 0, la, nl,
                                         int(hit_spp_n), 1 if trace_diffuse else 0, int(seed) & 0xFFFFFFFF, int(hit_first_index),
                                         C.byref(q.q)))
    q.lights, q.hits = (la, nl), hits
    q._keep = (count, hitP, hitN, hitT)
    return q


def shadow_scratch_bytes(n: int, n_lights: int, spp_n: int) -> int:
    b = C.c_size_t()
    check(load().rls_trace_shadow_scratch_bytes(int(n), int(n_lights), int(spp_n), C.byref(b)))
    return int(b.value)


def ggx_shader(sampler: GgxSampler, KdColor=(1.0, 1.0, 1.0), Kd=0.5, diffuseRoughness=0.0, Ks=0.5,
               KtColor=(1.0, 1.0, 1.0), Kt=0.0) -> "capi.GgxShader":
    """The node parameters of rlGgx (rls_ggx_shader) as ``GgxSampler.directLighting`` / ``GgxSampler.shade`` take them: the
    light loop reads the first four, the whole node (``ggx_node_rays``) KtColor and Kt too."""
    pn = sampler.pn
    sh = capi.GgxShader(param_rgb(KdColor, pn, "KdColor"), param(Kd, pn, "Kd"),
                        param(diffuseRoughness, pn, "diffuseRoughness"), param(Ks, pn, "Ks"),
                        param_rgb(KtColor, pn, "KtColor"), param(Kt, pn, "Kt"))
    sh._keep = (KdColor, Kd, diffuseRoughness, Ks, KtColor, Kt)      # tensor parameters stay alive with the struct
    return sh


class ShadowQueue:
    """The shadow rays of one light-loop emit over n points under n_lights lights at spp_n^2 samples (rls_shadow_queue):
    point-major CSR; within a point lights ascending, within a light the light-strategy samples, then the BSDF diffuse-lobe
    samples, then the BSDF specular-lobe samples.  Planes are allocated for the full capacity n * n_lights * 3 * spp_n^2; the
    properties view the first ``count`` rays.  ``disney``: an rlDisney queue (three planes of weight_diffuse; rlGgx has one).
    ``skin``: a lobe's light loop of the rlSkin node: no weight_diffuse, two rays a sample at most (capacity n * n_lights * 2 *
    spp_n^2), within a light the samples ascending and a sample's light-strategy ray before its BSDF-strategy ray; resolved by
    ``SkinNodeQueues.resolve``.  ``scatter`` (with ``skin``): integrateScatter's Oren-Nayar light loop at the diffuse rays' points
    of an rlSkin bounce emit: weight_diffuse [1, count] alone, no weight_specular; rlGgx's order without the specular segment."""

    def __init__(self, ctx, n: int, n_lights: int, spp_n: int, disney: bool = False, scratch: Optional[torch.Tensor] = None,
                 skin: bool = False, scatter: bool = False):
        self.ctx, self.n, self.n_lights, self.spp_n, self.disney = ctx, int(n), int(n_lights), int(spp_n), bool(disney)
        self.skin, self.scatter = bool(skin), bool(scatter)
        if self.skin and self.disney:
            raise ValueError("skin and disney exclude each other")
        if self.scatter and not self.skin:
            raise ValueError("scatter: a queue of the rlSkin node")
        dev = ctx.torch_device
        cap = self.n * self.n_lights * (2 if skin else 3) * self.spp_n * self.spp_n
        self.capacity = cap
        self.offsets = torch.empty(self.n + 1, dtype=torch.int64, device=dev)
        self._dir = torch.empty(3, cap, dtype=torch.float32, device=dev)
        self._maxdist = torch.empty(cap, dtype=torch.float32, device=dev)
        self._ws = torch.empty(0 if scatter else 3, cap, dtype=torch.float32, device=dev)
        self._wd = torch.empty(1 if scatter else 0 if skin else 3 if disney else 1, cap, dtype=torch.float32, device=dev)
        self._kind = torch.empty(cap, dtype=torch.uint8, device=dev)
        self._point = torch.empty(cap, dtype=torch.int32, device=dev)          # uint32 on the device; n < 2^31 here
        self._sample = torch.empty(cap, dtype=torch.uint8, device=dev)
        self._scratch = scratch if scratch is not None else \
            torch.empty(max(shadow_scratch_bytes(self.n, self.n_lights, self.spp_n), 1), dtype=torch.uint8, device=dev)
        q = ShadowQueue_()
        q.capacity = cap
        q.offsets = self.offsets.data_ptr()
        q.dir = capi.Vec3(*[self._dir[k].data_ptr() for k in range(3)])
        q.maxdist = self._maxdist.data_ptr()
        q.weight_specular = capi.Rgb(*[None if scatter else self._ws[k].data_ptr() for k in range(3)])
        wd = self._wd
        q.weight_diffuse = capi.Rgb(None if skin and not scatter else wd[0].data_ptr(), wd[1].data_ptr() if disney else None,
                                    wd[2].data_ptr() if disney else None)
        q.kind, q.point, q.sample = self._kind.data_ptr(), self._point.data_ptr(), self._sample.data_ptr()
        q.scratch, q.scratch_bytes = self._scratch.data_ptr(), self._scratch.numel()
        self.q = q
        # what the last emit took and the resolve takes again: the lights; rlGgx: the sampler and its shader
        self.lights = None
        self.sampler = None
        self.shader = None

    @property
    def count(self) -> int:
        """offsets[n]: the number of rays (reads the device: synchronises)"""
        return int(self.offsets[self.n].item())

    @property
    def dir(self) -> torch.Tensor:
        return self._dir[:, :self.count]

    @property
    def maxdist(self) -> torch.Tensor:
        return self._maxdist[:self.count]

    @property
    def weight_specular(self) -> torch.Tensor:
        return self._ws[:, :self.count]

    @property
    def weight_diffuse(self) -> torch.Tensor:
        """[3, count] (rlDisney) or [1, count] (rlGgx: Oren-Nayar's scalar term)"""
        return self._wd[:, :self.count]

    @property
    def kind(self) -> torch.Tensor:
        """uint8 [count]: light index | RLS_SHADOW_BSDF | RLS_SHADOW_SPECULAR | RLS_SHADOW_DIFFUSE"""
        return self._kind[:self.count]

    @property
    def point(self) -> torch.Tensor:
        return self._point[:self.count]

    @property
    def sample(self) -> torch.Tensor:
        return self._sample[:self.count]

    def resolve(self, visibility: torch.Tensor, out=None, count: Optional[int] = None):
        """visibility [3, >= count] float32, one per ray and channel (1 unoccluded, 0 blocked) ->
        (direct_diffuse [3, n], direct_specular [3, n]): with visibility 1 the AOVs of rls_ggx_direct_lighting /
        rls_disney_direct_lighting.  ``count``: the ray count when the caller knows it (skips the read of offsets[n])."""
        if self.skin:
            raise RuntimeError("resolve: a lobe's shadow queue of the rlSkin node is resolved by SkinNodeQueues.resolve")
        if self.lights is None:
            raise RuntimeError("resolve: no emit has filled this queue (trace.ggx_shadow_rays / disney_shadow_rays)")
        ctx, n = self.ctx, self.n
        count = self.count if count is None else int(count)
        vis = _radiance(visibility, count, "visibility")
        dd, ds = out if out is not None else (ctx.empty(3, n), ctx.empty(3, n))
        lights, nl = self.lights
        lib = load()
        if self.disney:
            check(lib.rls_trace_disney_direct_resolve(ctx.handle, n, lights, nl, self.spp_n, C.byref(self.q), vis,
                                                      rgb(dd, n, "direct_diffuse"), rgb(ds, n, "direct_specular")))
        else:
            check(lib.rls_trace_ggx_direct_resolve(ctx.handle, n, C.byref(self.sampler.c), C.byref(self.shader), lights, nl,
                                                   self.spp_n, C.byref(self.q), vis, rgb(dd, n, "direct_diffuse"),
                                                   rgb(ds, n, "direct_specular")))
        return dd, ds


def _shadow_queue(sampler, lights, spp_n: int, queue: Optional[ShadowQueue], disney: bool):
    la, nl = light_array(lights)
    q = ShadowQueue(sampler.ctx, sampler.n, nl, spp_n, disney) if queue is None else queue
    if q.n != sampler.n or q.spp_n != int(spp_n) or q.n_lights != nl or q.disney != disney:
        raise ValueError("queue: allocated for another batch size, light count, spp_n or node")
    return q, la, nl


def ggx_shadow_rays(sampler: GgxSampler, shader: "capi.GgxShader", P: torch.Tensor, lights, spp_n: int, seed: int,
                    first_index: int = 0, queue: Optional[ShadowQueue] = None) -> ShadowQueue:
    """The shadow rays of rlGgx's light loop (src/rlGgx.cpp:285-299): the samples rls_ggx_direct_lighting draws, one ray per
    term-carrying sample with direction, distance to the light and both lobes' weights.  ``shader``: ``trace.ggx_shader``;
    ``lights``: one ``make_light`` or a sequence; P: [3, n] float32, sg->P per point."""
    ctx, n = sampler.ctx, sampler.n
    q, la, nl = _shadow_queue(sampler, lights, spp_n, queue, False)
    check(load().rls_trace_ggx_direct_emit(ctx.handle, n, C.byref(sampler.c), C.byref(shader), _points(P, n), la, nl,
                                           int(spp_n), int(seed) & 0xFFFFFFFF, int(first_index), C.byref(q.q)))
    q.lights, q.sampler, q.shader, q.P = (la, nl), sampler, shader, P
    return q


def disney_shadow_rays(sampler: DisneySampler, P: torch.Tensor, lights, spp_n: int, seed: int, first_index: int = 0,
                       queue: Optional[ShadowQueue] = None) -> ShadowQueue:
    """The shadow rays of rlDisney's light loop (src/rlDisney.cpp:695-705): the samples rls_disney_direct_lighting draws."""
    ctx, n = sampler.ctx, sampler.n
    q, la, nl = _shadow_queue(sampler, lights, spp_n, queue, True)
    check(load().rls_trace_disney_direct_emit(ctx.handle, n, C.byref(sampler.c), _points(P, n), la, nl, int(spp_n),
                                              int(seed) & 0xFFFFFFFF, int(first_index), C.byref(q.q)))
    q.lights, q.sampler, q.P = (la, nl), sampler, P
    return q


# ---------------------------------------------------------------------------------------------
# Whole nodes: every ray of rls_ggx_shade / rls_disney_shade in one emit, their AOVs in one resolve


def node_scratch_bytes(n: int, n_lights: int, spp_n: int) -> int:
    """The scratch block the queues of one node emit can share: the largest any of them needs."""
    b = scratch_bytes(n, spp_n)
    return max(b, shadow_scratch_bytes(n, n_lights, spp_n)) if n_lights > 0 else b


class _NodeQueues:
    """What the nodes' queue sets share, each node describing its members: the shadow queues (None without lights), the ray
    queues and rlSkin's probe queue by member name, the C struct, the emit's C call, what the last emit took."""
    SHADOWS = ("shadow",)    # the ShadowQueue members and ShadowQueue's keyword arguments
    SHADOW_KW = {}
    RAY_MEMBERS = ()         # (member name, RayQueue's keyword arguments) per ray queue, in the C struct's order
    RAYS = ()                # their names (__init_subclass__)
    SCALARS = ()             # rlSkin: ``probes`` (a ProbeQueue) and these [n] planes follow the ray queues
    STRUCT = None            # the C struct of the set, the name of the emit's C call
    EMIT = ""
    shadow = None            # (a node that names its shadow queues otherwise has none of this name)

    def __init_subclass__(cls):
        cls.RAYS = tuple(name for name, _ in cls.RAY_MEMBERS)

    def __init__(self, ctx, n: int, n_lights: int, spp_n: int, share_scratch: bool = False):
        self.ctx, self.n, self.n_lights, self.spp_n = ctx, int(n), int(n_lights), int(spp_n)
        scratch = None
        if share_scratch:
            scratch = torch.empty(max(node_scratch_bytes(self.n, self.n_lights, self.spp_n), 1), dtype=torch.uint8,
                                  device=ctx.torch_device)
        self.scratch = scratch
        for name in self.SHADOWS:
            setattr(self, name, ShadowQueue(ctx, self.n, self.n_lights, self.spp_n, scratch=scratch, **self.SHADOW_KW)
                    if self.n_lights > 0 else None)
        for name, kw in self.RAY_MEMBERS:
            setattr(self, name, RayQueue(ctx, n, spp_n, scratch=scratch, **kw))
        if self.SCALARS:
            self.probes = ProbeQueue(ctx, n, spp_n)
            for name in self.SCALARS:
                setattr(self, name, torch.empty(self.n, dtype=torch.float32, device=ctx.torch_device))
        self.lights = None
        self.sampler = None
        self.shader = None
        self.P = None
        self.traced = True
        self.state = None        # a bounce emit's (RayState, GiDepths_): its resolve takes them again
        self.scales = None       # rlDisney's bounce emit: (indirectDiffuseScale, indirectSpecularScale)

    def _queues(self) -> dict:
        """the compacted queues by member name, in the C struct's order"""
        return {name: getattr(self, name) for name in self.SHADOWS + self.RAYS}

    def _struct(self):
        q = self.STRUCT()
        for name, m in self._queues().items():
            setattr(q, name, C.pointer(m.q) if m is not None else None)
        if self.SCALARS:
            q.probes = C.pointer(self.probes.q)
            for name in self.SCALARS:
                setattr(q, name, getattr(self, name).data_ptr())
        return q

    def _matches(self, sampler, nl: int, spp_n: int) -> bool:
        return self.n == sampler.n and self.spp_n == int(spp_n) and self.n_lights == nl

    def _out(self, sampler, out, cls):
        n, ctx = self.n, self.ctx
        if out is None:
            out = {k: ctx.empty(3, n) for k in sampler.SHADE_AOVS + ("out",)}
        o = cls()
        for k in sampler.SHADE_AOVS:
            setattr(o, k, rgb(out[k], n, k))
        if "out" in out:
            o.out = rgb(out["out"], n, "out")
        return out, o

    def counts(self) -> dict:
        """the ray count of every compacted queue (reads the device: synchronises); rlSkin's probe queue is dense"""
        return {name: m.count if m is not None else 0 for name, m in self._queues().items()}


class GgxNodeQueues(_NodeQueues):
    """The rays of the whole rlGgx node (rls_trace_ggx_shade_emit): ``shadow`` (ShadowQueue, None without lights), ``glossy``
    (3 weight planes), ``refract`` (weight [1, count], kind) and ``diffuse`` (weight [1, count]) RayQueues -- the samples
    ``GgxSampler.shade`` draws."""
    RAY_MEMBERS = (("glossy", {}), ("refract", {"refract": True}), ("diffuse", {"planes": 1}))
    STRUCT, EMIT, BOUNCE_EMIT = GgxNodeQueues_, "rls_trace_ggx_shade_emit", "rls_trace_ggx_bounce_emit"

    def resolve(self, visibility, glossy, refract, diffuse, out=None, counts: Optional[dict] = None) -> dict:
        """What the renderer traced, [3, >= count] float32 per queue (``visibility`` is not read without lights and may be
        None) -> the dict ``GgxSampler.shade`` returns: the five AOVs and out, [3, n] each.  ``counts``: the ray counts where
        the caller knows them (skips the reads of offsets[n], e.g. while recording a graph)."""
        if self.sampler is None:
            raise RuntimeError("resolve: no emit has filled these queues (trace.ggx_node_rays)")
        cnt = self.counts() if counts is None else counts
        t = GgxNodeTraced_()
        if self.shadow is not None:
            t.visibility = _radiance(visibility, cnt["shadow"], "visibility")
        t.glossy = _radiance(glossy, cnt["glossy"], "glossy")
        t.refract = _radiance(refract, cnt["refract"], "refract")
        t.diffuse = _radiance(diffuse, cnt["diffuse"], "diffuse")
        out, o = self._out(self.sampler, out, capi.GgxShadeOut)
        la, nl = self.lights
        q = self._struct()
        if self.state is not None:
            state, depths = self.state
            check(load().rls_trace_ggx_bounce_resolve(self.ctx.handle, self.n, C.byref(self.sampler.c), C.byref(self.shader), la,
                                                      nl, self.spp_n, C.byref(state.struct(self.n)), C.byref(depths), C.byref(q),
                                                      C.byref(t), C.byref(o)))
            return out
        check(load().rls_trace_ggx_shade_resolve(self.ctx.handle, self.n, C.byref(self.sampler.c), C.byref(self.shader), la, nl,
                                                 1 if self.traced else 0, self.spp_n, C.byref(q), C.byref(t), C.byref(o)))
        return out


class DisneyNodeQueues(_NodeQueues):
    """The rays of the whole rlDisney node (rls_trace_disney_shade_emit): ``shadow`` (None without lights), ``diffuse`` and
    ``specular`` RayQueues -- the samples ``DisneySampler.shade`` draws."""
    SHADOW_KW = {"disney": True}
    RAY_MEMBERS = (("diffuse", {"lobe": RLS_RAY_DIFFUSE}), ("specular", {"lobe": RLS_RAY_GLOSSY}))
    STRUCT, EMIT, BOUNCE_EMIT = DisneyNodeQueues_, "rls_trace_disney_shade_emit", "rls_trace_disney_bounce_emit"

    def resolve(self, visibility, diffuse, specular, out=None, counts: Optional[dict] = None) -> dict:
        """-> the dict ``DisneySampler.shade`` returns: the four AOVs and out, [3, n] each."""
        if self.sampler is None:
            raise RuntimeError("resolve: no emit has filled these queues (trace.disney_node_rays)")
        cnt = self.counts() if counts is None else counts
        t = DisneyNodeTraced_()
        if self.shadow is not None:
            t.visibility = _radiance(visibility, cnt["shadow"], "visibility")
        t.diffuse = _radiance(diffuse, cnt["diffuse"], "diffuse")
        t.specular = _radiance(specular, cnt["specular"], "specular")
        out, o = self._out(self.sampler, out, capi.DisneyShadeOut)
        la, nl = self.lights
        q = self._struct()
        if self.state is not None:
            state, depths = self.state
            m = self.sampler.c.materials                          # a tensor scale: per material where the closure has an index
            pn = int(m.count) if m.id else self.n
            kd, ks = (param(v, pn, what) for v, what in zip(self.scales, ("indirectDiffuseScale", "indirectSpecularScale")))
            check(load().rls_trace_disney_bounce_resolve(self.ctx.handle, self.n, C.byref(self.sampler.c), kd, ks, la, nl,
                                                         self.spp_n, C.byref(state.struct(self.n)), C.byref(depths), C.byref(q),
                                                         C.byref(t), C.byref(o)))
            return out
        check(load().rls_trace_disney_shade_resolve(self.ctx.handle, self.n, la, nl, self.spp_n, C.byref(q), C.byref(t),
                                                    C.byref(o)))
        return out


def _node_emit(cls, sampler, shader, P, lights, spp_n: int, seed: int, first_index: int, queues, share_scratch: bool,
               traced: Optional[bool] = None, state=None, scales=None):
    """One node emit into a queue set of class ``cls`` (``queues``, or a new one): the C call takes the closure, the node
    parameters where the node has them (``shader``), P and the lights, ``traced`` where the node has the switch, then the
    sampling and the queues.  The set -- and its ``shadow`` queue, which resolves by itself too -- remembers what the emit took.
    ``state``: (RayState, depths) for the node's bounce call, which takes them after the sampling in place of ``traced``."""
    ctx, n = sampler.ctx, sampler.n
    la, nl = light_array(lights)
    q = cls(ctx, n, nl, spp_n, share_scratch) if queues is None else queues
    if not q._matches(sampler, nl, spp_n):
        raise ValueError("queues: allocated for another batch size, light count or spp_n")
    cq = q._struct()
    closure = (C.byref(sampler.c),) if shader is None else (C.byref(sampler.c), C.byref(shader))
    switch = () if traced is None else (1 if traced else 0,)
    emit, bounce = cls.EMIT, ()
    if state is not None:
        state = (state[0], gi_depths(state[1]))
        emit, switch = cls.BOUNCE_EMIT, ()
        bounce = (C.byref(state[0].struct(n)), C.byref(state[1]))
    check(getattr(load(), emit)(ctx.handle, n, *closure, _points(P, n), la, nl, *switch, int(spp_n), int(seed) & 0xFFFFFFFF,
                                int(first_index), *bounce, C.byref(cq)))
    q.state, q.scales = state, scales
    for m in (q, q.shadow):
        if m is not None:
            m.lights, m.sampler, m.shader, m.P = (la, nl), sampler, shader, P
    if traced is not None:
        q.traced = bool(traced)
    return q


def ggx_node_rays(sampler: GgxSampler, shader: "capi.GgxShader", P: torch.Tensor, lights, spp_n: int, seed: int,
                  first_index: int = 0, traced: bool = True, queues: Optional[GgxNodeQueues] = None,
                  share_scratch: bool = False) -> GgxNodeQueues:
    """Every ray of rlGgx's shader_evaluate (src/rlGgx.cpp:248-327) as ``GgxSampler.shade`` samples it: the light loop's shadow
    rays, integrateGlossy (stream pair 24), integrateRefract (25; ``traced=False``: the one ray of the untraced branch) and the
    Oren-Nayar indirect diffuse loop (26), behind the node's gates.  ``shader``: ``trace.ggx_shader`` with KtColor / Kt;
    ``lights``: None, one ``make_light`` or a sequence.  ``share_scratch``: the queues share one scratch block."""
    return _node_emit(GgxNodeQueues, sampler, shader, P, lights, spp_n, seed, first_index, queues, share_scratch, bool(traced))


def disney_node_rays(sampler: DisneySampler, P: torch.Tensor, lights, spp_n: int, seed: int, first_index: int = 0,
                     queues: Optional[DisneyNodeQueues] = None, share_scratch: bool = False) -> DisneyNodeQueues:
    """Every ray of rlDisney's shader_evaluate (src/rlDisney.cpp:685-727) as ``DisneySampler.shade`` samples it: the light
    loop's shadow rays, integrateDiffuse (stream pair 24) and integrateGlossy (25)."""
    return _node_emit(DisneyNodeQueues, sampler, None, P, lights, spp_n, seed, first_index, queues, share_scratch)


# ---------------------------------------------------------------------------------------------
# Secondary-ray hits: the two nodes shaded under a per-point ray state (rls_trace_*_bounce_emit / _resolve)


def gi_depths(depths) -> GiDepths_:
    """The options' GI depths as rls_gi_depths: a GiDepths_, a mapping with the keys total / diffuse / glossy / refraction, or
    the four values in that order."""
    if isinstance(depths, GiDepths_):
        return depths
    if isinstance(depths, dict):
        return GiDepths_(*(int(depths[k]) for k in ("total", "diffuse", "glossy", "refraction")))
    total, diffuse, glossy, refraction = depths
    return GiDepths_(int(total), int(diffuse), int(glossy), int(refraction))


class RayState:
    """sg->Rt and the sg->Rr* counters per shading point (rls_ray_state): five uint8 CUDA tensors [n] -- ``ray_type`` (RLS_RT_*
    bits), ``Rr``, ``Rr_diff``, ``Rr_gloss``, ``Rr_refr``.  ``RayState.camera(ctx, n)``: camera rays at depth 0."""
    PLANES = ("ray_type", "Rr", "Rr_diff", "Rr_gloss", "Rr_refr")

    def __init__(self, ray_type, Rr, Rr_diff, Rr_gloss, Rr_refr):
        self.ray_type, self.Rr, self.Rr_diff, self.Rr_gloss, self.Rr_refr = ray_type, Rr, Rr_diff, Rr_gloss, Rr_refr
        n = int(ray_type.shape[0]) if isinstance(ray_type, torch.Tensor) and ray_type.dim() == 1 else -1
        for name in self.PLANES:
            t = getattr(self, name)
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.shape != (n,) or \
                    not t.is_contiguous():
                raise TypeError(f"RayState.{name}: expected a contiguous uint8 CUDA tensor [n]")
        self.n = n

    @classmethod
    def camera(cls, ctx, n: int) -> "RayState":
        z = [torch.zeros(int(n), dtype=torch.uint8, device=ctx.torch_device) for _ in range(4)]
        return cls(torch.full((int(n),), RLS_RT_CAMERA, dtype=torch.uint8, device=ctx.torch_device), *z)

    @classmethod
    def empty(cls, ctx, n: int) -> "RayState":
        return cls(*[torch.empty(int(n), dtype=torch.uint8, device=ctx.torch_device) for _ in cls.PLANES])

    def struct(self, n: int) -> RayState_:
        if self.n < int(n):
            raise ValueError(f"RayState: {self.n} points, the call has {n}")
        return RayState_(*[getattr(self, name).data_ptr() if self.n > 0 else None for name in self.PLANES])


def ggx_bounce_rays(sampler: GgxSampler, shader: "capi.GgxShader", P: torch.Tensor, lights, spp_n: int, seed: int,
                    state: RayState, depths, first_index: int = 0, queues: Optional[GgxNodeQueues] = None,
                    share_scratch: bool = False) -> GgxNodeQueues:
    """``ggx_node_rays`` at the hits of secondary rays (rls_trace_ggx_bounce_emit): per point the ray-depth switches of rlGgx's
    shader_evaluate read off ``state`` and ``depths`` (``gi_depths``) decide which lobes the shadow rays carry, which branch of
    integrateRefract the point takes, and whether the indirect loops run (camera rays only).  The queues remember the state:
    ``.resolve(...)`` is the bounce resolve."""
    return _node_emit(GgxNodeQueues, sampler, shader, P, lights, spp_n, seed, first_index, queues, share_scratch,
                      state=(state, depths))


def disney_bounce_rays(sampler: DisneySampler, P: torch.Tensor, lights, spp_n: int, seed: int, state: RayState, depths,
                       first_index: int = 0, queues: Optional[DisneyNodeQueues] = None, share_scratch: bool = False,
                       indirectDiffuseScale=1.0, indirectSpecularScale=1.0) -> DisneyNodeQueues:
    """``disney_node_rays`` at the hits of secondary rays (rls_trace_disney_bounce_emit): the indirect loops run on camera rays
    within the depth limits; on diffuse and glossy rays the resolve scales the direct terms by the node's ``indirectDiffuseScale`` /
    ``indirectSpecularScale`` (values, or tensors like the sampler's other parameters)."""
    return _node_emit(DisneyNodeQueues, sampler, None, P, lights, spp_n, seed, first_index, queues, share_scratch,
                      state=(state, depths), scales=(indirectDiffuseScale, indirectSpecularScale))


def advance_state(ctx, queue, parent: RayState, ray_type: int, out: Optional[RayState] = None,
                  rays: Optional[int] = None) -> RayState:
    """The state of the hits of ``queue``'s rays (a RayQueue or ShadowQueue emitted for points in state ``parent``), which
    leave as rays of ``ray_type`` (rls_trace_ray_state_advance): Rr and the type's counter grow by one, saturating at 255.
    ``rays``: the queue's ray count where the caller knows it (else read from the device); ``out``: a RayState to write."""
    rays = queue.count if rays is None else int(rays)
    child = RayState.empty(ctx, rays) if out is None else out
    if child.n < rays:
        raise ValueError("advance_state: out holds fewer planes than the queue has rays")
    check(load().rls_trace_ray_state_advance(ctx.handle, rays, queue._point.data_ptr(), C.byref(parent.struct(queue.n)),
                                             int(ray_type), C.byref(child.struct(rays))))
    return child


class SkinNodeQueues(_NodeQueues):
    """The rays of the whole rlSkin node (rls_trace_skin_emit): per GGX lobe a ShadowQueue of the lobe's light loop
    (``sheen_shadow``, ``specular_shadow``; None without lights; specular terms only, two rays a sample at most: capacity
    n * n_lights * 2 * spp_n^2) and a RayQueue of its integrateGlossy (``sheen_glossy``, ``specular_glossy``), and the ProbeQueue
    of integrateScatter (``probes``) -- the samples ``SkinShader.integrate`` draws.  ``sheenFresnel``, ``specularFresnel``,
    ``sssWeight`` [n]: the layers' hand-down scalars, written by the emit."""
    SHADOWS = ("sheen_shadow", "specular_shadow")
    SHADOW_KW = {"skin": True}
    RAY_MEMBERS = (("sheen_glossy", {}), ("specular_glossy", {}))
    SCALARS = ("sheenFresnel", "specularFresnel", "sssWeight")
    STRUCT, EMIT = SkinNodeQueues_, "rls_trace_skin_emit"

    def resolve(self, sheen_visibility, specular_visibility, sheen_glossy, specular_glossy, count, P, N, irradiance,
                use_cavity_fade: bool = False, literal_matrix: bool = False, out=None, counts: Optional[dict] = None) -> dict:
        """What the renderer traced -> the dict ``SkinShader.integrate`` returns: sheen, specular, sss, out [3, n] and
        sheenFresnel, specularFresnel, sssWeight [n].  The visibilities and radiances are [3, >= count] float32 per queue (the
        visibilities are not read without lights and may be None); count, P, N, irradiance are the probe hits as
        ``ProbeQueue.resolve`` takes them.  ``counts``: the ray counts where the caller knows them (skips the reads of
        offsets[n], e.g. while recording a graph)."""
        t, hits, out, o = self._traced(sheen_visibility, specular_visibility, sheen_glossy, specular_glossy, count, P, N, irradiance,
                                       out, self.counts() if counts is None else counts)
        ctx, n = self.ctx, self.n
        la, nl = self.lights
        q = self._struct()
        check(load().rls_trace_skin_resolve(ctx.handle, n, C.byref(self.sampler.c), _points(self.P, n), la, nl,
                                            1 if use_cavity_fade else 0, 1 if literal_matrix else 0, self.spp_n, C.byref(q),
                                            C.byref(t), C.byref(o)))
        return out

    def _traced(self, sheen_visibility, specular_visibility, sheen_glossy, specular_glossy, count, P, N, irradiance, out, cnt):
        """the node's traced struct (and the hits it points at, to be kept alive), the output dict and its C struct"""
        if self.sampler is None:
            raise RuntimeError("resolve: no emit has filled these queues (trace.skin_node_rays / skin_bounce_rays)")
        ctx, n = self.ctx, self.n
        t = SkinNodeTraced_()
        if self.n_lights > 0:
            t.sheen_visibility = _radiance(sheen_visibility, cnt["sheen_shadow"], "sheen_visibility")
            t.specular_visibility = _radiance(specular_visibility, cnt["specular_shadow"], "specular_visibility")
        t.sheen_glossy = _radiance(sheen_glossy, cnt["sheen_glossy"], "sheen_glossy")
        t.specular_glossy = _radiance(specular_glossy, cnt["specular_glossy"], "specular_glossy")
        hits = _probe_hits(count, P, N, irradiance, self.probes.count)
        t.hits = C.pointer(hits)
        if out is None:
            out = {k: ctx.empty(3, n) for k in ("sheen", "specular", "sss", "out")}
            out.update({k: ctx.empty(n) for k in self.SCALARS})
        o = capi.SkinIntegrateOut()
        for k in ("sheen", "specular", "sss", "out"):
            if k in out:
                setattr(o, k, rgb(out[k], n, k))
        for k in self.SCALARS:
            if k in out:
                setattr(o, k, plane(out[k], n, k))
        return t, hits, out, o


class SkinBounceQueues(SkinNodeQueues):
    """``SkinNodeQueues`` for an rlSkin bounce emit (rls_trace_skin_bounce_emit): the node's queues and ``diffuse_shadow``, the
    ShadowQueue of integrateScatter's Oren-Nayar light loop at the diffuse rays' points (None without lights; weight_diffuse
    [1, count] alone)."""
    STRUCT, EMIT, BOUNCE_EMIT = SkinBounceQueues_, "rls_trace_skin_bounce_emit", "rls_trace_skin_bounce_emit"

    def __init__(self, ctx, n: int, n_lights: int, spp_n: int, share_scratch: bool = False):
        super().__init__(ctx, n, n_lights, spp_n, share_scratch)
        self.diffuse_shadow = ShadowQueue(ctx, self.n, self.n_lights, self.spp_n, scratch=self.scratch, skin=True, scatter=True) \
            if self.n_lights > 0 else None

    def _struct(self):
        node = super()._struct()
        q = SkinBounceQueues_()
        for name, _ in SkinNodeQueues_._fields_:
            setattr(q.node, name, getattr(node, name))
        q.diffuse_shadow = C.pointer(self.diffuse_shadow.q) if self.diffuse_shadow is not None else None
        return q

    def counts(self) -> dict:
        cnt = super().counts()
        cnt["diffuse_shadow"] = self.diffuse_shadow.count if self.diffuse_shadow is not None else 0
        return cnt

    def resolve(self, sheen_visibility, specular_visibility, sheen_glossy, specular_glossy, count, P, N, irradiance,
                diffuse_visibility=None, use_cavity_fade: bool = False, literal_matrix: bool = False, out=None,
                counts: Optional[dict] = None) -> dict:
        """``SkinNodeQueues.resolve`` under the emit's ray state (rls_trace_skin_bounce_resolve).  ``diffuse_visibility``:
        [3, >= count] float32 for ``diffuse_shadow``'s rays; not read without lights and may be None."""
        cnt = self.counts() if counts is None else counts
        node, hits, out, o = self._traced(sheen_visibility, specular_visibility, sheen_glossy, specular_glossy, count, P, N,
                                          irradiance, out, cnt)
        if self.state is None:
            raise RuntimeError("resolve: no bounce emit has filled these queues (trace.skin_bounce_rays)")
        t = SkinBounceTraced_()
        for name, _ in SkinNodeTraced_._fields_:
            setattr(t.node, name, getattr(node, name))
        if self.n_lights > 0:
            t.diffuse_visibility = _radiance(diffuse_visibility, cnt["diffuse_shadow"], "diffuse_visibility")
        ctx, n = self.ctx, self.n
        la, nl = self.lights
        q = self._struct()
        state, depths = self.state
        check(load().rls_trace_skin_bounce_resolve(ctx.handle, n, C.byref(self.sampler.c), _points(self.P, n), la, nl,
                                                   1 if use_cavity_fade else 0, 1 if literal_matrix else 0, self.spp_n,
                                                   C.byref(state.struct(n)), C.byref(depths), C.byref(q), C.byref(t), C.byref(o)))
        return out


def skin_node_rays(shader, P: torch.Tensor, lights, spp_n: int, seed: int, first_index: int = 0,
                   queues: Optional[SkinNodeQueues] = None, share_scratch: bool = False) -> SkinNodeQueues:
    """Every ray of rlSkin's shader_evaluate (src/rlSkin.cpp:174-254) as ``SkinShader.integrate`` samples it: per GGX lobe the
    light loop's shadow rays and integrateGlossy's rays (stream pairs 0 and 1), then integrateScatter's probe rays (pair 2).
    ``shader``: a ``SkinShader``; ``lights``: None, one ``make_light`` or a sequence; P: [3, n] float32, sg->P per point.
    ``share_scratch``: the queues share one scratch block."""
    return _node_emit(SkinNodeQueues, shader, None, P, lights, spp_n, seed, first_index, queues, share_scratch)


def skin_bounce_rays(shader, P: torch.Tensor, lights, spp_n: int, seed: int, state: RayState, depths, first_index: int = 0,
                     queues: Optional[SkinBounceQueues] = None, share_scratch: bool = False) -> SkinBounceQueues:
    """``skin_node_rays`` at the hits of secondary rays (rls_trace_skin_bounce_emit): per point the switches of rlSkin's
    shader_evaluate read off ``state`` and ``depths`` (``gi_depths``) -- nothing at a shadow ray's point, both GGX lobes behind
    Rr_gloss <= GI_glossy_depth, each lobe's integrateGlossy behind Rr == 0 (which moves the mean-Fresnel hand-down, so
    sssWeight), and on a diffuse ray integrateScatter's probe walk replaced by one Oren-Nayar light loop, whose shadow rays go
    into ``diffuse_shadow`` at the seed ``seed ^ RLS_SKIN_DIFFUSE_SEED``.  The queues remember the state: ``.resolve(...)`` is the
    bounce resolve."""
    return _node_emit(SkinBounceQueues, shader, None, P, lights, spp_n, seed, first_index, queues, share_scratch,
                      state=(state, depths))


# ---------------------------------------------------------------------------------------------
# Shadow rays' hits: the opacity each node returns and the fold of the opacities along a shadow ray into a visibility


def _ray_type(ray_type, n: int):
    """the rls_ray_state.ray_type plane of n points: None (no point is a shadow ray's), a uint8 CUDA tensor [n] or a RayState"""
    if ray_type is None:
        return None
    t = ray_type.ray_type if isinstance(ray_type, RayState) else ray_type
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 1 or t.shape[0] < n or \
            not t.is_contiguous():
        raise TypeError(f"ray_type: expected a contiguous uint8 CUDA tensor [>= {n}] or a RayState")
    return t.data_ptr() if n > 0 else None


def ggx_opacity(ctx, n: int, opacity=1.0, opacity_color=(1.0, 1.0, 1.0), KtColor=(1.0, 1.0, 1.0), Kt=0.0, ray_type=None,
                materials=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sg->out_opacity of rlGgx at n points (rls_trace_ggx_opacity) -> [3, n]: at a shadow ray's point (``ray_type`` &
    RLS_RT_SHADOW) 1 - KtColor * Kt (src/rlGgx.cpp:264-268), at any other clamp(opacity * opacity_color, 0, 1) (:250, :326).
    The parameters are numbers or CUDA tensors like the samplers': per-point [n] / [3, n], or with ``materials`` = (ids, count)
    per-material columns.  ``ray_type``: None, a uint8 tensor [n] or a ``RayState``."""
    n = int(n)
    m, pn = material_index(materials, n)
    p = GgxOpacity_(param(opacity, pn, "opacity"), param_rgb(opacity_color, pn, "opacity_color"),
                    param_rgb(KtColor, pn, "KtColor"), param(Kt, pn, "Kt"), m)
    res = ctx.empty(3, n) if out is None else out
    check(load().rls_trace_ggx_opacity(ctx.handle, n, C.byref(p), _ray_type(ray_type, n), rgb(res, n, "out_opacity")))
    return res


def disney_opacity(ctx, n: int, opacity=(1.0, 1.0, 1.0), ray_type=None, materials=None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sg->out_opacity of rlDisney (rls_trace_disney_opacity) -> [3, n]: at a shadow ray's point the opacity as it is, NOT
    clamped (src/rlDisney.cpp:685-687), at any other clamp(opacity, 0, 1) (:728)."""
    n = int(n)
    m, pn = material_index(materials, n)
    p = DisneyOpacity_(param_rgb(opacity, pn, "opacity"), m)
    res = ctx.empty(3, n) if out is None else out
    check(load().rls_trace_disney_opacity(ctx.handle, n, C.byref(p), _ray_type(ray_type, n), rgb(res, n, "out_opacity")))
    return res


def skin_opacity(ctx, n: int, opacity=1.0, opacity_color=(1.0, 1.0, 1.0), ray_type=None, materials=None,
                 incoming: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sg->out_opacity of rlSkin (rls_trace_skin_opacity) -> [3, n]: clamp(opacity * opacity_color, 0, 1) (src/rlSkin.cpp:167,
    :255), at a shadow ray's point multiplied into the sg->out_opacity the node found (:169-172): ``incoming`` [3, n], None
    reading as 1; it may be ``out``."""
    n = int(n)
    m, pn = material_index(materials, n)
    p = SkinOpacity_(param(opacity, pn, "opacity"), param_rgb(opacity_color, pn, "opacity_color"), m)
    res = ctx.empty(3, n) if out is None else out
    inc = capi.CRgb(None, None, None) if incoming is None or n == 0 else _radiance(incoming, n, "incoming")
    check(load().rls_trace_skin_opacity(ctx.handle, n, C.byref(p), _ray_type(ray_type, n), inc, rgb(res, n, "out_opacity")))
    return res


class ShadowHits:
    """The hits of shadow rays as rls_shadow_hits: hit k of ray j is element k * stride + j.
    count: uint8 CUDA [>= rays], the hits of every ray (values above max_hits read as max_hits).
    opacity, without ``index``: float32 CUDA [3, max_hits, stride] (or [3, max_hits * stride] with ``stride`` given), out_opacity
    per element; with ``index``: a table [3, table_count], and index an int32 / uint32 CUDA tensor [max_hits, stride] (or
    [max_hits * stride] with ``stride`` given) whose entries pick the table's column (clamped to the last)."""

    def __init__(self, count: torch.Tensor, opacity: torch.Tensor, max_hits: int, stride: Optional[int] = None,
                 index: Optional[torch.Tensor] = None):
        max_hits = int(max_hits)
        if not 1 <= max_hits <= 255:
            raise ValueError("max_hits must be in 1 .. 255")
        if not isinstance(count, torch.Tensor) or count.dtype != torch.uint8 or not count.is_cuda or count.dim() != 1 or \
                not count.is_contiguous():
            raise TypeError("count: expected a contiguous uint8 CUDA tensor [rays]")
        elements = index if index is not None else opacity
        lead = 0 if index is not None else 1
        if not isinstance(elements, torch.Tensor) or not elements.is_cuda or not elements.is_contiguous():
            raise TypeError("opacity / index: expected contiguous CUDA tensors")
        if elements.dim() == lead + 2:
            if elements.shape[lead] != max_hits or (stride is not None and int(stride) != elements.shape[lead + 1]):
                raise ValueError("opacity / index: expected [.., max_hits, stride]")
            stride = int(elements.shape[lead + 1])
        elif elements.dim() != lead + 1 or stride is None or elements.shape[lead] < max_hits * int(stride):
            raise ValueError("opacity / index: expected [.., max_hits, stride], or [.., >= max_hits * stride] with stride given")
        if not isinstance(opacity, torch.Tensor) or opacity.dtype != torch.float32 or not opacity.is_cuda or \
                opacity.shape[0] != 3 or not opacity.is_contiguous():
            raise TypeError("opacity: expected a contiguous float32 CUDA tensor of 3 planes")
        if index is not None and (index.dtype not in (torch.int32, torch.uint32) or opacity.dim() != 2 or opacity.shape[1] < 1):
            raise TypeError("index: expected an int32 CUDA tensor beside an opacity table [3, table_count >= 1]")
        self.count, self.opacity, self.index, self.max_hits, self.stride = count, opacity, index, max_hits, int(stride)
        h = ShadowHits_()
        h.max_hits, h.stride, h.count = self.max_hits, self.stride, count.data_ptr()
        planes = opacity.reshape(3, -1)
        h.opacity = capi.CRgb(*[planes[k].data_ptr() for k in range(3)])
        if index is not None:
            h.index, h.table_count = index.data_ptr(), int(opacity.shape[1])
        self.h = h


def shadow_visibility(ctx, rays: int, hits: ShadowHits, base: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The visibility of ``rays`` shadow rays from the opacities of their hits (rls_trace_shadow_visibility) -> [3, rays]: per
    ray and channel base (None: 1) times (1 - opacity) of every hit, in hit order; no clamp.  What ``ShadowQueue.resolve``, the
    node queues' ``.resolve`` and ``HitQueues.resolve`` take as visibility.  ``base`` [3, >= rays] may be ``out``."""
    rays = int(rays)
    if hits.stride < rays or hits.count.shape[0] < rays:
        raise ValueError(f"hits: stride {hits.stride} / count [{hits.count.shape[0]}] below {rays} rays")
    res = ctx.empty(3, rays) if out is None else out
    b = capi.CRgb(None, None, None) if base is None or rays == 0 else _radiance(base, rays, "base")
    check(load().rls_trace_shadow_visibility(ctx.handle, rays, C.byref(hits.h), b, rgb(res, rays, "visibility")))
    return res


# ---- routing a queue's hits to the nodes ------------------------------------------------------------------------------------------
def route_scratch_bytes(rays: int, bins: int) -> int:
    b = C.c_size_t()
    check(load().rls_trace_route_scratch_bytes(int(rays), int(bins), C.byref(b)))
    return int(b.value)


_W32 = (torch.float32, torch.int32, torch.uint32)


def _route_rows(t: torch.Tensor, what: str) -> list:
    """the planes of one tensor: itself (1-D) or its rows ([k, count]), float32 / int32 / uint32 words or uint8 bytes"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dim() not in (1, 2) or t.stride(-1) != 1 or \
            t.dtype not in _W32 + (torch.uint8,):
        raise TypeError(f"{what}: expected a float32 / int32 / uint32 / uint8 CUDA tensor [count] or [k, count] with unit inner "
                        f"stride")
    return [t] if t.dim() == 1 else [t[k] for k in range(t.shape[0])]


def _route_index(index: torch.Tensor, m: Optional[int]) -> int:
    if not isinstance(index, torch.Tensor) or index.dtype not in (torch.int32, torch.uint32) or not index.is_cuda or \
            index.dim() != 1 or not index.is_contiguous():
        raise TypeError("index: expected a contiguous int32 / uint32 CUDA tensor [m]")
    m = int(index.shape[0]) if m is None else int(m)
    if m > index.shape[0]:
        raise ValueError(f"index holds {index.shape[0]} entries, the call has {m}")
    return m


def route_planes(src, dst) -> RoutePlanes_:
    """rls_route_planes of two equally long lists of 1-D plane tensors, pairwise of one dtype: the 32-bit planes in list order,
    then the byte planes in list order.  The counts are passed on as they are: the library refuses what exceeds its caps."""
    if len(src) != len(dst):
        raise ValueError("route_planes: as many dst planes as src planes")
    p = RoutePlanes_()
    words, octets = [], []
    for s, d in zip(src, dst):
        if s.dtype != d.dtype or s.dim() != 1 or d.dim() != 1 or s.stride(0) != 1 or d.stride(0) != 1:
            raise TypeError("route_planes: a src and its dst are 1-D planes of one dtype with unit stride")
        (octets if s.dtype == torch.uint8 else words).append((s, d))
    p.n_w32, p.n_u8 = len(words), len(octets)
    for k, (s, d) in enumerate(words[:RLS_ROUTE_MAX_W32]):
        p.src_w32[k], p.dst_w32[k] = s.data_ptr(), d.data_ptr()
    for k, (s, d) in enumerate(octets[:RLS_ROUTE_MAX_U8]):
        p.src_u8[k], p.dst_u8[k] = s.data_ptr(), d.data_ptr()
    return p


def _route_move(ctx, index: torch.Tensor, src, dst, m: Optional[int], gather: bool) -> None:
    m = _route_index(index, m)
    if m == 0 or not src:
        return
    fn = load().rls_trace_route_gather if gather else load().rls_trace_route_scatter
    # (more planes than one call takes: several calls, words and bytes capped separately)
    words = [(s, d) for s, d in zip(src, dst) if s.dtype != torch.uint8]
    octets = [(s, d) for s, d in zip(src, dst) if s.dtype == torch.uint8]
    while words or octets:
        part = words[:RLS_ROUTE_MAX_W32] + octets[:RLS_ROUTE_MAX_U8]
        words, octets = words[RLS_ROUTE_MAX_W32:], octets[RLS_ROUTE_MAX_U8:]
        p = route_planes([s for s, _ in part], [d for _, d in part])
        check(fn(ctx.handle, m, index.data_ptr(), C.byref(p)))


def route_gather(ctx, index: torch.Tensor, src, dst, m: Optional[int] = None) -> None:
    """dst[p][j] = src[p][index[j]], j < m (rls_trace_route_gather): ``src`` / ``dst`` lists of 1-D plane tensors, ``index`` an
    int32 / uint32 CUDA tensor (a range of ``HitRoutes.order``)."""
    _route_move(ctx, index, src, dst, m, True)


def route_scatter(ctx, index: torch.Tensor, src, dst, m: Optional[int] = None) -> None:
    """dst[p][index[j]] = src[p][j], j < m (rls_trace_route_scatter)"""
    _route_move(ctx, index, src, dst, m, False)


def route_fill(ctx, index: torch.Tensor, value, dst, m: Optional[int] = None) -> None:
    """dst[p][index[j]] = value[p], j < m (rls_trace_route_fill): ``dst`` a list of 1-D float32 planes, ``value`` as many numbers"""
    m = _route_index(index, m)
    value = [float(v) for v in value]
    if len(value) != len(dst):
        raise ValueError("route_fill: one value per plane")
    for d in dst:
        if not isinstance(d, torch.Tensor) or d.dtype != torch.float32 or not d.is_cuda or d.dim() != 1 or d.stride(0) != 1:
            raise TypeError("route_fill: dst planes are 1-D float32 CUDA tensors with unit stride")
    if m == 0:
        return
    ptrs = (C.c_void_p * max(len(dst), 1))(*[d.data_ptr() for d in dst])
    vals = (C.c_float * max(len(dst), 1))(*value)
    check(load().rls_trace_route_fill(ctx.handle, m, index.data_ptr(), len(dst), ptrs, vals))


class HitRoutes:
    """The stable partition of ``rays`` rays by the node bin they hit (rls_hit_routes): owns ``offsets`` [bins + 2] int64,
    ``order`` [rays] (uint32 on the device, int32 here: ray indices below 2^31 read as they are), ``slot`` (the inverse, where
    asked) and the scratch.  Bin ``b``'s rays are ``index(b)``, ascending; ``b == bins`` gives the misses."""

    def __init__(self, ctx, rays: int, bins: int, slot: bool = False):
        self.ctx, self.rays, self.bins = ctx, int(rays), int(bins)
        dev = ctx.torch_device
        self.offsets = torch.empty(self.bins + 2, dtype=torch.int64, device=dev)
        self.order = torch.empty(self.rays, dtype=torch.int32, device=dev)
        self.slot = torch.empty(self.rays, dtype=torch.int32, device=dev) if slot else None
        self._scratch = torch.empty(max(route_scratch_bytes(self.rays, self.bins), 1), dtype=torch.uint8, device=dev)
        r = HitRoutes_()
        r.bins, r.offsets = self.bins, self.offsets.data_ptr()
        r.order = self.order.data_ptr() if self.rays > 0 else None
        r.slot = self.slot.data_ptr() if slot and self.rays > 0 else None
        r.scratch, r.scratch_bytes = self._scratch.data_ptr(), self._scratch.numel()
        self.r = r
        self._host = None

    def route(self, bin: torch.Tensor) -> "HitRoutes":
        if not isinstance(bin, torch.Tensor) or bin.dtype != torch.uint8 or not bin.is_cuda or bin.dim() != 1 or \
                bin.shape[0] < self.rays or not bin.is_contiguous():
            raise TypeError(f"bin: expected a contiguous uint8 CUDA tensor [>= {self.rays}]")
        self._host = None
        check(load().rls_trace_route_hits(self.ctx.handle, self.rays, bin.data_ptr() if self.rays > 0 else None,
                                          C.byref(self.r)))
        return self

    def bounds(self) -> list:
        """offsets on the host (one device-to-host copy after a route, cached: it synchronises)"""
        if self._host is None:
            self._host = [int(v) for v in self.offsets.tolist()]
        return self._host

    def sizes(self) -> list:
        """the ray count of every bin 0 .. bins - 1 and of the misses (bins + 1 values)"""
        o = self.bounds()
        return [o[b + 1] - o[b] for b in range(self.bins + 1)]

    def index(self, b: int) -> torch.Tensor:
        """bin b's ray indices, ascending: a view into ``order`` (b == bins: the misses)"""
        if not 0 <= int(b) <= self.bins:
            raise ValueError(f"bin {b} outside 0 .. {self.bins}")
        o = self.bounds()
        return self.order[o[int(b)]:o[int(b) + 1]]

    def gather(self, b: int, *tensors) -> tuple:
        """bin b's columns of every tensor ([rays] or [k, rays]) as dense tensors ([m] / [k, m]), one per argument"""
        idx = self.index(b)
        m = int(idx.shape[0])
        src, dst, out = [], [], []
        for t in tensors:
            rows = _route_rows(t, "gather")
            if t.shape[-1] < self.rays:
                raise ValueError(f"gather: a tensor of {t.shape[-1]} columns, the routes have {self.rays} rays")
            res = torch.empty(t.shape[:-1] + (m,), dtype=t.dtype, device=t.device)
            src += rows
            dst += _route_rows(res, "gather")
            out.append(res)
        route_gather(self.ctx, idx, src, dst)
        return tuple(out)

    def gather_state(self, b: int, state: RayState) -> RayState:
        """the RayState of bin b's rays out of the per-ray ``state``"""
        return RayState(*self.gather(b, *[getattr(state, name) for name in RayState.PLANES]))

    def scatter(self, b: int, src_rgb: torch.Tensor, dst_rgb: torch.Tensor) -> torch.Tensor:
        """bin b's dense ``src_rgb`` [k, m] back to its rays' columns of ``dst_rgb`` [k, rays]"""
        idx = self.index(b)
        src, dst = _route_rows(src_rgb, "scatter"), _route_rows(dst_rgb, "scatter")
        if src_rgb.shape[-1] < idx.shape[0] or dst_rgb.shape[-1] < self.rays or len(src) != len(dst):
            raise ValueError("scatter: src [k, >= the bin's size] and dst [k, >= rays]")
        route_scatter(self.ctx, idx, src, dst)
        return dst_rgb

    def fill_misses(self, value, dst_rgb: torch.Tensor) -> torch.Tensor:
        """``value`` (one number per plane) into the misses' columns of ``dst_rgb`` [k, rays]"""
        if dst_rgb.shape[-1] < self.rays:
            raise ValueError("fill_misses: dst [k, >= rays]")
        route_fill(self.ctx, self.index(self.bins), value, _route_rows(dst_rgb, "fill_misses"))
        return dst_rgb


def route_hits(ctx, bin: torch.Tensor, bins: int, slot: bool = False, routes: Optional[HitRoutes] = None,
               rays: Optional[int] = None) -> HitRoutes:
    """Route ``rays`` (default: all of ``bin``) traced rays by the node bin they hit (rls_trace_route_hits): ``bin`` uint8 CUDA
    [rays], a value below ``bins`` that node's bin, any other (255 by convention) a miss.  ``routes``: a HitRoutes to write
    again (no allocation: recordable by ``ctx.capture()``)."""
    rays = int(bin.shape[0]) if rays is None else int(rays)
    if routes is None:
        routes = HitRoutes(ctx, rays, bins, slot)
    elif routes.rays != rays or routes.bins != int(bins) or (slot and routes.slot is None):
        raise ValueError("route_hits: routes was made for another ray count, bin count or without slot")
    return routes.route(bin)
