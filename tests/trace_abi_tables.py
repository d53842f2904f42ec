"""the surface of the companion library (include/rlshaders_amd_trace.h, librls_trace.so, rlshaders_amd/trace.py) by verb family,
as data: a new family adds one entry here and every whole-surface check of tests/test_trace_abi.py covers it.

  arity      entry point -> parameter count, written out: the change detector of the header
  structs    the header structs the family brought (each mirrored by a ctypes.Structure of trace.py)
  callables  what trace.py offers for it
  snippet    the body of a C99 / C++14 function: every initialiser, call expression (with its argument count) and constant
             expression a caller of the family writes
  width      kernels per math mode and lane-group width, <G, fast> for G in 1, 4, 16, 64
  mode       kernels per math mode, <fast>
  free       kernels free of the math mode (+, x and integer arithmetic only; templates or guarded, launched from the EXACT
             unit's host code alone), by the instances in use"""


def _family(arity, structs=(), callables=(), snippet=None, width=(), mode=(), free=()):
    return dict(arity=arity, structs=structs, callables=callables, snippet=snippet, width=width, mode=mode, free=free)


FAMILIES = dict(
    integrators=_family(
        dict(rls_trace_scratch_bytes=3, rls_trace_ggx_glossy_emit=8, rls_trace_ggx_refract_emit=8, rls_trace_ggx_glossy_resolve=5,
             rls_trace_ggx_refract_resolve=6, rls_trace_disney_emit=9),
        structs=("rls_ray_queue",), callables=("glossy_rays", "refract_rays", "disney_rays"),
        snippet='rls_ray_queue q = {0}; size_t b = 0; (void)q;\n'
                '  return rls_trace_scratch_bytes(1, 1, &b) == RLS_OK && RLS_RAY_TIR_MIRROR == 1 ? 0 : 1;',
        width=("ggx_glossy_emit_kernel", "ggx_refract_emit_kernel", "disney_diffuse_emit_kernel", "disney_specular_emit_kernel"),
        free=("trace_scan_block_kernel", "trace_scan_totals_kernel", "trace_scan_add_kernel", "trace_compact_kernel<1>",
              "trace_compact_kernel<3>", "trace_resolve_kernel<1>", "trace_resolve_kernel<3>")),
    sss=_family(
        dict(rls_trace_sss_probe_emit=8, rls_trace_sss_scatter_resolve=11),
        structs=("rls_probe_queue", "rls_probe_hits"), callables=("sss_probe_rays",),
        mode=("sss_probe_emit_kernel", "sss_scatter_resolve_kernel")),
    lights=_family(
        dict(rls_trace_shadow_scratch_bytes=4, rls_trace_ggx_direct_emit=11, rls_trace_disney_direct_emit=10,
             rls_trace_ggx_direct_resolve=11, rls_trace_disney_direct_resolve=9),
        structs=("rls_shadow_queue",), callables=("ggx_shadow_rays", "disney_shadow_rays", "ShadowQueue", "ggx_shader"),
        snippet='rls_shadow_queue q = {0}; size_t b = 0; (void)q;\n'
                '  if ((RLS_SHADOW_LIGHT_MASK | RLS_SHADOW_BSDF | RLS_SHADOW_SPECULAR | RLS_SHADOW_DIFFUSE) != 0x3F) return 2;\n'
                '  if (RLS_SHADOW_LIGHT_MASK != RLS_MAX_LIGHTS - 1) return 3;\n'
                '  return rls_trace_shadow_scratch_bytes(1, 1, 1, &b) == RLS_OK ? 0 : 1;',
        width=("ggx_direct_emit_kernel", "disney_direct_emit_kernel"),
        free=("shadow_compact_kernel<0>", "shadow_compact_kernel<1>", "shadow_compact_kernel<3>", "shadow_resolve_kernel<1>",
              "shadow_resolve_kernel<3>")),
    hits=_family(
        dict(rls_trace_sss_hits_scratch_bytes=7, rls_trace_sss_hits_emit=16, rls_trace_sss_hits_resolve=10),
        structs=("rls_hit_queues",), callables=("sss_hit_rays",),
        width=("sss_hits_emit_kernel",), mode=("sss_hits_gate_kernel",),
        free=("sss_hits_list_kernel", "hits_compact_kernel", "sss_hits_fill_kernel", "sss_hits_resolve_kernel")),
    shade=_family(
        dict(rls_trace_ggx_shade_emit=12, rls_trace_ggx_shade_resolve=11, rls_trace_disney_shade_emit=10,
             rls_trace_disney_shade_resolve=8),
        structs=("rls_ggx_node_queues", "rls_ggx_node_traced", "rls_disney_node_queues", "rls_disney_node_traced"),
        callables=("ggx_node_rays", "disney_node_rays"),
        snippet='rls_ggx_node_queues q = {0}; rls_ggx_node_traced t; rls_disney_node_queues d = {0};\n'
                '  rls_disney_node_traced u; rls_ggx_shade_out o; rls_disney_shade_out p; (void)t; (void)u; (void)o; (void)p;\n'
                '  return rls_trace_ggx_shade_resolve(0, 0, 0, 0, 0, 0, 1, 1, &q, 0, 0) +\n'
                '         rls_trace_disney_shade_resolve(0, 0, 0, 0, 1, &d, 0, 0);',
        width=("ggx_node_glossy_emit_kernel", "ggx_node_refract_emit_kernel", "ggx_node_diffuse_emit_kernel",
               "disney_node_diffuse_emit_kernel", "disney_node_specular_emit_kernel"),
        free=("ggx_node_resolve_kernel", "disney_node_resolve_kernel", "ggx_node_compose_kernel", "disney_node_compose_kernel")),
    skin=_family(
        dict(rls_trace_skin_emit=10, rls_trace_skin_resolve=12),
        structs=("rls_skin_node_queues", "rls_skin_node_traced"), callables=("skin_node_rays",),
        snippet='rls_skin_node_queues q = {0}; rls_skin_node_traced t; rls_skin_integrate_out o; rls_cvec3 P = {0};\n'
                '  (void)t; (void)o;\n'
                '  return rls_trace_skin_emit(0, 0, 0, P, 0, 0, 1, 7u, 0, &q) +\n'
                '         rls_trace_skin_resolve(0, 0, 0, P, 0, 0, 0, 0, 1, &q, 0, 0);',
        width=("skin_shadow_emit_kernel", "skin_sheen_glossy_emit_kernel", "skin_specular_glossy_emit_kernel"),
        # the probe emit and the one resolve follow the context's math mode (the scatter walk's profile and MIS arithmetic)
        mode=("skin_probe_emit_kernel", "skin_node_resolve_kernel")),
    bounce=_family(
        dict(rls_trace_ggx_bounce_emit=13, rls_trace_ggx_bounce_resolve=12, rls_trace_disney_bounce_emit=12,
             rls_trace_disney_bounce_resolve=13, rls_trace_ray_state_advance=6),
        structs=("rls_gi_depths", "rls_ray_state"), callables=("ggx_bounce_rays", "disney_bounce_rays", "advance_state", "RayState"),
        snippet='rls_ggx_node_queues q = {0}; rls_disney_node_queues d = {0}; rls_ray_state s = {0};\n'
                '  rls_gi_depths g = { 8, 2, 2, 4 }; rls_param k = { 0, 1.0f }; int rt = RLS_RT_CAMERA | RLS_RT_GLOSSY;\n'
                '  rls_cvec3 P = { 0, 0, 0 };\n'
                '  return rls_trace_ggx_bounce_emit(0, 0, 0, 0, P, 0, 0, 1, 7, 0, &s, &g, &q) +\n'
                '         rls_trace_disney_bounce_emit(0, 0, 0, P, 0, 0, 1, 7, 0, &s, &g, &d) +\n'
                '         rls_trace_ggx_bounce_resolve(0, 0, 0, 0, 0, 0, 1, &s, &g, &q, 0, 0) +\n'
                '         rls_trace_disney_bounce_resolve(0, 0, 0, k, k, 0, 0, 1, &s, &g, &d, 0, 0) +\n'
                '         rls_trace_ray_state_advance(0, 0, 0, &s, rt, &s);',
        width=("ggx_bounce_direct_emit_kernel", "ggx_bounce_glossy_emit_kernel", "ggx_bounce_refract_emit_kernel",
               "ggx_bounce_diffuse_emit_kernel", "disney_bounce_direct_emit_kernel", "disney_bounce_diffuse_emit_kernel",
               "disney_bounce_specular_emit_kernel"),
        free=("ggx_bounce_resolve_kernel", "disney_bounce_resolve_kernel", "state_advance_kernel")),
    skin_bounce=_family(
        dict(rls_trace_skin_bounce_emit=12, rls_trace_skin_bounce_resolve=14),
        structs=("rls_skin_bounce_queues", "rls_skin_bounce_traced"), callables=("skin_bounce_rays",),
        snippet='rls_skin_bounce_queues q; rls_skin_bounce_traced t; rls_skin_integrate_out o; rls_ray_state s;\n'
                '  rls_gi_depths g = { 8, 2, 2, 4 }; rls_cvec3 P = { 0, 0, 0 }; unsigned seed = 7u ^ RLS_SKIN_DIFFUSE_SEED;\n'
                '  q.diffuse_shadow = 0; q.node.probes = 0; t.node.hits = 0; t.diffuse_visibility.r = 0; s.Rr = 0; (void)o;\n'
                '  return rls_trace_skin_bounce_emit(0, 0, 0, P, 0, 0, 1, seed, 0, &s, &g, &q) +\n'
                '         rls_trace_skin_bounce_resolve(0, 0, 0, P, 0, 0, 0, 0, 1, &s, &g, &q, &t, &o);',
        width=("skin_bounce_shadow_emit_kernel", "skin_bounce_sheen_glossy_emit_kernel", "skin_bounce_specular_glossy_emit_kernel",
               "skin_diffuse_emit_kernel"),
        mode=("skin_bounce_probe_emit_kernel", "skin_bounce_resolve_kernel")),
    opacity=_family(
        dict(rls_trace_ggx_opacity=5, rls_trace_disney_opacity=5, rls_trace_skin_opacity=6, rls_trace_shadow_visibility=5),
        structs=("rls_ggx_opacity", "rls_disney_opacity", "rls_skin_opacity", "rls_shadow_hits"),
        callables=("ggx_opacity", "disney_opacity", "skin_opacity", "ShadowHits", "shadow_visibility"),
        snippet='rls_ggx_opacity g = {{0, 1.0f}, {0, 0, 0, 1.0f, 1.0f, 1.0f}, {0, 0, 0, 0.2f, 0.9f, 0.7f},\n'
                '                       {0, 0.5f}, {0, 0}};\n'
                '  rls_disney_opacity d = {{0, 0, 0, 1.0f, 1.0f, 1.0f}, {0, 0}};\n'
                '  rls_skin_opacity s = {{0, 1.0f}, {0, 0, 0, 1.0f, 1.0f, 1.0f}, {0, 0}};\n'
                '  rls_shadow_hits h = {4, 0, 0, {0, 0, 0}, 0, 0}; rls_rgb o = {0, 0, 0}; rls_crgb b = {0, 0, 0};\n'
                '  return rls_trace_ggx_opacity(0, 0, &g, 0, o) + rls_trace_disney_opacity(0, 0, &d, 0, o) +\n'
                '         rls_trace_skin_opacity(0, 0, &s, 0, b, o) + rls_trace_shadow_visibility(0, 0, &h, b, o);',
        free=("ggx_opacity_kernel", "disney_opacity_kernel", "skin_opacity_kernel", "shadow_visibility_kernel")),
    route=_family(
        dict(rls_trace_route_scratch_bytes=3, rls_trace_route_hits=4, rls_trace_route_gather=4, rls_trace_route_scatter=4,
             rls_trace_route_fill=6),
        structs=("rls_hit_routes", "rls_route_planes"),
        callables=("route_hits", "HitRoutes", "route_gather", "route_scatter", "route_fill", "route_scratch_bytes"),
        snippet='rls_hit_routes r = {2, 0, 0, 0, 0, 0}; rls_route_planes p = {0, 0, {0}, {0}, {0}, {0}};\n'
                '  size_t b = 0; float v[3] = {0.0f, 0.0f, 0.0f}; float *d[3] = {0, 0, 0};\n'
                '  return rls_trace_route_scratch_bytes(1, 2, &b) + rls_trace_route_hits(0, 0, 0, &r) +\n'
                '         rls_trace_route_gather(0, 0, 0, &p) + rls_trace_route_scatter(0, 0, 0, &p) +\n'
                '         rls_trace_route_fill(0, 0, 0, 3, d, v) + (RLS_ROUTE_MAX_BINS == 16 ? 0 : 1);',
        free=("route_count_kernel", "route_place_kernel", "route_gather_kernel", "route_scatter_kernel", "route_fill_kernel")),
)


def every(key):
    """one column of the table over all families: the merged dict for "arity", else the concatenated tuple"""
    if key == "arity":
        return {name: n for f in FAMILIES.values() for name, n in f["arity"].items()}
    return tuple(x for f in FAMILIES.values() for x in f[key])
