"""Timing of the caller-traced integrators (rlshaders_amd/trace.py): emit and resolve of rlGgx's integrateGlossy and
integrateRefract, with rls_ggx_integrate / rls_ggx_integrate_refract on the same batch in the same process; with
--closure disney those of rlDisney's two lobes, with rls_disney_integrate (reduced, both lobes) on the same batch; with
--closure sss rlSss's probe-ray emit and scatter resolve, with rls_sss_integrate_scatter on the same batch.

    python tools/trace_bench.py [--closure ggx|disney|sss|sss-walk|sss-hits|ggx-lights|disney-lights|ggx-node|disney-node|skin-node|ggx-bounce|disney-bounce|skin-bounce|shadow-fold|shadow-walk|route|nearest|nearest-refit|nearest-rebuild|nearest-group|nearest-any] [--mix even|skewed|one] [--log2n 24] [--spp-n 4] [--repeats 5] [--warmup 2] [--fast] [--state camera|secondary|half]

Prints one JSON line: ms per call (median over the repeats, device events, after the warm-up), rays per second, the
algorithmic bytes of each call over its time and as a fraction of 8 TB/s, and emit time / integrate time.  Byte accounting:
emit writes 12 (dir) + 12 (weight; refraction 4) + 4 (point) + 1 (sample) [+ 1 (kind)] B per kept ray; with its staging it
also writes 12 + 12 (4) + 2 B per sample and reads them back per kept ray (`*_with_staging`).  Resolve reads 12 (radiance) +
12 (weight; refraction 4) B per ray and 8 B per point (offsets) and writes 12 B per point.  The radiance is uniform random.
An rlDisney lobe is accounted as glossy (3 weight planes, no kind).  Its record has integrate_ms (both lobes in one call)
and per lobe emit_over_integrate; "emits_over_integrate" is (emit_diffuse + emit_glossy) / integrate.
rlSss: the emit writes 12 (origin) + 12 (dir) + 4 (maxdist) + 4 (point) + 1 (sample) = 33 B per ray, every ray (the queue is
dense); the resolve reads 1 B of count per ray plus 12 (P) + 12 (N) + 12 (irradiance) = 36 B per reported hit slot.  Its
hits come from a plane intersected with torch on the device (the shading points lie on the plane z = 0, lit from +z):
timing needs plausible hits, not the oracle's.
--closure sss-walk: the probe walk (rlshaders_amd.walk, librls_walk.so) on --closure sss's closure with the shading points on a
sphere of radius 0.5 about the origin (the plane ends every walk after one hit): rls_walk_begin, then step by step over a torch
closest-hit tracer -- the active count, the nearest hits, the accepted hits, the survivors, the step's time (the tracer's is
outside the events) and the bytes it moves -- the sum over the walk, and sss_probe_emit and sss_scatter_resolve from the same
process.  Medians of at least 9 whole walks after at least 3 warm-up walks, device events.

--closure sss-hits: the same plane and probe hits (about 0.5 a ray) shaded through the caller's tracer (trace.sss_hit_rays,
HitQueues.resolve) under --lights lights at --hit-spp-n^2 samples a light (default 1), with the diffuse ray: the hits emit (the
gate, the list, both queues) and the resolve, uniform random visibility and radiance; hit_capacity is the ray count (one slot a
ray).  Beside them rls_trace_ggx_direct_emit over as many POINTS as there were listed hits (the hits' positions and normals,
wo = N, diffuseRoughness 0) at the same lights and samples: the light loop alone, point-major, with its specular lobe.
--closure ggx-lights / disney-lights: the shadow-ray emit and the visibility resolve of the node's light loop
(trace.ggx_shadow_rays / disney_shadow_rays, ShadowQueue.resolve) next to rls_ggx_direct_lighting / rls_disney_direct_lighting on
the same batch: --lights spherical lights (default 2, MIS on) over shading points in the slab [0,4) x [0,4) x [0,1), a uniform
random coloured visibility.  A kept ray is 12 (dir) + 4 (maxdist) + 12 (weight_specular) + 4 or 12 (weight_diffuse: rlGgx
one plane, rlDisney three) + 1 (kind) + 4 (point) + 1 (sample) = 38 / 46 B; the staging holds a 4 B tag for every one of the
lights x 3 x spp slots of a point and 32 / 40 B per kept ray, read back by the compaction.  `kept` is rays / slots.
--closure ggx-node / disney-node: the whole node (trace.ggx_node_rays / disney_node_rays) on the batch of the light-loop runs
(the slab, --lights lights, per-point parameters; rlGgx with KtColor, Kt U[0,1)): the node emit (all queues, one call), the
light loop's share of it (the same kernels through the light-loop emit), the node resolve (one launch), the SEPARATE existing
resolves on the same queues (the light-loop resolve plus one glossy / refraction resolve per ray queue: they write one sum
per queue and leave the composition to the caller), and rls_ggx_shade / rls_disney_shade.  Uniform random radiance and
visibility.  The queues share one scratch block.
--closure ggx-bounce / disney-bounce: the node at the hits of secondary rays (trace.ggx_bounce_rays / disney_bounce_rays) on the
ggx-node / disney-node batch, under --state: `camera` (every point a camera ray at depth 0: the node call's rays, so the
difference to it is what the per-point switches cost), `secondary` (every point a glossy ray's hit at depth 1: no indirect
rays) or `half` (the two alternating point by point: neighbouring lanes differ); GI depths total 8, diffuse 2, glossy 2,
refraction 4.  The node call's emit and resolve are timed in the SAME process, before and after the bounce call's: the
difference between the node call's two figures is the spread to read the bounce call's against.
--closure skin-node: the rlSkin node (trace.skin_node_rays) with per-point parameters on the plane z = 0 (shading points in
[0,4) x [0,4), the plane lit from +z) under --lights lights: the node emit (five queues, one call), the node resolve (one
launch; uniform random visibility and radiance, the probe hits of the plane intersected with torch on the device),
rls_skin_integrate on the same batch, and the existing stand-alone resolves that fit the node's queues -- one glossy resolve
per lobe and the scatter resolve.  The lobes' shadow queues (one sum per light, no diffuse planes) have no stand-alone
resolve, and there is no compose kernel for this node: `separate_partial_ms` is a LOWER bound on a separate-kernels path.
--closure skin-bounce: the rlSkin node at the hits of secondary rays (trace.skin_bounce_rays) on the skin-node batch under
--state (`camera`: the node call's rays and an empty diffuse_shadow; `secondary`: every point a glossy ray's hit at depth 1, no
glossy rays; `half`: the two alternating; `diffuse`: every point a diffuse ray's hit, the Oren-Nayar light loop in place of the
probe walk), the node call beside it in the same process as for the other two nodes.
--closure shadow-fold: rls_trace_shadow_visibility (trace.shadow_visibility) over 2^log2n shadow rays at max_hits 4, counts
uniform in 0 .. 4, stride = rays, uniform random opacities, no base: `direct` (an opacity per element) and `indexed` (an index
per element into a table of 4096 surfaces).  Bytes, direct: 1 (count) + 12 per hit read, 12 written per ray; indexed: 1 +
(4 (index) + 12 (the table's entry, from cache)) per hit read, 12 written per ray.  --spp-n is not read.
--closure shadow-walk: the shadow walk (rlshaders_amd.shadow_walk, librls_shadow_walk.so) over --closure shadow-fold's rays and
surfaces in its indexed form: 2^log2n rays, ray j crossing count[j] (uniform in 0 .. 4) of the table's 4096 surfaces one unit of
distance apart, no base.  Step k hands every listed ray its k-th surface (a hit while k < count[j]); the hits are prepared outside
the timed calls.  begin, every step (median, fastest, slowest of at least 9 runs after at least 3 warm-up runs, device events) and
their sum, beside rls_trace_shadow_visibility over the same hits given as a list, whose visibility the walk's must equal byte for
byte.  Bytes of a step: 34 per listed ray (ray, maxdist, steps, hit, T read; state and left written; ray and state read again by
the place kernel), 32 per hit (t, index, the table's entry from cache, T written), 61 per survivor (found.P, dir, left read; ray,
steps, origin, dir, maxdist written).  --spp-n is not read.
--closure route: routing 2^log2n traced rays to 3 node bins and the misses (trace.route_hits, HitRoutes) at --mix even (a
quarter of the rays in each bin and a quarter misses), skewed (70 / 20 / 9 % and 1 % misses) or one (every ray in bin 0):
route_hits without and with slot, a 12-plane gather and a 3-plane scatter of bin 0, the fill of the misses' 3 planes.  Beside
each the device-to-device copy (torch copy_) that moves the verb's algorithmic traffic, half of it read and half written --
route: 2 B read + 4 B written per ray, + 4 B with slot; gather / scatter: 4 B of index + 8 B per word plane per element; fill:
4 B of index + 4 B per plane per element.  Medians of at least 9 calls after at least 3 warm-up calls, device events, with the
fastest and slowest call beside them.  --spp-n is not read.
--closure nearest-refit: moving meshes (rlshaders_amd.nearest_refit, librls_nearest_refit.so).  "update": Refit.update on device
vertices (the mesh twisted about y by 0.5 radians) against nearest.Scene(...) creation on the same vertices -- a host clock around
the build, the upload and a synchronise, the median of 3 -- at the --level icosphere (6: 81 920 triangles) and at a grid of
2 * 724^2 triangles; the update with the tree's top folded into one single-workgroup launch and with one launch per level
(RLS_NEAREST_REFIT_FOLD=0), the two alternating twice, each the median, fastest and slowest of at least 9 calls after 3 warm-up
calls, device events.  "queries": --closure nearest's coherent and incoherent streams of 2^log2n rays on the tree refit to the
icosphere twisted by 0.5 and by 2 radians and on a tree rebuilt from the twisted vertices, and their ratio; same_as_refit: the two
trees' hit and t planes are the same bytes.  --spp-n is not read.
--closure nearest-rebuild: the tree rebuilt on the device (rlshaders_amd.nearest_rebuild, librls_nearest_rebuild.so), on the two
meshes of --closure nearest-refit.  "update": Rebuild.update on device vertices (the mesh twisted by 0.5 radians) beside
Refit.update on the same vertices, each the median, fastest and slowest of at least 9 calls after 3 warm-up calls, device events,
and beside nearest.Scene(...) creation on them (the only rebuild there was: a host clock around the build, the upload and a
synchronise, the median of 9 after 3); the launches of an update and the bytes of its working set.  "queries": --closure
nearest's two streams after the 0.5 and the 2 radian twist on the refit tree, on the device-rebuilt tree and on a host-rebuilt
one (a fresh scene); same_as_host_rebuilt: every found plane of the device-rebuilt tree's queries is the fresh scene's bytes.
--spp-n is not read.
--closure nearest-group: instanced scenes (rlshaders_amd.nearest_group, librls_nearest_group.so).  --instances copies of the
--level icosphere (rigidly turned, on a cubic grid 2.5 radii apart) under one Group, queried by a camera grid's rays (coherent)
and by uniformly distributed rays from the points they hit with the pair last / last_instance set (incoherent), 2^log2n each.
Beside each (a) "flat": the same geometry baked into ONE nearest.Scene (where it fits 2^22 triangles), the same rays, and the
share of rays whose hit flag agrees; (b) "alone": --closure nearest's camera on one instance, through a Group of one and through
the plain Scene -- what the second level costs a ray.  "update": Group.update with both matrix planes against baking the
vertices on the device (a batched matrix product) + Rebuild.update of the flat scene; the device bytes of the group and of the
flat scene.  Medians, fastest and slowest of at least 9 calls after 3 warm-up calls, device events.  --spp-n is not read.
--closure nearest-any: any-hit shadow queries (rlshaders_amd.nearest_any, librls_nearest_any.so).  (a) "streams": --closure
nearest's coherent and incoherent streams of 2^log2n rays on the --level icosphere, given finite reaches, through rls_nearest_hits
(hit, t, P, surface: what the shadow walk's tracer asks for) and through rls_nearest_any_hits (state, visibility, reach), and their
ratio.  (b) "opaque": a --closure ggx-lights shadow queue (--lights, --spp-n) through an opaque icosphere above the points: ONE
any-hit launch against shadow_walk.run over nearest.tracer with an all-ones table (its rounds, and the host's reads of the active
count, inside the events); same_visibility: the two planes are the same bytes.  (c) "mixed": a translucent shell about the opaque
sphere: nearest_any.shadow (the launch, the flags, the walk on the veiled rays) against the full walk, the share of rays walked,
same_open_rays: the clear and veiled rays' visibility is the same bytes; blocked_not_zero / walk_blocked_not_zero: the blocked rays
whose visibility is not all zero after the two-phase route (none, by construction) and after the full walk (a ray that grazes the
opaque surface may miss it from its moved origin); "any" / "nearest": one any-hit and one nearest-hit launch
over the queue's rays on that scene.  Medians, fastest and slowest of at least 9 calls
after 3 warm-up calls, device events.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_TBPS = 8.0


def timed(fn, repeats: int, warmup: int) -> float:
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2]


def rate(bytes_, ms):
    return round(bytes_ / (ms * 1e-3) / 1e12, 4)


def accounting(n: int, spp: int, rays: int, ms_emit: float, ms_res: float, refract: bool) -> dict:
    """ms per call, rays per second and the algorithmic bytes of one emit and one resolve (module docstring)"""
    wb = 4 if refract else 12
    per_ray = 12 + wb + 4 + 1 + (1 if refract else 0)
    emit_bytes = rays * per_ray
    staging = n * spp * (12 + wb + 2) + rays * (12 + wb + 2) + n * spp * 2 + n * 8 * 4   # + tags read, offsets scan
    res_bytes = rays * (12 + wb) + n * 8 + n * 12
    return {
        "emit_ms": round(ms_emit, 4), "resolve_ms": round(ms_res, 4),
        "emit_rays_per_s": round(rays / (ms_emit * 1e-3), 1), "resolve_rays_per_s": round(rays / (ms_res * 1e-3), 1),
        "emit_tb_per_s": rate(emit_bytes, ms_emit), "emit_tb_per_s_with_staging": rate(emit_bytes + staging, ms_emit),
        "emit_frac_of_8tbps_with_staging": round(rate(emit_bytes + staging, ms_emit) / HBM_TBPS, 4),
        "resolve_tb_per_s": rate(res_bytes, ms_res), "resolve_frac_of_8tbps": round(rate(res_bytes, ms_res) / HBM_TBPS, 4),
    }


def bench_disney(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """rlDisney (BASELINE config 3's inputs: every parameter U[0,1) per point): each lobe's emit and resolve against
    rls_disney_integrate in reduced mode"""
    import torch
    import rlshaders_amd as R
    from rlshaders_amd import trace as T
    wo, N, T_ = R.gen_frame(ctx, seed, 0, n)
    u = lambda stream: R.gen_uniform(ctx, seed, 0, n, stream)
    base = torch.stack([u(8 + j) for j in range(3)])
    d = R.DisneySampler(ctx, wo, N, T_, base_color=base, **{k: u(32 + j) for j, k in enumerate(R._capi.DISNEY_SCALARS)})
    sums = d.integrate(spp_n, seed)
    ms_int = timed(lambda: d.integrate(spp_n, seed, out=sums), args.repeats, args.warmup)
    rec["integrate_ms"] = round(ms_int, 4)
    out = ctx.empty(3, n)
    emits = 0.0
    for name, lobe in (("diffuse", R.RLS_RAY_DIFFUSE), ("glossy", R.RLS_RAY_GLOSSY)):
        q = T.RayQueue(ctx, n, spp_n, lobe=lobe)
        ms_emit = timed(lambda: T.disney_rays(d, lobe, spp_n, seed, queue=q), args.repeats, args.warmup)
        rays = q.count
        L = torch.rand(3, max(rays, 1), device=ctx.torch_device)
        ms_res = timed(lambda: q.resolve(L, out=out, count=rays), args.repeats, args.warmup)
        rec[name] = {"rays": rays, "rays_per_point": round(rays / n, 4)}
        rec[name].update(accounting(n, spp_n * spp_n, rays, ms_emit, ms_res, False))
        rec[name]["emit_over_integrate"] = round(ms_emit / ms_int, 4)
        emits += ms_emit
        del q, L
        torch.cuda.empty_cache()
    rec["emits_over_integrate"] = round(emits / ms_int, 4)


def bench_sss(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """rlSss on the plane z = 0: the probe-ray emit and the scatter resolve of device-traced hits against
    rls_sss_integrate_scatter over the same analytic plane"""
    import math
    import torch
    import rlshaders_amd as R
    from rlshaders_amd import trace as T
    g = torch.Generator(device=ctx.torch_device).manual_seed(seed)
    dev = ctx.torch_device
    Ns = torch.zeros(3, n, device=dev)
    Ns[2] = 1
    ang = torch.rand(n, device=dev, generator=g) * (2 * math.pi)
    Tg = torch.stack([torch.cos(ang), torch.sin(ang), torch.zeros_like(ang)]).contiguous()
    P = torch.zeros(3, n, device=dev)
    P[:2] = torch.rand(2, n, device=dev, generator=g)
    s = R.SssSampler(ctx, Ns, Tg, (0.8, 0.5, 0.3), (0.05, 0.1, 0.2))
    sc = R.make_scene("plane", light_dir=(0, 0, 1), light_color=(1.0, 1.0, 1.0))
    res = ctx.empty(3, n)
    ms_int = timed(lambda: s.integrateScatter(P, sc, spp_n, seed, out=res), args.repeats, args.warmup)
    q = T.ProbeQueue(ctx, n, spp_n)
    ms_emit = timed(lambda: T.sss_probe_rays(s, P, spp_n, seed, queue=q), args.repeats, args.warmup)
    O, D, md = q.origin, q.dir, q.maxdist
    with torch.no_grad():
        t = -O[2] / D[2]
        ok = (D[2] != 0) & (t > 0) & (t <= md)
        hP = (O + D * t).unsqueeze(1).contiguous()
        hN = torch.zeros_like(hP)
        hN[2] = 1
        E = torch.full_like(hP, 1.0 / math.pi)
        cnt = ok.to(torch.uint8)
    hits = int(cnt.sum().item())
    ms_res = timed(lambda: q.resolve(cnt, hP, hN, E, out=res), args.repeats, args.warmup)
    rays = q.count
    emit_bytes, res_bytes = rays * 33, rays * 1 + hits * 36
    rec["sss"] = {
        "rays": rays, "hits_per_ray": round(hits / rays, 4), "integrate_ms": round(ms_int, 4),
        "emit_ms": round(ms_emit, 4), "resolve_ms": round(ms_res, 4),
        "emit_rays_per_s": round(rays / (ms_emit * 1e-3), 1), "resolve_rays_per_s": round(rays / (ms_res * 1e-3), 1),
        "emit_tb_per_s": rate(emit_bytes, ms_emit), "emit_frac_of_8tbps": round(rate(emit_bytes, ms_emit) / HBM_TBPS, 4),
        "resolve_tb_per_s": rate(res_bytes, ms_res), "resolve_frac_of_8tbps": round(rate(res_bytes, ms_res) / HBM_TBPS, 4),
        "emit_over_integrate": round(ms_emit / ms_int, 4),
        "emit_plus_resolve_over_integrate": round((ms_emit + ms_res) / ms_int, 4),
    }


def bench_sss_walk(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """bench_sss's closure on a sphere (module docstring, --closure sss-walk): the probe walk step by step"""
    import math
    import torch
    import rlshaders_amd as R
    from rlshaders_amd import build, trace as T, walk as W
    build.build_walk_library()
    repeats, warmup = max(args.repeats, 9), max(args.warmup, 3)
    dev, radius = ctx.torch_device, 0.5
    _, Ns, Tg = R.gen_frame(ctx, seed, 0, n)
    P = (Ns * radius).contiguous()
    s = R.SssSampler(ctx, Ns, Tg, (0.8, 0.5, 0.3), (0.05, 0.1, 0.2))
    q = T.ProbeQueue(ctx, n, spp_n)
    res = ctx.empty(3, n)
    ms_emit = timed(lambda: T.sss_probe_rays(s, P, spp_n, seed, queue=q), repeats, warmup)
    rays = q.count
    w = W.ProbeWalk(ctx, q, P)

    def closest(r, m):
        """the renderer: the sphere's closest hit in (0, maxdist] of the first m listed rays"""
        o, d, md = r.origin[:, :m], r.dir[:, :m], r.maxdist[:m]
        a, b, c = (d * d).sum(0), (o * d).sum(0), (o * o).sum(0) - radius * radius
        sq = (b * b - a * c).clamp_min(0).sqrt()
        t0, t1 = (-b - sq) / a, (-b + sq) / a
        t = torch.where(t0 > 0, t0, t1)
        hit = (b * b - a * c >= 0) & (t > 0) & (t <= md)
        hp = (o + d * t).contiguous()
        nrm = (hp / radius).contiguous()
        return W.Found(hit.to(torch.uint8), t.contiguous(), hp, nrm, nrm), int(hit.sum().item())

    steps, begin_ms = [], []
    for run in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        w.begin()
        b.record()
        b.synchronize()
        begin_ms.append(a.elapsed_time(b))
        for k in range(W.RLS_WALK_TRIALS):
            m = w.active
            if m == 0:
                break
            found, hits = closest(w.rays, m)
            stored = int(w.hit_count.sum(dtype=torch.int64).item())
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            w.step(found, bound=m)
            b.record()
            b.synchronize()
            if k == len(steps):
                steps.append({"active": m, "hits": hits, "ms": []})
            if run >= warmup:
                steps[k]["ms"].append(a.elapsed_time(b))
            if run == warmup:
                steps[k]["accepted"] = int(w.hit_count.sum(dtype=torch.int64).item()) - stored
                steps[k]["survivors"] = w.active
    total_ms = total_bytes = 0.0
    for st in steps:
        ms = sorted(st.pop("ms"))
        # per listed ray, the step kernel reads ray 4, maxdist 4, trials 1, hit 1, count 1, prev 12 and writes flag 1, left 4; the
        # place kernel reads ray 4 and flag 1 again: 33.  A hit: t 4, P / N / Ns 36.  An accepted hit: P / N 24 and count 1
        # written.  A survivor: found.P 12, dir 12, left 4 read, ray 4, trials 1, origin 12, dir 12, maxdist 4 written: 61.
        bytes_ = st["active"] * 33 + st["hits"] * 40 + st["accepted"] * 25 + st["survivors"] * 61
        st.update(ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), bytes=bytes_,
                  tb_per_s=rate(bytes_, ms[len(ms) // 2]))
        total_ms += st["ms"]
        total_bytes += bytes_
    begin_ms = sorted(begin_ms[warmup:])
    cnt, hP, hN, _ = w.hits()
    E = torch.full((3, w.max_hits, rays), 1.0 / math.pi, device=dev)
    ms_res = timed(lambda: q.resolve(cnt, hP, hN, E, out=res), repeats, warmup)
    # the copy DESIGN section 5 measures the kernels against, over as many bytes as the first step moves
    a_, b_ = (torch.empty(max(steps[0]["bytes"] // 2, 1), dtype=torch.uint8, device=dev) for _ in range(2))
    copy = timed_spread(lambda: b_.copy_(a_), repeats, warmup)
    rec["sss-walk"] = {
        "rays": rays, "repeats": repeats, "warmup": warmup, "begin_ms": round(begin_ms[len(begin_ms) // 2], 4),
        "begin_tb_per_s": rate(rays * 7 + steps[0]["active"] * 61, begin_ms[len(begin_ms) // 2]), "steps": steps,
        "walk_ms": round(total_ms, 4), "walk_bytes": int(total_bytes), "walk_tb_per_s": rate(total_bytes, total_ms),
        "hits_per_ray": round(int(cnt.sum(dtype=torch.int64).item()) / max(rays, 1), 4),
        "emit_ms": round(ms_emit, 4), "resolve_ms": round(ms_res, 4),
        "walk_over_emit_plus_resolve": round((total_ms + begin_ms[len(begin_ms) // 2]) / (ms_emit + ms_res), 4),
        "copy_of_first_step_bytes_ms": copy["ms"], "copy_tb_per_s": rate(steps[0]["bytes"], copy["ms"]),
    }


def bench_sss_hits(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """bench_sss's plane and hits, lit through the hit verbs; the rlGgx light-loop emit over as many points beside them"""
    import math
    import torch
    import rlshaders_amd as R
    from rlshaders_amd import trace as T
    from rlshaders_amd.closures import make_light
    g = torch.Generator(device=ctx.torch_device).manual_seed(seed)
    dev = ctx.torch_device
    nl, hs = args.lights, args.hit_spp_n
    lights = [make_light(center=c, radius=r, radiance=e) for c, r, e in LIGHT_SPECS[:nl]]
    Ns = torch.zeros(3, n, device=dev)
    Ns[2] = 1
    ang = torch.rand(n, device=dev, generator=g) * (2 * math.pi)
    Tg = torch.stack([torch.cos(ang), torch.sin(ang), torch.zeros_like(ang)]).contiguous()
    P = torch.zeros(3, n, device=dev)
    P[:2] = torch.rand(2, n, device=dev, generator=g)
    s = R.SssSampler(ctx, Ns, Tg, (0.8, 0.5, 0.3), (0.05, 0.1, 0.2))
    q = T.sss_probe_rays(s, P, spp_n, seed)
    O, D, md = q.origin, q.dir, q.maxdist
    with torch.no_grad():
        t = -O[2] / D[2]
        ok = (D[2] != 0) & (t > 0) & (t <= md)
        hP = torch.where(ok, O + D * t, torch.zeros_like(O)).unsqueeze(1).contiguous()
        hN = torch.zeros_like(hP)
        hN[2] = 1
        hT = torch.zeros_like(hP)
        hT[0] = 1
        cnt = ok.to(torch.uint8)
    rays = q.count
    hq = T.HitQueues(ctx, n, spp_n, 1, rays, rays, nl, hs, True)
    emit = lambda: T.sss_hit_rays(s, P, q, cnt, hP, hN, lights, hs, seed, hitT=hT, trace_diffuse=True, queues=hq)
    ms_emit = timed(emit, args.repeats, args.warmup)
    listed, sc, dc = hq.listed, hq.shadow_count, hq.diffuse_count
    vis = torch.rand(3, max(sc, 1), device=dev)
    rad = torch.rand(3, max(dc, 1), device=dev)
    E = ctx.empty(3, 1, rays)
    ms_res = timed(lambda: hq.resolve(vis, rad, out=E, counts=(sc, dc)), args.repeats, args.warmup)
    # the light loop alone over `listed` points: the listed hits as an rlGgx batch
    el = hq.hit_element
    gP, gN, gT = (x.reshape(3, -1)[:, el].contiguous() for x in (hP, hN, hT))
    m = max(listed, 1)
    gg = R.GgxSampler(ctx, gN, gN, gT, specColor=(0.9, 0.5, 0.3), ior=1.45, roughness=0.3) if listed else None
    ms_ggx, ggx_rays = float("nan"), 0
    if gg is not None:
        sh = T.ggx_shader(gg, KdColor=(1.0, 1.0, 1.0), Kd=1.0, diffuseRoughness=0.0, Ks=0.5)
        gq = T.ShadowQueue(ctx, m, nl, hs)
        ms_ggx = timed(lambda: T.ggx_shadow_rays(gg, sh, gP, lights, hs, seed, queue=gq), args.repeats, args.warmup)
        ggx_rays = gq.count
    out_rays = sc + dc
    rec["lights"], rec["hit_spp_n"] = nl, hs
    rec["sss-hits"] = {
        "probe_rays": rays, "hit_capacity": rays, "listed_hits": listed, "hits_per_ray": round(listed / rays, 4),
        "shadow_rays": sc, "diffuse_rays": dc, "emit_ms": round(ms_emit, 4), "resolve_ms": round(ms_res, 4),
        "emit_rays_per_s": round(out_rays / (ms_emit * 1e-3), 1), "resolve_rays_per_s": round(out_rays / (ms_res * 1e-3), 1),
        "emit_hits_per_s": round(listed / (ms_emit * 1e-3), 1),
        "ggx_direct_emit_ms_over_listed_points": round(ms_ggx, 4), "ggx_direct_emit_rays": ggx_rays,
        "emit_over_ggx_direct_emit": round(ms_emit / ms_ggx, 4),
    }


LIGHT_SPECS = (((2.0, 2.0, 3.0), 1.25, (3.0, 2.0, 1.0)), ((1.0, 5.0, 4.0), 1.0, (5.0, 1.0, 1.0)), ((-3.0, 1.0, 2.5), 0.5, (0.5, 4.0, 2.0)),
               ((0.5, -2.5, 6.0), 2.0, (1.0, 1.0, 6.0)), ((6.0, -1.0, 1.5), 0.8, (0.3, 0.6, 0.9)), ((-1.0, -1.0, 8.0), 3.0, (0.7, 0.7, 0.2)),
               ((5.0, 5.0, 5.0), 1.5, (1.0, 2.0, 3.0)), ((-2.0, 6.0, 3.0), 1.0, (2.0, 1.0, 0.5)))


def bench_lights(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """the light loop of rlGgx or rlDisney (per-point parameters U[0,1) like the other closures' batches): emit and resolve
    against the analytic direct-lighting call"""
    import torch
    import rlshaders_amd as R
    from rlshaders_amd import trace as T
    from rlshaders_amd.closures import make_light
    disney = args.closure == "disney-lights"
    nl = args.lights
    lights = [make_light(center=c, radius=r, radiance=e) for c, r, e in LIGHT_SPECS[:nl]]
    wo, N, T_ = R.gen_frame(ctx, seed, 0, n)
    u = lambda stream, lo=0.0, hi=1.0: R.gen_uniform(ctx, seed, 0, n, stream, lo, hi)
    P = torch.stack([u(60, 0.0, 4.0), u(61, 0.0, 4.0), u(62)]).contiguous()
    out = (ctx.empty(3, n), ctx.empty(3, n))
    if disney:
        base = torch.stack([u(8 + j) for j in range(3)])
        s = R.DisneySampler(ctx, wo, N, T_, base_color=base, **{k: u(32 + j) for j, k in enumerate(R._capi.DISNEY_SCALARS)})
        analytic = lambda: s.directLighting(P, lights, spp_n, seed, out=out)
        q = T.ShadowQueue(ctx, n, nl, spp_n, disney=True)
        emit = lambda: T.disney_shadow_rays(s, P, lights, spp_n, seed, queue=q)
    else:
        ks = torch.stack([u(10 + k) for k in range(3)])
        s = R.GgxSampler(ctx, wo, N, T_, specColor=ks, ior=u(13, 1.05, 2.55), roughness=u(14, 0.05, 1.0),
                         anisotropic=R.gen_aniso(ctx, seed, 0, n))
        shp = dict(KdColor=torch.stack([u(20 + k) for k in range(3)]), Kd=u(23), diffuseRoughness=u(24), Ks=u(25))
        sh = T.ggx_shader(s, **shp)
        analytic = lambda: s.directLighting(P, lights, spp_n, seed, out=out, **shp)
        q = T.ShadowQueue(ctx, n, nl, spp_n)
        emit = lambda: T.ggx_shadow_rays(s, sh, P, lights, spp_n, seed, queue=q)
    ms_int = timed(analytic, args.repeats, args.warmup)
    ms_emit = timed(emit, args.repeats, args.warmup)
    rays = q.count
    vis = torch.rand(3, max(rays, 1), device=ctx.torch_device)
    res = (ctx.empty(3, n), ctx.empty(3, n))
    ms_res = timed(lambda: q.resolve(vis, out=res, count=rays), args.repeats, args.warmup)
    slots = n * nl * 3 * spp_n * spp_n
    wd = 12 if disney else 4
    per_ray = 12 + 4 + 12 + wd + 1 + 4 + 1
    staged = 12 + 4 + 12 + wd
    emit_bytes = rays * per_ray
    staging = slots * 4 * 2 + rays * staged * 2 + n * 8 * 4          # tags written and read, kept records likewise, the scan
    res_bytes = rays * (12 + 12 + wd + 1) + n * 8 + n * 24
    rec["lights"] = nl
    rec[args.closure] = {
        "rays": rays, "rays_per_point": round(rays / n, 4), "kept": round(rays / slots, 4), "bytes_per_ray": per_ray,
        "analytic_ms": round(ms_int, 4), "emit_ms": round(ms_emit, 4), "resolve_ms": round(ms_res, 4),
        "emit_rays_per_s": round(rays / (ms_emit * 1e-3), 1), "resolve_rays_per_s": round(rays / (ms_res * 1e-3), 1),
        "emit_tb_per_s": rate(emit_bytes, ms_emit), "emit_tb_per_s_with_staging": rate(emit_bytes + staging, ms_emit),
        "emit_bytes_with_staging": emit_bytes + staging,
        "resolve_tb_per_s": rate(res_bytes, ms_res), "resolve_frac_of_8tbps": round(rate(res_bytes, ms_res) / HBM_TBPS, 4),
        "emit_over_analytic": round(ms_emit / ms_int, 4),
        "emit_plus_resolve_over_analytic": round((ms_emit + ms_res) / ms_int, 4),
    }


def bench_node(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """the whole rlGgx or rlDisney node on bench_lights' batch: emit, fused resolve, the separate resolves, the analytic call"""
    import torch
    import rlshaders_amd as R
    from rlshaders_amd import trace as T
    from rlshaders_amd.closures import make_light
    disney = args.closure == "disney-node"
    nl = args.lights
    lights = [make_light(center=c, radius=r, radiance=e) for c, r, e in LIGHT_SPECS[:nl]]
    wo, N, T_ = R.gen_frame(ctx, seed, 0, n)
    u = lambda stream, lo=0.0, hi=1.0: R.gen_uniform(ctx, seed, 0, n, stream, lo, hi)
    P = torch.stack([u(60, 0.0, 4.0), u(61, 0.0, 4.0), u(62)]).contiguous()
    if disney:
        base = torch.stack([u(8 + j) for j in range(3)])
        s = R.DisneySampler(ctx, wo, N, T_, base_color=base, **{k: u(32 + j) for j, k in enumerate(R._capi.DISNEY_SCALARS)})
        aov = {k: ctx.empty(3, n) for k in s.SHADE_AOVS + ("out",)}
        analytic = lambda: s.shade(P, lights, spp_n, seed, out=aov)
        nq = T.DisneyNodeQueues(ctx, n, nl, spp_n, share_scratch=True)
        emit = lambda: T.disney_node_rays(s, P, lights, spp_n, seed, queues=nq)
        shadow_emit = lambda: T.disney_shadow_rays(s, P, lights, spp_n, seed, queue=nq.shadow)
    else:
        ks = torch.stack([u(10 + k) for k in range(3)])
        s = R.GgxSampler(ctx, wo, N, T_, specColor=ks, ior=u(13, 1.05, 2.55), roughness=u(14, 0.05, 1.0),
                         anisotropic=R.gen_aniso(ctx, seed, 0, n))
        shp = dict(KdColor=torch.stack([u(20 + k) for k in range(3)]), Kd=u(23), diffuseRoughness=u(24), Ks=u(25),
                   KtColor=torch.stack([u(26 + k) for k in range(3)]), Kt=u(29))
        sh = T.ggx_shader(s, **shp)
        aov = {k: ctx.empty(3, n) for k in s.SHADE_AOVS + ("out",)}
        analytic = lambda: s.shade(P, lights, spp_n, seed, out=aov, **shp)
        nq = T.GgxNodeQueues(ctx, n, nl, spp_n, share_scratch=True)
        emit = lambda: T.ggx_node_rays(s, sh, P, lights, spp_n, seed, queues=nq)
        shadow_emit = lambda: T.ggx_shadow_rays(s, sh, P, lights, spp_n, seed, queue=nq.shadow)
    ms_int = timed(analytic, args.repeats, args.warmup)
    ms_shadow = timed(shadow_emit, args.repeats, args.warmup)
    ms_emit = timed(emit, args.repeats, args.warmup)
    cnt = nq.counts()
    planes = [torch.rand(3, max(cnt[r], 1), device=ctx.torch_device) for r in ("shadow",) + nq.RAYS]
    res = {k: ctx.empty(3, n) for k in aov}
    ms_res = timed(lambda: nq.resolve(*planes, out=res, counts=cnt), args.repeats, args.warmup)
    # the same entry point as the existing resolve kernels plus a compose kernel (RLS_NODE_RESOLVE=separate: plain sums)
    import os
    os.environ["RLS_NODE_RESOLVE"] = "separate"
    try:
        ms_res_sep = timed(lambda: nq.resolve(*planes, out=res, counts=cnt), args.repeats, args.warmup)
    finally:
        del os.environ["RLS_NODE_RESOLVE"]
    # the separate existing resolves on the same queues, each timed on its own and all of them back to back
    two = (ctx.empty(3, n), ctx.empty(3, n))
    sums = [ctx.empty(3, n) for _ in nq.RAYS]
    parts = [lambda: nq.shadow.resolve(planes[0], out=two, count=cnt["shadow"])]
    for j, r in enumerate(nq.RAYS):
        parts.append(lambda j=j, r=r: getattr(nq, r).resolve(planes[1 + j], out=sums[j], count=cnt[r]))
    ms_parts = [timed(f, args.repeats, args.warmup) for f in parts]
    ms_sep = timed(lambda: [f() for f in parts], args.repeats, args.warmup)
    rec["lights"] = nl
    rec[args.closure] = {
        "rays": cnt, "analytic_ms": round(ms_int, 4), "emit_ms": round(ms_emit, 4),
        "shadow_emit_ms": round(ms_shadow, 4), "ray_emits_ms": round(ms_emit - ms_shadow, 4),
        "node_resolve_ms": round(ms_res, 4), "node_resolve_as_separate_kernels_plus_compose_ms": round(ms_res_sep, 4),
        "separate_resolves_ms": round(ms_sep, 4),
        "separate_resolve_ms_each": dict(zip(("shadow",) + nq.RAYS, [round(m, 4) for m in ms_parts])),
        "node_resolve_over_separate": round(ms_res / ms_sep, 4), "emit_over_analytic": round(ms_emit / ms_int, 4),
        "emit_plus_resolve_over_analytic": round((ms_emit + ms_res) / ms_int, 4),
    }


def bench_bounce(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """the bounce call of rlGgx or rlDisney on bench_node's batch under --state, the node call beside it in the same process"""
    import torch
    import rlshaders_amd as R
    from rlshaders_amd import trace as T
    from rlshaders_amd.closures import make_light
    disney = args.closure == "disney-bounce"
    nl = args.lights
    lights = [make_light(center=c, radius=r, radiance=e) for c, r, e in LIGHT_SPECS[:nl]]
    wo, N, T_ = R.gen_frame(ctx, seed, 0, n)
    u = lambda stream, lo=0.0, hi=1.0: R.gen_uniform(ctx, seed, 0, n, stream, lo, hi)
    P = torch.stack([u(60, 0.0, 4.0), u(61, 0.0, 4.0), u(62)]).contiguous()
    dev = ctx.torch_device
    secondary = {"camera": torch.zeros(n, dtype=torch.bool, device=dev), "secondary": torch.ones(n, dtype=torch.bool, device=dev),
                 "half": (torch.arange(n, device=dev) % 2).to(torch.bool)}[args.state]
    depth = secondary.to(torch.uint8)
    zero = torch.zeros(n, dtype=torch.uint8, device=dev)
    rt = torch.where(secondary, torch.tensor(T.RLS_RT_GLOSSY, dtype=torch.uint8, device=dev),
                     torch.tensor(T.RLS_RT_CAMERA, dtype=torch.uint8, device=dev))
    state = T.RayState(rt, depth, zero, depth.clone(), zero.clone())
    depths = T.gi_depths((8, 2, 2, 4))
    if disney:
        base = torch.stack([u(8 + j) for j in range(3)])
        s = R.DisneySampler(ctx, wo, N, T_, base_color=base, **{k: u(32 + j) for j, k in enumerate(R._capi.DISNEY_SCALARS)})
        kd, ks = u(50), u(51)
        nq, bq = (T.DisneyNodeQueues(ctx, n, nl, spp_n, share_scratch=True) for _ in range(2))
        node_emit = lambda: T.disney_node_rays(s, P, lights, spp_n, seed, queues=nq)
        emit = lambda: T.disney_bounce_rays(s, P, lights, spp_n, seed, state, depths, queues=bq, indirectDiffuseScale=kd,
                                            indirectSpecularScale=ks)
    else:
        ksc = torch.stack([u(10 + k) for k in range(3)])
        s = R.GgxSampler(ctx, wo, N, T_, specColor=ksc, ior=u(13, 1.05, 2.55), roughness=u(14, 0.05, 1.0),
                         anisotropic=R.gen_aniso(ctx, seed, 0, n))
        shp = dict(KdColor=torch.stack([u(20 + k) for k in range(3)]), Kd=u(23), diffuseRoughness=u(24), Ks=u(25),
                   KtColor=torch.stack([u(26 + k) for k in range(3)]), Kt=u(29))
        sh = T.ggx_shader(s, **shp)
        nq, bq = (T.GgxNodeQueues(ctx, n, nl, spp_n, share_scratch=True) for _ in range(2))
        node_emit = lambda: T.ggx_node_rays(s, sh, P, lights, spp_n, seed, queues=nq)
        emit = lambda: T.ggx_bounce_rays(s, sh, P, lights, spp_n, seed, state, depths, queues=bq)
    res = {k: ctx.empty(3, n) for k in s.SHADE_AOVS + ("out",)}

    def both(q, fn):
        ms_emit = timed(fn, args.repeats, args.warmup)
        cnt = q.counts()
        planes = [torch.rand(3, max(cnt[r], 1), device=dev) for r in ("shadow",) + q.RAYS]
        ms_res = timed(lambda: q.resolve(*planes, out=res, counts=cnt), args.repeats, args.warmup)
        del planes
        return cnt, round(ms_emit, 4), round(ms_res, 4)

    _, ne0, nr0 = both(nq, node_emit)
    cnt, be, br = both(bq, emit)
    ncnt, ne1, nr1 = both(nq, node_emit)
    rec["lights"], rec["state"] = nl, args.state
    rec[args.closure] = {
        "rays": cnt, "node_rays": ncnt, "emit_ms": be, "resolve_ms": br, "node_emit_ms": [ne0, ne1], "node_resolve_ms": [nr0, nr1],
        "emit_over_node": round(be / min(ne0, ne1), 4), "resolve_over_node": round(br / min(nr0, nr1), 4),
    }


def skin_batch(args, ctx, n: int, seed: int):
    """the rlSkin batch of skin-node and skin-bounce: per-point parameters on the plane z = 0 -> (shader, P, lights, Ns, Tg, p, dist, mult)"""
    import math
    import torch
    import rlshaders_amd as R
    from rlshaders_amd.closures import make_light
    nl = args.lights
    dev = ctx.torch_device
    lights = [make_light(center=c, radius=r, radiance=e) for c, r, e in LIGHT_SPECS[:nl]]
    wo, _, _ = R.gen_frame(ctx, seed, 0, n)
    wo[2] = wo[2].abs() + 0.05
    wo = (wo / wo.norm(dim=0, keepdim=True)).contiguous()
    u = lambda stream, lo=0.0, hi=1.0: R.gen_uniform(ctx, seed, 0, n, stream, lo, hi)
    u3 = lambda stream, lo=0.0, hi=1.0: torch.stack([u(stream + k, lo, hi) for k in range(3)])
    Ns = torch.zeros(3, n, device=dev)
    Ns[2] = 1
    ang = u(63, 0.0, 2 * math.pi)
    Tg = torch.stack([torch.cos(ang), torch.sin(ang), torch.zeros_like(ang)]).contiguous()
    P = torch.stack([u(60, 0.0, 4.0), u(61, 0.0, 4.0), torch.zeros(n, device=dev)]).contiguous()
    dist, mult = u3(30, 0.02, 0.3), u(33, 0.5, 1.5)
    p = dict(sss_color=u3(10), sss_weight=u(13, 0.2, 1.0), sss_dist_multiplier=mult, sss_scatter_dist=dist,
             specular_color=u3(14), specular_weight=u(17, 0.1, 0.9), specular_roughness=u(18, 0.05, 1.0), specular_ior=u(19, 1.05, 2.0),
             sheen_color=u3(20), sheen_weight=u(23, 0.1, 0.9), sheen_roughness=u(24, 0.05, 1.0), sheen_ior=u(25, 1.05, 2.0))
    return R.SkinShader(ctx, wo, Ns, Tg, **p), P, lights, Ns, Tg, p, dist, mult


def plane_hits(pq):
    """the probe queue's rays intersected with the plane z = 0 on the device -> (count, P, N, E = 1 / pi, the hits found)"""
    import math
    import torch
    O, D, md = pq.origin, pq.dir, pq.maxdist
    with torch.no_grad():
        t = -O[2] / D[2]
        ok = (D[2] != 0) & (t > 0) & (t <= md)
        hP = (O + D * t).unsqueeze(1).contiguous()
        hN = torch.zeros_like(hP)
        hN[2] = 1
        E = torch.full_like(hP, 1.0 / math.pi)
        hc = ok.to(torch.uint8)
    return hc, hP, hN, E, int(hc.sum().item())


def bench_skin_bounce(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """the bounce call of rlSkin on the skin-node batch under --state, the node call beside it in the same process"""
    import torch
    from rlshaders_amd import trace as T
    sk, P, lights, *_ = skin_batch(args, ctx, n, seed)
    nl, dev = args.lights, ctx.torch_device
    odd = (torch.arange(n, device=dev) % 2).to(torch.bool)
    secondary = {"camera": torch.zeros_like(odd), "secondary": torch.ones_like(odd), "half": odd, "diffuse": torch.ones_like(odd)}[args.state]
    depth = secondary.to(torch.uint8)
    zero = torch.zeros(n, dtype=torch.uint8, device=dev)
    kind = T.RLS_RT_DIFFUSE if args.state == "diffuse" else T.RLS_RT_GLOSSY
    rt = torch.where(secondary, torch.tensor(kind, dtype=torch.uint8, device=dev), torch.tensor(T.RLS_RT_CAMERA, dtype=torch.uint8, device=dev))
    state = T.RayState(rt, depth, depth.clone() if args.state == "diffuse" else zero, zero.clone() if args.state == "diffuse" else depth.clone(),
                       zero.clone())
    depths = T.gi_depths((8, 2, 2, 4))
    nq, bq = T.SkinNodeQueues(ctx, n, nl, spp_n, share_scratch=True), T.SkinBounceQueues(ctx, n, nl, spp_n, share_scratch=True)
    keys3, keys1 = ("sheen", "specular", "sss", "out"), ("sheenFresnel", "specularFresnel", "sssWeight")
    res = {k: ctx.empty(3, n) for k in keys3}
    res.update({k: ctx.empty(n) for k in keys1})

    def both(q, fn, bounce):
        ms_emit = timed(fn, args.repeats, args.warmup)
        cnt = q.counts()
        hc, hP, hN, E, hits = plane_hits(q.probes)
        rnd = lambda k: torch.rand(3, max(cnt[k], 1), device=dev)
        planes = [rnd("sheen_shadow"), rnd("specular_shadow"), rnd("sheen_glossy"), rnd("specular_glossy")]
        kw = dict(diffuse_visibility=rnd("diffuse_shadow")) if bounce else {}
        ms_res = timed(lambda: q.resolve(*planes, hc, hP, hN, E, out=res, counts=cnt, **kw), args.repeats, args.warmup)
        del planes, kw, hc, hP, hN, E
        return dict(cnt, probes=q.probes.count, probe_hits=hits), round(ms_emit, 4), round(ms_res, 4)

    node_emit = lambda: T.skin_node_rays(sk, P, lights, spp_n, seed, queues=nq)
    emit = lambda: T.skin_bounce_rays(sk, P, lights, spp_n, seed, state, depths, queues=bq)
    _, ne0, nr0 = both(nq, node_emit, False)
    cnt, be, br = both(bq, emit, True)
    ncnt, ne1, nr1 = both(nq, node_emit, False)
    rec["lights"], rec["state"] = nl, args.state
    rec[args.closure] = {
        "rays": cnt, "node_rays": ncnt, "emit_ms": be, "resolve_ms": br, "node_emit_ms": [ne0, ne1], "node_resolve_ms": [nr0, nr1],
        "emit_over_node": round(be / min(ne0, ne1), 4), "resolve_over_node": round(br / min(nr0, nr1), 4),
    }


def bench_skin_node(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """the whole rlSkin node on the plane z = 0: emit, the one-launch resolve, the stand-alone resolves that exist, the analytic call"""
    import torch
    import rlshaders_amd as R
    from rlshaders_amd import trace as T
    nl = args.lights
    sk, P, lights, Ns, Tg, p, dist, mult = skin_batch(args, ctx, n, seed)
    scene = R.make_scene("plane", light_dir=(0, 0, 1), light_color=(1.0, 1.0, 1.0))
    keys3, keys1 = ("sheen", "specular", "sss", "out"), ("sheenFresnel", "specularFresnel", "sssWeight")
    aov = {k: ctx.empty(3, n) for k in keys3}
    aov.update({k: ctx.empty(n) for k in keys1})
    ms_int = timed(lambda: sk.integrate(P, scene, spp_n, seed, env=(0.7, 0.8, 0.9), out=aov, lights=lights), args.repeats, args.warmup)
    nq = T.SkinNodeQueues(ctx, n, nl, spp_n, share_scratch=True)
    ms_emit = timed(lambda: T.skin_node_rays(sk, P, lights, spp_n, seed, queues=nq), args.repeats, args.warmup)
    cnt = nq.counts()
    hc, hP, hN, E, hits = plane_hits(nq.probes)
    rnd = lambda k: torch.rand(3, max(cnt[k], 1), device=ctx.torch_device)
    planes = [rnd("sheen_shadow"), rnd("specular_shadow"), rnd("sheen_glossy"), rnd("specular_glossy")]
    res = {k: ctx.empty(3, n) for k in keys3}
    res.update({k: ctx.empty(n) for k in keys1})
    ms_res = timed(lambda: nq.resolve(*planes, hc, hP, hN, E, out=res, counts=cnt), args.repeats, args.warmup)
    # the existing stand-alone resolves that fit: one glossy resolve per lobe, the scatter resolve
    ss = R.SssSampler(ctx, Ns, Tg, p["sss_color"], dist, multiplier=mult)
    nq.probes.sampler, nq.probes.P = ss, P
    sums = [ctx.empty(3, n) for _ in range(3)]
    parts = [lambda: nq.sheen_glossy.resolve(planes[2], out=sums[0], count=cnt["sheen_glossy"]),
             lambda: nq.specular_glossy.resolve(planes[3], out=sums[1], count=cnt["specular_glossy"]),
             lambda: nq.probes.resolve(hc, hP, hN, E, out=sums[2])]
    ms_parts = [timed(f, args.repeats, args.warmup) for f in parts]
    ms_sep = timed(lambda: [f() for f in parts], args.repeats, args.warmup)
    rec["lights"] = nl
    rec[args.closure] = {
        "rays": dict(cnt, probes=nq.probes.count), "hits_per_probe": round(hits / max(nq.probes.count, 1), 4),
        "analytic_ms": round(ms_int, 4), "emit_ms": round(ms_emit, 4), "node_resolve_ms": round(ms_res, 4),
        "separate_partial_ms": round(ms_sep, 4),
        "separate_partial_ms_each": dict(zip(("sheen_glossy", "specular_glossy", "scatter"), [round(m, 4) for m in ms_parts])),
        "separate_partial_lacks": "the two lobes' light-loop sums and the composition: no stand-alone kernels exist for them",
        "emit_over_analytic": round(ms_emit / ms_int, 4),
        "emit_plus_resolve_over_analytic": round((ms_emit + ms_res) / ms_int, 4),
    }


def bench_shadow_fold(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """the fold of the hits' opacities into the shadow rays' visibility, direct and indexed (module docstring)"""
    import torch
    from rlshaders_amd import trace as T
    dev, max_hits, table_count = ctx.torch_device, 4, 4096
    g = torch.Generator(device=dev).manual_seed(seed)
    count = torch.randint(0, max_hits + 1, (n,), generator=g, device=dev).to(torch.uint8)
    hits = int(count.sum(dtype=torch.int64).item())
    out = ctx.empty(3, n)
    rec.update({"rays": n, "max_hits": max_hits, "hits": hits, "hits_per_ray": round(hits / n, 4)})
    for form in ("direct", "indexed"):
        if form == "direct":
            opacity, index = torch.rand(3, max_hits, n, generator=g, device=dev), None
            bytes_ = n * (1 + 12) + hits * 12
        else:
            opacity = torch.rand(3, table_count, generator=g, device=dev)
            index = torch.randint(0, table_count, (max_hits, n), generator=g, device=dev, dtype=torch.int32)
            bytes_ = n * (1 + 12) + hits * (4 + 12)
        h = T.ShadowHits(count, opacity, max_hits, index=index)
        ms = timed(lambda: T.shadow_visibility(ctx, n, h, out=out), args.repeats, args.warmup)
        rec[form] = {"ms": round(ms, 4), "bytes": bytes_, "rays_per_s": round(n / (ms * 1e-3), 1), "tb_per_s": rate(bytes_, ms),
                     "frac_of_8tbps": round(rate(bytes_, ms) / HBM_TBPS, 4)}
        if index is not None:
            rec[form]["table_count"] = table_count
        del h, opacity, index
        torch.cuda.empty_cache()


def bench_shadow_walk(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """the shadow walk over bench_shadow_fold's indexed rays and surfaces, beside the fold of the same hits (module docstring)"""
    import torch
    from rlshaders_amd import build, shadow_walk as W, trace as T
    build.build_shadow_walk_library()
    repeats, warmup = max(args.repeats, 9), max(args.warmup, 3)
    dev, max_hits, table_count = ctx.torch_device, 4, 4096
    g = torch.Generator(device=dev).manual_seed(seed)
    count = torch.randint(0, max_hits + 1, (n,), generator=g, device=dev).to(torch.uint8)
    table = torch.rand(3, table_count, generator=g, device=dev)
    index = torch.randint(0, table_count, (max_hits, n), generator=g, device=dev, dtype=torch.int32)
    d = torch.randn(3, n, generator=g, device=dev)
    d = (d / d.norm(dim=0)).contiguous()
    O = torch.rand(3, n, generator=g, device=dev)
    q = W.RawQueue(d, torch.full((n,), 1e3, device=dev), torch.arange(n, dtype=torch.int32, device=dev))
    w = W.ShadowWalk(ctx, q, O, max_steps=2 * max_hits)
    fold = ctx.empty(3, n)
    hits = T.ShadowHits(count, table, max_hits, index=index)
    fold_ms = timed_spread(lambda: T.shadow_visibility(ctx, n, hits, out=fold), repeats, warmup)

    def found(r, m, k):
        """the renderer: listed ray j meets its k-th surface one unit on, while it has one"""
        j = r.ray[:m].long()
        hit = count[j] > k
        ix = index[min(k, max_hits - 1)][j].contiguous()
        P = (r.origin[:, :m] + r.dir[:, :m]).contiguous()
        return W.Found(hit.to(torch.uint8), torch.ones(m, device=dev), P, table, index=ix), int(hit.sum().item())

    steps, begin_ms = [], []
    for run in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        w.begin()
        b.record()
        b.synchronize()
        begin_ms.append(a.elapsed_time(b))
        for k in range(w.max_steps):
            m = w.active
            if m == 0:
                break
            f, nhit = found(w.rays, m, k)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            w.step(f, bound=m)
            b.record()
            b.synchronize()
            if k == len(steps):
                steps.append({"active": m, "hits": nhit, "ms": []})
            if run >= warmup:
                steps[k]["ms"].append(a.elapsed_time(b))
            if run == warmup:
                steps[k]["survivors"] = w.active
    same = bool(torch.equal(w.visibility.view(torch.int32), fold.view(torch.int32)))
    total_ms = total_bytes = 0.0
    for st in steps:
        ms = sorted(st.pop("ms"))
        bytes_ = st["active"] * 34 + st["hits"] * 32 + st["survivors"] * 61
        st.update(ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), bytes=bytes_,
                  bytes_per_active_ray=round(bytes_ / st["active"], 1), tb_per_s=rate(bytes_, ms[len(ms) // 2]))
        total_ms += st["ms"]
        total_bytes += bytes_
    begin_ms = sorted(begin_ms[warmup:])
    bm = begin_ms[len(begin_ms) // 2]
    nhits = int(count.sum(dtype=torch.int64).item())
    fold_bytes = n * (1 + 12) + nhits * (4 + 12)
    rec["shadow-walk"] = {
        "rays": n, "max_hits": max_hits, "table_count": table_count, "hits": nhits, "repeats": repeats, "warmup": warmup,
        "begin_ms": round(bm, 4), "begin_min_ms": round(begin_ms[0], 4), "begin_max_ms": round(begin_ms[-1], 4),
        # begin: per ray maxdist read, T and state written, state read again: 20; per listed ray point, O, dir, maxdist read and
        # ray, steps, origin, dir, maxdist written: 65
        "begin_tb_per_s": rate(n * 20 + steps[0]["active"] * 65, bm),
        "steps": steps, "steps_ms": round(total_ms, 4), "steps_bytes": int(total_bytes), "steps_tb_per_s": rate(total_bytes, total_ms),
        "walk_ms": round(bm + total_ms, 4), "fold_ms": fold_ms["ms"], "fold_min_ms": fold_ms["min_ms"], "fold_max_ms": fold_ms["max_ms"],
        "fold_tb_per_s": rate(fold_bytes, fold_ms["ms"]), "walk_over_fold": round((bm + total_ms) / fold_ms["ms"], 2),
        "walk_equals_fold": same,
    }


def icosphere(level: int, radius: float = 1.0, center=(0.0, 0.0, 0.0)):
    """a subdivided icosahedron, 20 * 4^level triangles -> (V float32 [nv, 3], tri uint32 [nt, 3], unit normals [nv, 3])"""
    import numpy as np
    g = (1 + 5 ** 0.5) / 2
    V = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
                  (-g, 0, -1), (-g, 0, 1)], np.float64)
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    T = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)], np.int64)
    for _ in range(level):
        e = np.sort(np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]]), axis=1)
        edges, inv = np.unique(e, axis=0, return_inverse=True)
        mid = V[edges[:, 0]] + V[edges[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = (len(V) + inv.reshape(-1)).reshape(3, -1)              # the midpoints of ab, bc, ca of every triangle
        V = np.concatenate([V, mid])
        a, b, c = T[:, 0], T[:, 1], T[:, 2]
        T = np.concatenate([np.stack(t, axis=1) for t in ((a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2]))])
    return (V * radius + np.asarray(center, np.float64)).astype(np.float32), T.astype(np.uint32), V.astype(np.float32)


def bench_nearest(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """rls_nearest_hits on an icosphere of 81 920 triangles: a camera grid's rays (coherent), then cosine-distributed rays from the
    points they hit with `last` set (incoherent), each beside a copy_ of the bytes of its ray and found planes"""
    import numpy as np
    import torch
    from rlshaders_amd import nearest
    nearest.load()
    repeats, warmup = max(args.repeats, 9), max(args.warmup, 3)
    dev = ctx.torch_device
    V, tri, normals = icosphere(args.level)
    scene = nearest.Scene(ctx, V, tri, normals=normals)
    side = int(round(n ** 0.5))
    n = side * side
    g = torch.Generator(device=dev).manual_seed(seed)
    # a pinhole at (0, 0, -3) looking at the sphere through a side x side grid of 1.3 x 1.3 at z = -2: about half the rays hit
    u = (torch.arange(side, device=dev, dtype=torch.float32) + 0.5) / side * 1.3 - 0.65
    d = torch.stack([u.repeat(side), u.repeat_interleave(side), torch.ones(n, device=dev)]).contiguous()
    o = torch.tensor([0.0, 0.0, -3.0], device=dev)[:, None].expand(3, n).contiguous()
    planes = ("P", "N", "Ns", "surface", "prim")
    found = nearest.Found(ctx, n, planes=planes)
    rays = nearest.Rays(o, d)

    def with_copy(fn, bytes_):
        r = timed_spread(fn, repeats, warmup)
        a, b = (torch.empty(max(bytes_ // 2, 1), dtype=torch.uint8, device=dev) for _ in range(2))
        c = timed_spread(lambda: b.copy_(a), repeats, warmup)
        del a, b
        r.update({"bytes": bytes_, "copy_ms": c["ms"], "copy_min_ms": c["min_ms"], "copy_max_ms": c["max_ms"],
                  "over_copy": round(r["ms"] / c["ms"], 2)})
        return r

    def account(r, hits, ray_bytes, hit_bytes, sample):
        # read per ray: origin, dir (24) [+ last 4]; written per ray: hit (1); per hit: t, P, N, Ns, surface, prim (48) [+ last 4]
        bytes_ = n * ray_bytes + n + hits * hit_bytes
        out = with_copy(r, bytes_)
        out.update({"rays": n, "hits": hits, "mrays_per_s": round(n / out["ms"] / 1e3, 1), "bytes_per_ray": round(bytes_ / n, 1)})
        # the nodes and triangles a ray visits: the kernel's traversal source run on the host over the same tree, on every
        # 4096 rays of the stream: one out of every run of n / 4096, at a place in the run that moves with the run (a fixed
        # stride would pick two columns of the camera's grid)
        o_, d_, skip_ = sample
        run = max(n // 4096, 1)
        k = torch.arange(min(n, 4096), device=dev)
        pick = k * run + (k * 37) % run
        st = nearest.host_stats(V, tri, o_[:, pick].cpu().numpy(), d_[:, pick].cpu().numpy(),
                                skip=None if skip_ is None else skip_[pick].cpu().numpy().view(np.uint32), leaf_size=scene.leaf_size)
        out.update({"sample_rays": st["rays"], "sample_hits": st["hits"], "nodes_per_ray": round(st["nodes"] / st["rays"], 1),
                    "triangles_per_ray": round(st["triangles"] / st["rays"], 1), "max_stack": st["max_stack"]})
        return out

    scene.hits(rays, found=found)
    hits = int(found.hit.sum(dtype=torch.int64).item())
    rec["scene"] = {"triangles": scene.nt, "nodes": scene.nodes, "depth": scene.depth, "leaf_size": scene.leaf_size,
                    "device_bytes": scene.device_bytes}
    rec["coherent"] = account(lambda: scene.hits(rays, found=found), hits, 24, 48, (o, d, None))
    # incoherent: from every hit point (the misses from points of the sphere chosen at random) a cosine-distributed direction
    # about the inward normal, the triangle the point lies on skipped through `last`
    hit = found.hit.bool()
    Pn = torch.randn(3, n, generator=g, device=dev)
    Pn = Pn / Pn.norm(dim=0)
    O2 = torch.where(hit[None, :], found.P, Pn).contiguous()
    inward = -(O2 / O2.norm(dim=0))
    w = torch.randn(3, n, generator=g, device=dev)
    w = w / w.norm(dim=0)
    d2 = (inward + 0.999 * w).contiguous()                          # a unit vector about the normal's tip: cosine-distributed
    last0 = torch.where(hit, found.prim, torch.full_like(found.prim, -1)).contiguous()
    last = last0.clone()
    rays2 = nearest.Rays(O2, d2)
    found2 = nearest.Found(ctx, n, planes=planes)

    def incoherent():
        last.copy_(last0)
        scene.hits(rays2, last=last, found=found2)

    incoherent()
    hits2 = int(found2.hit.sum(dtype=torch.int64).item())
    reset = timed_spread(lambda: last.copy_(last0), repeats, warmup)
    rec["incoherent"] = account(incoherent, hits2, 28, 52, (O2, d2, last0))
    rec["incoherent"]["last_reset_ms"] = reset["ms"]               # inside the timed call: the copy that sets `last` again
    scene.close()


def bench_nearest_refit(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """rls_nearest_refit_update against nearest.Scene(...) creation on the same vertices (a host build and an upload), at the
    81 920-triangle icosphere and at a 2^20-triangle grid, with the single-workgroup launch of the tree's top (the default) and
    with one launch per level (RLS_NEAREST_REFIT_FOLD=0); then --closure nearest's two streams on the refit tree and on a rebuilt
    tree, for the icosphere twisted about y by 0.5 and by 2 radians end to end"""
    import os
    import time

    import numpy as np
    import torch
    from rlshaders_amd import nearest, nearest_refit
    nearest_refit.load()
    repeats, warmup = max(args.repeats, 9), max(args.warmup, 3)
    dev = ctx.torch_device

    def twisted(V, radians):
        V = np.asarray(V, np.float64)
        a = radians * (V[:, 1] - V[:, 1].min()) / np.ptp(V[:, 1])
        c, s = np.cos(a), np.sin(a)
        return np.stack([c * V[:, 0] + s * V[:, 2], V[:, 1], -s * V[:, 0] + c * V[:, 2]], 1).astype(np.float32)

    def grid(side):
        g = np.linspace(-1.0, 1.0, side + 1)
        x, y = np.meshgrid(g, g, indexing="xy")
        V = np.stack([x, y, 0.1 * np.sin(3.0 * x) * np.cos(2.0 * y)], axis=-1).reshape(-1, 3).astype(np.float32)
        j, i = np.divmod(np.arange(side * side, dtype=np.int64), side)
        a = j * (side + 1) + i
        return V, np.stack([a, a + 1, a + side + 2, a, a + side + 2, a + side + 1], axis=1).reshape(-1, 3).astype(np.uint32)

    def make_refit(scene, fold):
        old = os.environ.get("RLS_NEAREST_REFIT_FOLD")
        os.environ["RLS_NEAREST_REFIT_FOLD"] = "1" if fold else "0"      # read when the refit is made
        try:
            return nearest_refit.Refit(scene)
        finally:
            if old is None:
                del os.environ["RLS_NEAREST_REFIT_FOLD"]
            else:
                os.environ["RLS_NEAREST_REFIT_FOLD"] = old

    V6, tri6, _ = icosphere(args.level)
    Vg, trig = grid(724)                                             # 2 * 724^2 = 1 048 352 triangles
    rec["update"] = {}
    for name, V, tri in (("icosphere", V6, tri6), ("grid", Vg, trig)):
        moved = twisted(V, 0.5)
        scene = nearest.Scene(ctx, V, tri)
        dv = torch.from_numpy(moved).to(dev)
        out = {"triangles": scene.nt, "nodes": scene.nodes, "depth": scene.depth}
        # the two versions alternate, twice: the spread between the passes is beside the difference
        for fold in (True, False, True, False):
            r = make_refit(scene, fold)
            t = timed_spread(lambda: r.update(dv), repeats, warmup)
            key = "update_folded" if fold else "update_per_level"
            out.setdefault(key, []).append(t)
            r.close()
        # the bytes an update moves at least: a record read (prim) and written, 36 bytes of vertices, 12 of indices a triangle;
        # a node read and its box written
        bytes_ = scene.nt * (4 + 48 + 36 + 12) + scene.nodes * (32 + 24)
        out["bytes"] = bytes_
        out["update_tb_per_s"] = rate(bytes_, out["update_folded"][0]["ms"])
        create = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s2 = nearest.Scene(ctx, moved, tri)
            torch.cuda.synchronize()
            create.append((time.perf_counter() - t0) * 1e3)
            s2.close()
        create.sort()
        out["create_ms"] = {"ms": round(create[1], 2), "min_ms": round(create[0], 2), "max_ms": round(create[2], 2)}
        out["create_over_update"] = round(create[1] / out["update_folded"][0]["ms"], 1)
        rec["update"][name] = out
        scene.close()

    # query cost: the drift of a refit tree against a rebuilt one
    side = int(round(n ** 0.5))
    n = side * side
    g = torch.Generator(device=dev).manual_seed(seed)
    u = (torch.arange(side, device=dev, dtype=torch.float32) + 0.5) / side * 1.3 - 0.65
    d = torch.stack([u.repeat(side), u.repeat_interleave(side), torch.ones(n, device=dev)]).contiguous()
    o = torch.tensor([0.0, 0.0, -3.0], device=dev)[:, None].expand(3, n).contiguous()
    planes = ("P", "N", "Ns", "surface", "prim")
    rec["queries"] = {"rays": n}
    for radians in (0.5, 2.0):
        moved = twisted(V6, radians)
        kept = nearest.Scene(ctx, V6, tri6)
        r = nearest_refit.Refit(kept)
        r.update(torch.from_numpy(moved).to(dev))
        rebuilt = nearest.Scene(ctx, moved, tri6)
        out = {}
        streams = None
        for name, scene in (("refit", kept), ("rebuilt", rebuilt)):
            found = nearest.Found(ctx, n, planes=planes)
            rays = nearest.Rays(o, d)
            scene.hits(rays, found=found)
            if streams is None:                                      # the incoherent stream: from the hits, as --closure nearest
                hit = found.hit.bool()
                Pn = torch.randn(3, n, generator=g, device=dev)
                Pn = Pn / Pn.norm(dim=0)
                O2 = torch.where(hit[None, :], found.P, Pn).contiguous()
                w = torch.randn(3, n, generator=g, device=dev)
                d2 = (-(O2 / O2.norm(dim=0)) + 0.999 * w / w.norm(dim=0)).contiguous()
                last0 = torch.where(hit, found.prim, torch.full_like(found.prim, -1)).contiguous()
                streams = (O2, d2, last0, found.hit.clone(), found.t.clone())
            O2, d2, last0, hit0, t0 = streams
            same = bool(torch.equal(found.hit, hit0) and torch.equal(found.t[hit0.bool()].view(torch.int32), t0[hit0.bool()].view(torch.int32)))
            last = last0.clone()
            rays2, found2 = nearest.Rays(O2, d2), nearest.Found(ctx, n, planes=planes)

            def incoherent():
                last.copy_(last0)
                scene.hits(rays2, last=last, found=found2)

            out[name] = {"coherent": timed_spread(lambda: scene.hits(rays, found=found), repeats, warmup),
                         "incoherent": timed_spread(incoherent, repeats, warmup), "hits": int(found.hit.sum(dtype=torch.int64).item()),
                         "same_as_refit": same}
        out["coherent_refit_over_rebuilt"] = round(out["refit"]["coherent"]["ms"] / out["rebuilt"]["coherent"]["ms"], 3)
        out["incoherent_refit_over_rebuilt"] = round(out["refit"]["incoherent"]["ms"] / out["rebuilt"]["incoherent"]["ms"], 3)
        rec["queries"][f"twist_{radians}"] = out
        r.close(), kept.close(), rebuilt.close()


def bench_nearest_rebuild(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """rls_nearest_rebuild_update beside rls_nearest_refit_update and nearest.Scene(...) creation on the same vertices, at the
    81 920-triangle icosphere and at a 2^20-triangle grid; then --closure nearest's two streams on the refit, the device-rebuilt
    and the host-rebuilt tree, for the icosphere twisted about y by 0.5 and by 2 radians end to end"""
    import time

    import numpy as np
    import torch
    from rlshaders_amd import nearest, nearest_rebuild, nearest_refit
    nearest_refit.load(), nearest_rebuild.load()
    repeats, warmup = max(args.repeats, 9), max(args.warmup, 3)
    dev = ctx.torch_device

    def twisted(V, radians):
        V = np.asarray(V, np.float64)
        a = radians * (V[:, 1] - V[:, 1].min()) / np.ptp(V[:, 1])
        c, s = np.cos(a), np.sin(a)
        return np.stack([c * V[:, 0] + s * V[:, 2], V[:, 1], -s * V[:, 0] + c * V[:, 2]], 1).astype(np.float32)

    def grid(side):
        g = np.linspace(-1.0, 1.0, side + 1)
        x, y = np.meshgrid(g, g, indexing="xy")
        V = np.stack([x, y, 0.1 * np.sin(3.0 * x) * np.cos(2.0 * y)], axis=-1).reshape(-1, 3).astype(np.float32)
        j, i = np.divmod(np.arange(side * side, dtype=np.int64), side)
        a = j * (side + 1) + i
        return V, np.stack([a, a + 1, a + side + 2, a, a + side + 2, a + side + 1], axis=1).reshape(-1, 3).astype(np.uint32)

    V6, tri6, _ = icosphere(args.level)
    Vg, trig = grid(724)                                             # 2 * 724^2 = 1 048 352 triangles
    rec["update"] = {}
    for name, V, tri in (("icosphere", V6, tri6), ("grid", Vg, trig)):
        moved = twisted(V, 0.5)
        scene = nearest.Scene(ctx, V, tri)
        dv = torch.from_numpy(moved).to(dev)
        rb, rf = nearest_rebuild.Rebuild(scene), nearest_refit.Refit(scene)
        levels = rb.levels
        out = {"triangles": scene.nt, "nodes": scene.nodes, "depth": scene.depth, "device_bytes": rb.device_bytes,
               "device_bytes_per_triangle": round(rb.device_bytes / max(scene.nt, 1), 1),
               # init; a pass of the sort: count, three of the scan, scatter; a round: mark, three of the scan, partition;
               # the leaves; the records; a level of boxes each
               "launches": 1 + (8 * 5 + (levels - 1) * 5 if levels > 1 else 0) + 2 + levels}
        # the two updates alternate, twice: the spread between the passes is beside the difference
        for _ in range(2):
            out.setdefault("rebuild", []).append(timed_spread(lambda: rb.update(dv), repeats, warmup))
            out.setdefault("refit", []).append(timed_spread(lambda: rf.update(dv), repeats, warmup))
        create = []
        for k in range(repeats + warmup):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s2 = nearest.Scene(ctx, moved, tri)
            torch.cuda.synchronize()
            if k >= warmup:
                create.append((time.perf_counter() - t0) * 1e3)
            s2.close()
        create.sort()
        out["create_ms"] = {"ms": round(create[len(create) // 2], 2), "min_ms": round(create[0], 2), "max_ms": round(create[-1], 2)}
        out["create_over_rebuild"] = round(out["create_ms"]["ms"] / out["rebuild"][0]["ms"], 1)
        out["rebuild_over_refit"] = round(out["rebuild"][0]["ms"] / out["refit"][0]["ms"], 1)
        rec["update"][name] = out
        rb.close(), rf.close(), scene.close()

    # query cost: the refit tree, the device-rebuilt tree, the host-rebuilt tree
    side = int(round(n ** 0.5))
    n = side * side
    g = torch.Generator(device=dev).manual_seed(seed)
    u = (torch.arange(side, device=dev, dtype=torch.float32) + 0.5) / side * 1.3 - 0.65
    d = torch.stack([u.repeat(side), u.repeat_interleave(side), torch.ones(n, device=dev)]).contiguous()
    o = torch.tensor([0.0, 0.0, -3.0], device=dev)[:, None].expand(3, n).contiguous()
    planes = ("P", "N", "Ns", "surface", "prim")
    rec["queries"] = {"rays": n}
    for radians in (0.5, 2.0):
        moved = twisted(V6, radians)
        dv = torch.from_numpy(moved).to(dev)
        kept, turned = nearest.Scene(ctx, V6, tri6), nearest.Scene(ctx, V6, tri6)
        rf, rb = nearest_refit.Refit(kept), nearest_rebuild.Rebuild(turned)
        rf.update(dv)
        rb.update(dv)
        fresh = nearest.Scene(ctx, moved, tri6)
        out, streams, results = {}, None, {}
        for name, scene in (("refit", kept), ("device_rebuilt", turned), ("host_rebuilt", fresh)):
            found = nearest.Found(ctx, n, planes=planes, alloc=lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev))
            rays = nearest.Rays(o, d)
            scene.hits(rays, found=found)
            if streams is None:                                      # the incoherent stream: from the hits, as --closure nearest
                hit = found.hit.bool()
                Pn = torch.randn(3, n, generator=g, device=dev)
                Pn = Pn / Pn.norm(dim=0)
                O2 = torch.where(hit[None, :], found.P, Pn).contiguous()
                w = torch.randn(3, n, generator=g, device=dev)
                d2 = (-(O2 / O2.norm(dim=0)) + 0.999 * w / w.norm(dim=0)).contiguous()
                last0 = torch.where(hit, found.prim, torch.full_like(found.prim, -1)).contiguous()
                streams = (O2, d2, last0)
            O2, d2, last0 = streams
            last = last0.clone()
            rays2 = nearest.Rays(O2, d2)
            found2 = nearest.Found(ctx, n, planes=planes, alloc=lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev))

            def incoherent():
                last.copy_(last0)
                scene.hits(rays2, last=last, found=found2)

            out[name] = {"coherent": timed_spread(lambda: scene.hits(rays, found=found), repeats, warmup),
                         "incoherent": timed_spread(incoherent, repeats, warmup), "hits": int(found.hit.sum(dtype=torch.int64).item())}
            results[name] = [getattr(f, k).clone() for f in (found, found2) for k in ("hit", "t") + planes] + [last.clone()]
        out["device_rebuilt"]["same_as_host_rebuilt"] = all(
            torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(results["device_rebuilt"], results["host_rebuilt"]))
        for stream in ("coherent", "incoherent"):
            out[f"{stream}_refit_over_device_rebuilt"] = round(out["refit"][stream]["ms"] / out["device_rebuilt"][stream]["ms"], 3)
            out[f"{stream}_device_over_host_rebuilt"] = round(out["device_rebuilt"][stream]["ms"] / out["host_rebuilt"][stream]["ms"], 3)
        rec["queries"][f"twist_{radians}"] = out
        rf.close(), rb.close(), kept.close(), turned.close(), fresh.close()


def bench_shadow_walk_nearest(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """a whole shadow walk with its queries inside the events: n rays from the unit cube through three nested tinted icospheres
    (3 x 5 120 triangles, radii 2, 3, 4), every step = rls_nearest_walk_hits + rls_shadow_walk_step"""
    import numpy as np
    import torch
    from rlshaders_amd import nearest, shadow_walk as W
    W.load(), nearest.load()
    repeats, warmup = max(args.repeats, 9), max(args.warmup, 3)
    dev = ctx.torch_device
    Vs, Ts, Ss = [], [], []
    for k, radius in enumerate((2.0, 3.0, 4.0)):
        V, tri, _ = icosphere(4, radius, (0.5, 0.5, 0.5))
        Ts.append(tri + sum(len(v) for v in Vs))
        Vs.append(V)
        Ss.append(np.full(len(tri), k, np.uint32))
    scene = nearest.Scene(ctx, np.concatenate(Vs), np.concatenate(Ts), surface=np.concatenate(Ss))
    g = torch.Generator(device=dev).manual_seed(seed)
    table = (torch.rand(3, 3, generator=g, device=dev) * 0.9).contiguous()
    d = torch.randn(3, n, generator=g, device=dev)
    d = (d / d.norm(dim=0)).contiguous()
    O = torch.rand(3, n, generator=g, device=dev)
    q = W.RawQueue(d, torch.full((n,), 1e3, device=dev), torch.arange(n, dtype=torch.int32, device=dev))
    w = W.ShadowWalk(ctx, q, O, max_steps=8)
    found = nearest.Found(ctx, n, planes=("P", "surface"))
    last = torch.empty(n, dtype=torch.int32, device=dev)
    steps, begin_ms = [], []
    for run in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        w.begin()
        last.fill_(-1)
        b.record()
        b.synchronize()
        begin_ms.append(a.elapsed_time(b))
        for k in range(w.max_steps):
            m = w.active
            if m == 0:
                break
            a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            a.record()
            scene.hits(w.rays, active=m, last=last, found=found)
            b.record()
            w.step(found.shadow_found(table), bound=m)
            c.record()
            c.synchronize()
            if k == len(steps):
                steps.append({"active": m, "hits": int(found.hit[:m].sum(dtype=torch.int64).item()), "trace_ms": [], "step_ms": []})
            if run >= warmup:
                steps[k]["trace_ms"].append(a.elapsed_time(b))
                steps[k]["step_ms"].append(b.elapsed_time(c))
    med = lambda v: round(sorted(v)[len(v) // 2], 4)
    for st in steps:
        st["trace_ms"], st["step_ms"] = med(st["trace_ms"]), med(st["step_ms"])
    bm = med(begin_ms[warmup:])
    trace_ms, step_ms = sum(st["trace_ms"] for st in steps), sum(st["step_ms"] for st in steps)
    rec["shadow-walk"] = {"tracer": "nearest", "rays": n, "triangles": scene.nt, "nodes": scene.nodes, "repeats": repeats, "warmup": warmup,
                          "begin_ms": bm, "steps": steps, "trace_ms": round(trace_ms, 4), "step_ms": round(step_ms, 4),
                          "walk_ms": round(bm + trace_ms + step_ms, 4), "walk_only_ms": round(bm + step_ms, 4),
                          "mean_visibility": float(w.visibility.mean().item())}
    scene.close()


def bench_nearest_group(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """a grid of instances of one icosphere under a group, beside the flat scene of the same geometry (module docstring)"""
    import numpy as np
    import torch
    from rlshaders_amd import build, codeid, nearest, nearest_group, nearest_rebuild
    nearest_group.load()
    repeats, warmup = max(args.repeats, 9), max(args.warmup, 3)
    dev = ctx.torch_device
    V, tri, normals = icosphere(args.level)
    nv, nt, count = V.shape[0], tri.shape[0], args.instances
    side3 = int(np.ceil(count ** (1.0 / 3.0)))
    rng = np.random.default_rng(seed)
    B = np.zeros((count, 3, 4))
    for j in range(count):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        B[j, :, :3] = q if np.linalg.det(q) > 0 else -q
        B[j, :, 3] = 2.5 * (np.array([j % side3, (j // side3) % side3, j // (side3 * side3)]) - (side3 - 1) / 2.0)
    half = 1.25 * side3                                               # the grid's half-width
    scene = nearest.Scene(ctx, V, tri, normals=normals)
    instances = [nearest_group.Instance(scene, B[j], surface_base=j) for j in range(count)]
    group = nearest_group.Group(ctx, instances)
    rec["group"] = dict(group.info(), triangles_a_scene=nt, scene_device_bytes=scene.device_bytes,
                        library_id=codeid.DeviceCode(build.NEAREST_GROUP_LIB).library_id)
    flat = None
    if count * nt <= nearest.RLS_NEAREST_MAX_TRIANGLES:
        Vf = np.concatenate([(V.astype(np.float64) @ B[j, :, :3].T + B[j, :, 3]).astype(np.float32) for j in range(count)])
        Tf = np.concatenate([tri.astype(np.int64) + j * nv for j in range(count)])
        flat = nearest.Scene(ctx, Vf, Tf, normals=np.concatenate([normals @ B[j, :, :3].T.astype(np.float32) for j in range(count)]))
        rec["flat"] = {"triangles": flat.nt, "depth": flat.depth, "device_bytes": flat.device_bytes}
    side = int(round(n ** 0.5))
    n = side * side
    g = torch.Generator(device=dev).manual_seed(seed)
    planes = ("P", "N", "Ns", "surface", "prim")
    u = (torch.arange(side, device=dev, dtype=torch.float32) + 0.5) / side * 2.6 - 1.3

    def camera(scale):
        d = torch.stack([u.repeat(side) * scale, u.repeat_interleave(side) * scale, torch.full((n,), 2.0 * scale, device=dev)]).contiguous()
        o = torch.tensor([0.0, 0.0, -3.0 * scale], device=dev)[:, None].expand(3, n).contiguous()
        return nearest.Rays(o, d)

    def run(fn, found):
        fn()
        r = timed_spread(fn, repeats, warmup)
        r.update({"rays": n, "hits": int(found.hit.sum(dtype=torch.int64).item()), "mrays_per_s": round(n / r["ms"] / 1e3, 1)})
        return r

    rays = camera(half)
    fg = nearest_group.Found(ctx, n, planes=planes + ("instance",))
    rec["coherent"] = {"group": run(lambda: group.hits(rays, found=fg), fg)}
    ff = nearest.Found(ctx, n, planes=planes)
    if flat is not None:
        rec["coherent"]["flat"] = run(lambda: flat.hits(rays, found=ff), ff)
        rec["coherent"]["same_hit_flag"] = round(float((fg.hit == ff.hit).float().mean().item()), 6)
        rec["coherent"]["group_over_flat"] = round(rec["coherent"]["group"]["ms"] / rec["coherent"]["flat"]["ms"], 2)
    # incoherent: from every hit point (the misses from points of the grid's box) a uniformly distributed direction, the
    # (instance, triangle) the point lies on skipped
    hit = fg.hit.bool()
    O2 = torch.where(hit[None, :], fg.P, (torch.rand(3, n, generator=g, device=dev) * 2 - 1) * half).contiguous()
    w = torch.randn(3, n, generator=g, device=dev)
    d2 = (w / w.norm(dim=0)).contiguous()
    none = torch.full_like(fg.prim, -1)
    last0, inst0 = torch.where(hit, fg.prim, none).contiguous(), torch.where(hit, fg.instance, none).contiguous()
    flat0 = torch.where(hit, fg.instance * nt + fg.prim, none).contiguous()
    last, inst, rays2 = last0.clone(), inst0.clone(), nearest.Rays(O2, d2)
    fg2, ff2 = nearest_group.Found(ctx, n, planes=planes + ("instance",)), nearest.Found(ctx, n, planes=planes)

    def incoherent_group():
        last.copy_(last0)
        inst.copy_(inst0)
        group.hits(rays2, last=last, last_instance=inst, found=fg2)

    def incoherent_flat():
        last.copy_(flat0)
        flat.hits(rays2, last=last, found=ff2)

    rec["incoherent"] = {"group": run(incoherent_group, fg2)}
    if flat is not None:
        rec["incoherent"]["flat"] = run(incoherent_flat, ff2)
        rec["incoherent"]["same_hit_flag"] = round(float((fg2.hit == ff2.hit).float().mean().item()), 6)
        rec["incoherent"]["group_over_flat"] = round(rec["incoherent"]["group"]["ms"] / rec["incoherent"]["flat"]["ms"], 2)
    # one instance alone: the second level's cost a ray
    one = nearest_group.Group(ctx, [nearest_group.Instance(scene, np.eye(4)[:3])])
    rays1 = camera(0.5)
    rec["alone"] = {"group": run(lambda: one.hits(rays1, found=fg), fg), "scene": run(lambda: scene.hits(rays1, found=ff), ff)}
    rec["alone"]["group_over_scene"] = round(rec["alone"]["group"]["ms"] / rec["alone"]["scene"]["ms"], 2)
    one.close()
    # the update: two matrix planes against baking + a rebuild of the flat scene
    A_, B_ = (torch.from_numpy(np.stack([getattr(i, k).reshape(12) for i in instances])).to(dev) for k in ("to_object", "to_world"))
    rec["update"] = {"group": timed_spread(lambda: group.update(A_, B_), repeats, warmup), "launches": 1 + group.info()["top_depth"]}
    if flat is not None:
        rebuild = nearest_rebuild.Rebuild(flat)
        Vd, L, t = torch.from_numpy(V).to(dev), B_.view(count, 3, 4)[:, :, :3].contiguous(), B_.view(count, 3, 4)[:, :, 3].contiguous()
        out = torch.empty(count, nv, 3, device=dev)

        def bake_and_rebuild():
            torch.baddbmm(t[:, None, :], Vd[None].expand(count, nv, 3), L.transpose(1, 2), out=out)
            rebuild.update(out.view(-1, 3))

        rec["update"]["bake_and_rebuild_flat"] = timed_spread(bake_and_rebuild, repeats, warmup)
        rec["update"]["flat_over_group"] = round(rec["update"]["bake_and_rebuild_flat"]["ms"] / rec["update"]["group"]["ms"], 1)
        rebuild.close()
        flat.close()
    group.close()
    scene.close()


def bench_nearest_any(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """the any-hit query beside the nearest-hit query and beside the shadow walk it shortens (module docstring)"""
    import numpy as np
    import torch
    import rlshaders_amd as R
    from rlshaders_amd import build, codeid, nearest, nearest_any, shadow_walk, trace as T
    from rlshaders_amd.closures import make_light
    nearest_any.load(), shadow_walk.load()
    repeats, warmup = max(args.repeats, 9), max(args.warmup, 3)
    dev = ctx.torch_device
    rec["library_id"] = codeid.DeviceCode(build.NEAREST_ANY_LIB).library_id
    rec["nearest_library_id"] = codeid.DeviceCode(build.NEAREST_LIB).library_id
    # ---- (a) the two streams of --closure nearest with finite reaches
    V, tri, normals = icosphere(args.level)
    scene = nearest.Scene(ctx, V, tri, normals=normals)
    rec["scene"] = {"triangles": scene.nt, "nodes": scene.nodes, "depth": scene.depth, "leaf_size": scene.leaf_size}
    side = int(round(n ** 0.5))
    m = side * side
    g = torch.Generator(device=dev).manual_seed(seed)
    u = (torch.arange(side, device=dev, dtype=torch.float32) + 0.5) / side * 1.3 - 0.65
    d = torch.stack([u.repeat(side), u.repeat_interleave(side), torch.ones(m, device=dev)]).contiguous()
    o = torch.tensor([0.0, 0.0, -3.0], device=dev)[:, None].expand(3, m).contiguous()
    found = nearest.Found(ctx, m, planes=("P", "surface"))
    state, vis, reach = (torch.empty(m, dtype=torch.uint8, device=dev), torch.empty(3, m, device=dev), torch.empty(m, device=dev))

    def pair(rays, last0):
        last = None if last0 is None else last0.clone()

        def near():
            if last is not None:
                last.copy_(last0)                                    # rls_nearest_hits writes `last`; the any-hit query never does
            scene.hits(rays, last=last, found=found)

        def any_():
            nearest_any.hits(scene, rays, last=last0, state=state, visibility=vis, reach=reach)

        near(), any_()
        out = {"rays": m, "hits": int(found.hit.sum(dtype=torch.int64).item()), "blocked": int((state == 1).sum().item()),
               "nearest": timed_spread(near, repeats, warmup), "any": timed_spread(any_, repeats, warmup)}
        if last is not None:
            out["last_reset_ms"] = timed_spread(lambda: last.copy_(last0), repeats, warmup)["ms"]
        out["same_hit_flag"] = bool(torch.equal(found.hit, state))
        out["any_over_nearest"] = round(out["any"]["ms"] / out["nearest"]["ms"], 3)
        return out

    rec["streams"] = {"coherent": pair(nearest.Rays(o, d, maxdist=torch.full((m,), 3.0, device=dev)), None)}
    first = nearest.Found(ctx, m, planes=("P", "prim"))
    scene.hits(nearest.Rays(o, d), found=first)
    hit = first.hit.bool()
    Pn = torch.randn(3, m, generator=g, device=dev)
    Pn = Pn / Pn.norm(dim=0)
    O2 = torch.where(hit[None, :], first.P, Pn).contiguous()
    w = torch.randn(3, m, generator=g, device=dev)
    d2 = (-(O2 / O2.norm(dim=0)) + 0.999 * w / w.norm(dim=0)).contiguous()
    last0 = torch.where(hit, first.prim, torch.full_like(first.prim, -1)).contiguous()
    rec["streams"]["incoherent"] = pair(nearest.Rays(O2, d2, maxdist=torch.full((m,), 1.5, device=dev)), last0)
    del found, first, state, vis, reach, O2, d2, w, Pn, o, d
    scene.close()
    # ---- (b), (c) a light loop's shadow queue under an occluder
    nl = args.lights
    lights = [make_light(center=c, radius=r, radiance=e) for c, r, e in LIGHT_SPECS[:nl]]
    points = max(n // (nl * 3 * spp_n * spp_n), 1)                   # about n shadow rays
    wo, N, T_ = R.gen_frame(ctx, seed, 0, points)
    uu = lambda stream, lo=0.0, hi=1.0: R.gen_uniform(ctx, seed, 0, points, stream, lo, hi)
    P = torch.stack([uu(60, 0.0, 4.0), uu(61, 0.0, 4.0), uu(62)]).contiguous()
    s = R.GgxSampler(ctx, wo, N, T_, specColor=torch.stack([uu(10 + k) for k in range(3)]), ior=uu(13, 1.05, 2.55),
                     roughness=uu(14, 0.05, 1.0), anisotropic=R.gen_aniso(ctx, seed, 0, points))
    sh = T.ggx_shader(s, KdColor=torch.stack([uu(20 + k) for k in range(3)]), Kd=uu(23), diffuseRoughness=uu(24), Ks=uu(25))
    q = T.ggx_shadow_rays(s, sh, P, lights, spp_n, seed)
    count, cap = q.count, q.capacity
    centre = (2.0, 2.0, 2.0)
    Vi, Ti, _ = icosphere(args.level, 0.7, centre)
    Vo, To, _ = icosphere(max(args.level - 1, 0), 1.0, centre)
    rays = nearest.Rays(P, q._dir, maxdist=q._maxdist, via=q._point, count=q.offsets[q.n:], rays=cap)
    state, vis, reach = (torch.empty(max(cap, 1), dtype=torch.uint8, device=dev), torch.empty(3, max(cap, 1), device=dev),
                         torch.empty(max(cap, 1), device=dev))

    def states():
        st = state[:count]
        return {k: int((st == v).sum().item()) for k, v in (("clear", 0), ("blocked", 1), ("veiled", 2))}

    found = nearest.Found(ctx, cap, planes=("P", "surface"))
    opaque = nearest.Scene(ctx, Vi, Ti)
    ones = torch.ones(3, 1, device=dev)
    one_launch = lambda: nearest_any.hits(opaque, rays, state=state, visibility=vis, reach=reach)
    kept = {}                                                        # the last result of each route, for the comparisons

    def full(sc, table):
        def run():
            kept["walk"] = shadow_walk.run(q, P, nearest.tracer(sc, opacity=table), max_steps=16)
        return run

    walk = full(opaque, ones)
    one_launch(), walk()
    rec["opaque"] = {"points": points, "lights": nl, "spp_n": spp_n, "rays": count, "triangles": opaque.nt, **states(),
                     "same_visibility": bool(torch.equal(vis[:, :count].view(torch.int32), kept["walk"].visibility[:, :count].view(torch.int32))),
                     "any": timed_spread(one_launch, repeats, warmup), "walk": timed_spread(walk, repeats, warmup),
                     "nearest": timed_spread(lambda: opaque.hits(rays, found=found), repeats, warmup)}
    rec["opaque"]["walk_over_any"] = round(rec["opaque"]["walk"]["ms"] / rec["opaque"]["any"]["ms"], 2)
    opaque.close()
    # (c) the translucent shell about the opaque sphere: surfaces 0 (the shell) and 1
    mixed = nearest.Scene(ctx, np.concatenate([Vo, Vi]), np.concatenate([To, Ti + len(Vo)]),
                          surface=np.concatenate([np.zeros(len(To), np.uint32), np.ones(len(Ti), np.uint32)]))
    table = torch.tensor([[0.3, 1.0], [0.5, 1.0], [0.7, 1.0]], device=dev)

    def two():
        kept["two"] = nearest_any.shadow(q, P, mixed, table, max_steps=16)

    full2 = full(mixed, table)
    two(), full2()
    st = kept["two"].state[:count]
    open_ = st != 1
    a, b = kept["two"].visibility[:, :count].view(torch.int32), kept["walk"].visibility[:, :count].view(torch.int32)
    rec["mixed"] = {"rays": count, "triangles": mixed.nt, "clear": int((st == 0).sum().item()), "blocked": int((st == 1).sum().item()),
                    "veiled": int((st == 2).sum().item()), "walked": kept["two"].walked, "walked_share": round(kept["two"].walked / max(count, 1), 4),
                    "same_open_rays": bool(torch.equal(a[:, open_], b[:, open_])),
                    "blocked_not_zero": int((a[:, ~open_] != 0).any(dim=0).sum().item()),
                    "walk_blocked_not_zero": int((b[:, ~open_] != 0).any(dim=0).sum().item()),
                    "two_phase": timed_spread(two, repeats, warmup), "walk": timed_spread(full2, repeats, warmup)}
    # the launch alone, inside the two-phase route's time: every translucent candidate on the ray is met, there is no best t to cull by
    flags = kept["two"].flags
    rec["mixed"]["any"] = timed_spread(lambda: nearest_any.hits(mixed, rays, opaque=flags, state=state, visibility=vis, reach=reach), repeats, warmup)
    rec["mixed"]["nearest"] = timed_spread(lambda: mixed.hits(rays, found=found), repeats, warmup)
    rec["mixed"]["walk_over_two_phase"] = round(rec["mixed"]["walk"]["ms"] / rec["mixed"]["two_phase"]["ms"], 2)
    mixed.close()


def timed_spread(fn, repeats: int, warmup: int) -> dict:
    """timed(), with the fastest and the slowest of the measured calls beside the median"""
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def bench_route(args, ctx, n: int, spp_n: int, seed: int, rec: dict) -> None:
    """the routing verbs beside the copy of their algorithmic traffic (module docstring)"""
    import torch
    from rlshaders_amd import trace as T
    dev, bins = ctx.torch_device, 3
    repeats, warmup = max(args.repeats, 9), max(args.warmup, 3)
    g = torch.Generator(device=dev).manual_seed(seed)
    share = {"even": (0.25, 0.25, 0.25, 0.25), "skewed": (0.70, 0.20, 0.09, 0.01), "one": (1.0, 0.0, 0.0, 0.0)}[args.mix]
    u = torch.rand(n, generator=g, device=dev)
    edges = torch.tensor(share, device=dev).cumsum(0)
    key = torch.bucketize(u, edges[:-1], right=True)
    bin_ = torch.where(key < bins, key, torch.full_like(key, 255)).to(torch.uint8)
    del u, key

    def with_copy(fn, bytes_, elements):
        """fn's time and the time of a copy of bytes_ / 2 bytes (bytes_ of traffic)"""
        if elements == 0:
            return None
        r = timed_spread(fn, repeats, warmup)
        a, b = (torch.empty(max(bytes_ // 2, 1), dtype=torch.uint8, device=dev) for _ in range(2))
        c = timed_spread(lambda: b.copy_(a), repeats, warmup)
        del a, b
        r.update({"elements": elements, "bytes": bytes_, "tb_per_s": rate(bytes_, r["ms"]), "copy_ms": c["ms"],
                  "copy_min_ms": c["min_ms"], "copy_max_ms": c["max_ms"], "copy_tb_per_s": rate(bytes_, c["ms"]),
                  "fraction_of_copy": round(c["ms"] / r["ms"], 4)})
        return r

    rec.update({"rays": n, "bins": bins, "mix": args.mix, "repeats": repeats, "warmup": warmup})
    plain, slotted = T.HitRoutes(ctx, n, bins), T.HitRoutes(ctx, n, bins, slot=True)
    rec["route"] = with_copy(lambda: T.route_hits(ctx, bin_, bins, routes=plain), n * 6, n)
    rec["route_slot"] = with_copy(lambda: T.route_hits(ctx, bin_, bins, slot=True, routes=slotted), n * 10, n)
    del slotted
    rec["sizes"] = plain.sizes()
    m, misses = rec["sizes"][0], rec["sizes"][bins]
    idx, miss_idx = plain.index(0), plain.index(bins)
    src = torch.rand(12, n, generator=g, device=dev)
    dense = torch.empty(12, m, device=dev)
    rec["gather_12"] = with_copy(lambda: T.route_gather(ctx, idx, list(src), list(dense)), m * (4 + 8 * 12), m)
    rec["scatter_3"] = with_copy(lambda: T.route_scatter(ctx, idx, list(dense[:3]), list(src[:3])), m * (4 + 8 * 3), m)
    rec["fill_3"] = with_copy(lambda: T.route_fill(ctx, miss_idx, (0.25, 0.3, 0.4), list(src[:3])), misses * (4 + 4 * 3), misses)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--spp-n", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fast", action="store_true", help="RLS_MATH_FAST (default EXACT)")
    ap.add_argument("--closure", choices=("ggx", "disney", "sss", "sss-hits", "ggx-lights", "disney-lights", "ggx-node", "disney-node", "skin-node",
                                          "ggx-bounce", "disney-bounce", "skin-bounce", "shadow-fold", "shadow-walk", "route", "sss-walk", "nearest", "nearest-refit", "nearest-rebuild", "nearest-group", "nearest-any"),
                    default="ggx")
    ap.add_argument("--mix", choices=("even", "skewed", "one"), default="even", help="route: the rays' split over 3 bins and the misses")
    ap.add_argument("--state", choices=("camera", "secondary", "half", "diffuse"), default="camera",
                    help="the bounce closures: every point a camera ray at depth 0, a glossy ray's hit at depth 1, or the two alternating; "
                         "skin-bounce: or a diffuse ray's hit at depth 1")
    ap.add_argument("--lights", type=int, default=2, help="the light loops: spherical lights, 1..8")
    ap.add_argument("--hit-spp-n", type=int, default=1, help="sss-hits: the light loop at the hits draws hit_spp_n^2 samples a light")
    ap.add_argument("--tracer", choices=("synthetic", "nearest"), default="synthetic",
                    help="shadow-walk: the hits prepared outside the events, or traced by rls_nearest_walk_hits inside them")
    ap.add_argument("--instances", type=int, default=64, help="nearest-group: the placed copies of the icosphere")
    ap.add_argument("--level", type=int, default=6, help="nearest: the icosphere's subdivisions (6: 81 920 triangles)")
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats must be at least 3")
    if not 1 <= args.lights <= 8:
        ap.error("--lights must be in 1..8")

    import torch
    import rlshaders_amd as R
    from rlshaders_amd import build, trace as T

    build.build_trace_library()
    ctx = R.Context(0)
    ctx.set_math_mode(args.fast)
    n, spp_n, seed = 1 << args.log2n, args.spp_n, 1234
    spp = spp_n * spp_n
    rec = {"tool": "trace_bench", "n": n, "spp_n": spp_n, "math": "fast" if args.fast else "exact", "repeats": args.repeats,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    if args.closure != "ggx":
        rec["closure"] = args.closure
        {"disney": bench_disney, "sss": bench_sss, "sss-walk": bench_sss_walk, "sss-hits": bench_sss_hits, "ggx-node": bench_node, "disney-node": bench_node,
         "skin-node": bench_skin_node, "ggx-bounce": bench_bounce, "disney-bounce": bench_bounce, "skin-bounce": bench_skin_bounce,
         "shadow-fold": bench_shadow_fold, "route": bench_route, "nearest": bench_nearest, "nearest-refit": bench_nearest_refit, "nearest-rebuild": bench_nearest_rebuild,
         "nearest-group": bench_nearest_group, "nearest-any": bench_nearest_any,
         "shadow-walk": bench_shadow_walk_nearest if args.tracer == "nearest" else bench_shadow_walk}.get(
            args.closure, bench_lights)(args, ctx, n, spp_n, seed, rec)
        ctx.close()
        print(json.dumps(rec), flush=True)
        return
    wo, N, T_ = R.gen_frame(ctx, seed, 0, n)
    ks = torch.stack([R.gen_uniform(ctx, seed, 0, n, 10 + k) for k in range(3)])
    s = R.GgxSampler(ctx, wo, N, T_, specColor=ks, ior=R.gen_uniform(ctx, seed, 0, n, 13, 1.05, 2.55),
                     roughness=R.gen_uniform(ctx, seed, 0, n, 14, 0.05, 1.0), anisotropic=R.gen_aniso(ctx, seed, 0, n))
    out = ctx.empty(3, n)
    side = ctx.empty(n)

    for lobe in ("glossy", "refract"):
        refract = lobe == "refract"
        if refract:
            integ = lambda: s.integrateRefract(spp_n, seed, traced=True)
        else:
            integ = lambda: s.integrate(spp_n, seed, out=(out, side))
        emit_fn = T.refract_rays if refract else T.glossy_rays
        q = T.RayQueue(ctx, n, spp_n, refract)
        ms_int = timed(integ, args.repeats, args.warmup)
        ms_emit = timed(lambda: emit_fn(s, spp_n, seed, queue=q), args.repeats, args.warmup)
        rays = q.count
        L = torch.rand(3, max(rays, 1), device=ctx.torch_device)
        ms_res = timed(lambda: q.resolve(L, out=out, count=rays), args.repeats, args.warmup)
        rec[lobe] = {"rays": rays, "rays_per_point": round(rays / n, 4), "integrate_ms": round(ms_int, 4)}
        rec[lobe].update(accounting(n, spp, rays, ms_emit, ms_res, refract))
        rec[lobe]["emit_over_integrate"] = round(ms_emit / ms_int, 4)
        del q, L
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
