/*
 * rlshaders_amd_trace.h -- caller-traced rlGgx, rlDisney and rlSss integrators (companion library librls_trace.so).
 *
 * The reference traces inside its integrators: integrateGlossy hands the callback triple to AiBRDFIntegrate, which
 * traces one glossy ray per sample (src/rlGgx.h:172-179), integrateRefract calls AiTrace per sample
 * (src/rlGgx.h:228-244), and rlDisney's integrateDiffuse / integrateGlossy hand theirs to AiBRDFIntegrate with
 * AI_RAY_DIFFUSE / AI_RAY_GLOSSY (src/rlDisney.cpp:240-243, 279-283).  rls_ggx_integrate / rls_ggx_integrate_refract /
 * rls_disney_integrate stand in for those rays with a uniform environment.  The calls below cut each integrator at the
 * point where the reference traces, so that a renderer can trace with its own tracer (rlSss's integrateScatter, whose
 * probe rays return hits rather than a radiance, and the light loops, whose shadow rays return a visibility, have calls of
 * their own: see the sections below):
 *
 *   1. emit:    every sample ray of the n^2-spp loop goes into a compacted, deterministic queue
 *               (direction, weight, point, sample[, kind]);
 *   2. (the renderer traces the queue and writes one radiance per ray);
 *   3. resolve: radiance x weight is reduced per point, in the reference's sample order.
 *
 * The samples are exactly those rls_ggx_integrate / rls_ggx_integrate_refract / rls_disney_integrate draw (same seed,
 * first_index, scrambled (0,2)-sequence, math mode of the context).  With a radiance of 1 on every ray the resolves
 * return, bit for bit, rls_ggx_integrate's sum_f_over_pdf, rls_ggx_integrate_refract(traced = 1, env = {1, 1, 1})'s
 * result and rls_disney_integrate's diffuse_sum / specular_sum.
 *
 * Queue layout: point-major, samples ascending within a point, CSR: point i's rays are [offsets[i], offsets[i+1]),
 * offsets[n] is the ray count.  The order depends on the inputs only.  offsets stays on the device (read offsets[n] with
 * rls_copy_to_host); no call here synchronises the host, so emit and resolve can be recorded into an rls_graph.
 * A sample whose weight is zero (all three channels for glossy and rlDisney) is not queued: it would contribute exactly
 * +0.  The resolves therefore never multiply a radiance by a zero weight -- a non-finite radiance cannot come from a
 * dropped ray.
 *
 * All pointers are device pointers owned by the caller; the library allocates nothing per call.  Link
 * librls_trace.so (it needs librlshaders_amd.so, which holds the context and error calls).
 */
#ifndef RLSHADERS_AMD_TRACE_H
#define RLSHADERS_AMD_TRACE_H

#include "rlshaders_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rls_ray_queue.kind values (refraction only) */
enum {
    RLS_RAY_TRANSMITTED = 0,   /* refracted through the microfacet: offset the origin to the far side of the surface */
    RLS_RAY_TIR_MIRROR = 1     /* total internal reflection, the mirror direction: offset it to the near side */
};

typedef struct rls_ray_queue {
    int64_t capacity;      /* rays every per-ray plane holds; must be >= n * spp_n^2 */
    int64_t *offsets;      /* [n + 1], required */
    rls_vec3 dir;          /* [capacity] x 3, required: the sample direction (unit, world space) */
    rls_rgb weight;        /* glossy, rlDisney: f / pdf (3 planes); refraction: getSampleWeight in weight.r only */
    uint32_t *point;       /* [capacity], NULL-able: the point's index in this call (0 .. n-1) */
    uint8_t *sample;       /* [capacity], NULL-able: the sample's index s in [0, spp_n^2) */
    uint8_t *kind;         /* [capacity], NULL-able, refraction only: RLS_RAY_TRANSMITTED / RLS_RAY_TIR_MIRROR */
    void *scratch;         /* device, >= rls_trace_scratch_bytes(n, spp_n) bytes: staging of the emit */
    size_t scratch_bytes;
} rls_ray_queue;

/* Device scratch an emit of n points at spp_n^2 samples needs (any emit). */
rls_status rls_trace_scratch_bytes(int64_t n, int spp_n, size_t *bytes);

/* integrateGlossy up to AiBRDFIntegrate's trace (src/rlGgx.h:172-179): per point and sample the microfacet normal,
 * L = reflect(view, M), Fresnel (src/rlGgx.h:103), f / pdf.  A ray is queued unless f / pdf is 0 in all three channels.
 * avg_reflect_weight (NULL-able): getAvgReflectWeight (src/rlGgx.h:181-184) over ALL samples, as rls_ggx_integrate
 * writes it. */
rls_status rls_trace_ggx_glossy_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, int spp_n, uint32_t seed,
                                     uint64_t first_index, const rls_ray_queue *q, float *avg_reflect_weight);

/* integrateRefract's traced branch up to AiTrace (src/rlGgx.h:228-241): per sample the refraction of the view about
 * the microfacet normal (the mirror direction on total internal reflection) and getSampleWeight.  A ray is queued
 * unless its weight is 0.  tir_fraction (NULL-able): the fraction of totally internally reflected samples, as
 * rls_ggx_integrate_refract writes it. */
rls_status rls_trace_ggx_refract_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, int spp_n, uint32_t seed,
                                      uint64_t first_index, const rls_ray_queue *q, float *tir_fraction);

/* integrateDiffuse / integrateGlossy of rlDisney up to AiBRDFIntegrate's trace (src/rlDisney.cpp:240-243, 279-283), one
 * lobe per call: lobe = RLS_RAY_DIFFUSE (the cosine lobe) or RLS_RAY_GLOSSY (the specular lobe), as rls_disney_sample
 * takes it.  Per point and sample the direction and f / pdf of the samples rls_disney_integrate draws for that lobe.  A
 * ray is queued if the sample is valid (pdf > 1e-4, src/rlDisney.cpp:309) and f / pdf is not 0 in all three channels;
 * kind is not written.  valid_count (NULL-able): the valid samples per point, rls_disney_integrate's diffuse_count /
 * specular_count.  Resolve with rls_trace_ggx_glossy_resolve. */
rls_status rls_trace_disney_emit(rls_context *ctx, int64_t n, const rls_disney_closure *c, int lobe, int spp_n,
                                 uint32_t seed, uint64_t first_index, const rls_ray_queue *q, float *valid_count);

/* AiBRDFIntegrate's sum with the traced radiance (src/rlGgx.h:172-179, src/rlDisney.cpp:240-243, 279-283): sum[i] = sum
 * over point i's rays, in queue order, of radiance[k] * weight[k] per channel -- un-normalised, the convention of
 * rls_ggx_integrate's sum_f_over_pdf and rls_disney_integrate's diffuse_sum / specular_sum.  Resolves rlGgx glossy
 * queues and rlDisney queues of either lobe.  radiance: 3 planes of offsets[n] values, indexed by ray. */
rls_status rls_trace_ggx_glossy_resolve(rls_context *ctx, int64_t n, const rls_ray_queue *q, rls_crgb radiance,
                                        rls_rgb sum);

/* integrateRefract's sum with the traced radiance (src/rlGgx.h:241-244): result[i] = (sum over point i's rays of
 * radiance[k] * weight[k]) * (1 / spp_n^2), the AiSamplerGetSampleInvCount normalisation. */
rls_status rls_trace_ggx_refract_resolve(rls_context *ctx, int64_t n, const rls_ray_queue *q, int spp_n,
                                         rls_crgb radiance, rls_rgb result);

/* ------------------------------------------------------------------------------------------
 * rlSss: SssSampler::integrateScatter (src/rlSss.h:167-280) cut where the reference traces its probe rays.
 *
 *   1. rls_trace_sss_probe_emit: one probe ray per sample (getProbeRay, src/rlSss.h:487-533) into a DENSE queue:
 *      ray j = i * spp_n^2 + s is sample s of point i.  Nothing is dropped -- a probe ray's contribution is not known
 *      before its hits are -- so offsets[i] = i * spp_n^2 and no scratch is needed.
 *   2. The renderer's part, per probe ray:
 *        - walk the ray as traceProbe does (src/rlSss.h:293-356): every hit along the ray up to maxdist, in ascending
 *          t, at most max_hits of them; the distance of a hit is the cumulative one along the ORIGINAL ray (0 < t <=
 *          maxdist), continued past each hit;
 *        - skip hits on other objects than the shading point's own (the probe's object test);
 *        - report sg->Ns at the hit aligned to sg->N as shadeProbeSample does (alignDir, src/rlSss.h:393-398);
 *        - report E = direct + indirect / pi at the hit: the irradiance BEFORE evalProfile and the cavity fade.  Either
 *          hand the hits to rls_trace_sss_hits_emit / _resolve (below, after the light loops), which emit the shadow rays of
 *          evalLightSample's light loop and integrateDiffuse's ray at every shaded hit and fill E from what the renderer
 *          traced for them; or evaluate both in the renderer's own code.
 *      The reference computes (direct * profile + indirect * profile) * fade; with one E it is (E * profile) * fade.
 *      With an indirect term of 0 the two are the same; otherwise they may differ by one rounding.
 *   3. rls_trace_sss_scatter_resolve: per point, the hits combined exactly as the integrator combines its own: the
 *      duplicate-hit test, the radius cut-off, the cavity fade, the shaded-hit count, evalProfile and the three-axis MIS
 *      pdf (src/rlSss.h:246-268, 316-317, 379-420), summed in sample order and, within a sample, in hit order.
 *
 * The samples are exactly those the analytic integrator (rls_sss_integrate_scatter in rlshaders_amd.h) draws: same seed,
 * first_index, scrambled (0,2)-sequence, math mode of the context.  Trace its queue against the integrator's plane or
 * sphere, report E = light_color * (AI_ONEOVERPI * max(0, N.L)) (0 where the gate is shut), and the resolve returns that
 * integrator's result and mean_depth bit for bit.
 * ---------------------------------------------------------------------------------------- */

/* the deepest probe walk the resolve takes: kMaxProbeDepth, src/rlSss.h:105 */
#define RLS_MAX_PROBE_HITS 12

typedef struct rls_probe_queue {
    int64_t capacity;      /* rays every per-ray plane holds; must be >= n * spp_n^2 */
    int64_t *offsets;      /* [n + 1], required: CSR like rls_ray_queue; here offsets[i] = i * spp_n^2 */
    rls_vec3 origin;       /* [capacity] x 3, required: sg->P + getProbeRay's offset (src/rlSss.h:487-533) */
    rls_vec3 dir;          /* [capacity] x 3, required: the probe direction (one of -N, U, V of the point's frame) */
    float *maxdist;        /* [capacity], required: ray.maxdist */
    uint32_t *point;       /* [capacity], NULL-able: the point's index in this call (0 .. n-1) */
    uint8_t *sample;       /* [capacity], NULL-able: the sample's index s in [0, spp_n^2) */
} rls_probe_queue;

typedef struct rls_probe_hits {
    int max_hits;          /* 1 .. RLS_MAX_PROBE_HITS: the hit slots per ray */
    int64_t stride;        /* >= n * spp_n^2: hit k of ray j is element k * stride + j of the planes below, which hold
                              max_hits * stride floats each */
    const uint8_t *count;  /* [n * spp_n^2], required: the hits reported for ray j; values above max_hits read as max_hits */
    rls_cvec3 P;           /* required: the hit position, ascending t along the ray */
    rls_cvec3 N;           /* required: sg->Ns at the hit, aligned to sg->N */
    rls_crgb irradiance;   /* required: E, before evalProfile and the cavity fade (see above) */
} rls_probe_hits;

/* getProbeRay for every sample of integrateScatter's loop (src/rlSss.h:224-228): per point the closure's profile and frame
 * (N, T, has_dPdu as the integrator reads them), P = sg->P.  Writes offsets, origin, dir, maxdist and, where given, point
 * and sample for all n * spp_n^2 rays, point-major with samples ascending.  Never synchronises the host. */
rls_status rls_trace_sss_probe_emit(rls_context *ctx, int64_t n, const rls_sss_closure *c, rls_cvec3 P, int spp_n,
                                    uint32_t seed, uint64_t first_index, const rls_probe_queue *q);

/* integrateScatter's combination of the renderer's hits (src/rlSss.h:245-279).  c, P, spp_n: those of the emit; q: its
 * queue (only the capacity is read: the hits are indexed by ray).  Per point, with prev = P at the start of every ray and
 * the hits visited in reported order: a hit is skipped unless |prev - hit| > AI_EPSILON, then prev = hit; d = hit - P,
 * skipped if |d| > maxRadius; the cavity fade where use_cavity_fade is set, skipped unless fade > AI_EPSILON; counted as
 * shaded; irr = (E * profile(|d|)) * fade per channel, skipped if 0 in all three; sum += irr / mis_pdf(d, N) (literal_matrix
 * as in the MIS pdf call of rlshaders_amd.h).  result = (sss_color * sum) * (1 / spp_n^2); mean_depth (NULL-able) = shaded
 * hits / spp_n^2. */
rls_status rls_trace_sss_scatter_resolve(rls_context *ctx, int64_t n, const rls_sss_closure *c, rls_cvec3 P, int spp_n,
                                         const rls_probe_queue *q, const rls_probe_hits *h, int use_cavity_fade,
                                         int literal_matrix, rls_rgb result, float *mean_depth);

/* ------------------------------------------------------------------------------------------
 * The light loops of rlGgx and rlDisney (`while (AiLightsGetSample(sg))`, src/rlGgx.cpp:285-299, src/rlDisney.cpp:695-705)
 * cut where AiEvaluateLightSample needs the light's visibility.  rls_ggx_direct_lighting / rls_disney_direct_lighting
 * (rlshaders_amd.h; their comment describes the estimator and the spherical lights) light the points with no occluders;
 * here the renderer traces the shadow rays:
 *
 *   1. emit:    one shadow ray per term-carrying sample of the two-sample MIS estimator into a compacted queue;
 *   2. (the renderer traces each ray from sg->P along dir up to maxdist and writes one visibility per ray and channel:
 *      1 - sg->Lo in Arnold's terms; 1 unoccluded, 0 blocked, coloured shadows allowed);
 *   3. resolve: visibility x weight is reduced per point and light exactly as the analytic loop reduces its terms.
 *
 * The samples are exactly those the analytic loops draw: light l uses the scramble streams 6 l .. 6 l + 5 of
 * hash(seed, first_index + i), the same (0,2) table, cone sampling, BSDF samplers and tests, mis_mode per light and the math
 * mode of the context.  With a visibility of 1 on every ray the resolves return rls_ggx_direct_lighting's and
 * rls_disney_direct_lighting's direct_diffuse and direct_specular bit for bit.
 *
 * Rays.  A light-strategy sample (a direction drawn inside the light's cone) is ONE ray that carries both lobes' terms:
 * weight_specular = f w / p of the specular lobe, weight_diffuse = f_d w_d / p of the diffuse lobe.  A BSDF-strategy
 * sample that hits the light's cone is one ray per lobe.  A ray is queued unless every term it carries is 0; kind has one
 * bit per lobe whose term on this ray is not 0 in every channel, and the resolves add only those terms: an absent term is
 * never multiplied by a visibility.  (Every running sum of the analytic loop starts at +0; the +-0 terms that are dropped
 * would not change it.)
 *
 * Order: point-major (CSR offsets as in rls_ray_queue); within a point the lights ascend; within a light three segments:
 * the light-strategy samples, the BSDF diffuse-lobe samples, the BSDF specular-lobe samples; samples ascend within a
 * segment.  The order depends on the inputs only.  No call synchronises the host.
 * ---------------------------------------------------------------------------------------- */

/* rls_shadow_queue.kind: the light's index | strategy | the terms the ray carries */
#define RLS_SHADOW_LIGHT_MASK 0x07   /* the light's index in `lights` (0 .. RLS_MAX_LIGHTS - 1) */
#define RLS_SHADOW_BSDF       0x08   /* set: a BSDF-strategy sample (one lobe); clear: a light-strategy sample (both) */
#define RLS_SHADOW_SPECULAR   0x10   /* weight_specular is not 0: the resolve adds visibility x weight_specular */
#define RLS_SHADOW_DIFFUSE    0x20   /* weight_diffuse is not 0: the resolve adds visibility x weight_diffuse */

typedef struct rls_shadow_queue {
    int64_t capacity;        /* rays every per-ray plane holds; must be >= n * n_lights * 3 * spp_n^2 */
    int64_t *offsets;        /* [n + 1], required */
    rls_vec3 dir;            /* required: the unit direction from sg->P towards the light */
    float *maxdist;          /* required: the distance from sg->P along dir to the light's sphere (near intersection; to the
                                point of closest approach where rounding lets a light sample graze past the sphere) */
    rls_rgb weight_specular; /* required, 3 planes: the specular lobe's term (0 where the ray carries none) */
    rls_rgb weight_diffuse;  /* required: rlDisney 3 planes; rlGgx .r only (Oren-Nayar's term is one scalar) */
    uint8_t *kind;           /* required: RLS_SHADOW_* */
    uint32_t *point;         /* NULL-able: the point's index in this call (0 .. n-1) */
    uint8_t *sample;         /* NULL-able: the sample's index s in [0, spp_n^2) within its segment */
    void *scratch;           /* device, >= rls_trace_shadow_scratch_bytes(n, n_lights, spp_n) bytes: staging of the emit */
    size_t scratch_bytes;
} rls_shadow_queue;

/* Device scratch an emit of n points under n_lights lights at spp_n^2 samples needs. */
rls_status rls_trace_shadow_scratch_bytes(int64_t n, int n_lights, int spp_n, size_t *bytes);

/* The shadow rays of rls_ggx_direct_lighting's loop: the arguments are that call's (c, sh, P, lights; sh supplies
 * sampleDiffuse = !AiColorIsSmall(KdColor * Kd) and the Oren-Nayar roughness). */
rls_status rls_trace_ggx_direct_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                     rls_cvec3 P, const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                     uint64_t first_index, const rls_shadow_queue *q);

/* The shadow rays of rls_disney_direct_lighting's loop. */
rls_status rls_trace_disney_direct_emit(rls_context *ctx, int64_t n, const rls_disney_closure *c, rls_cvec3 P,
                                        const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                        uint64_t first_index, const rls_shadow_queue *q);

/* AiEvaluateLightSample's sums with the traced visibility.  Per point, light by light, four sums (light or BSDF strategy x
 * diffuse or specular lobe) grow in queue order by visibility[k] * weight[k] per channel, over the rays whose kind has the
 * lobe's bit (rlGgx: weight_diffuse.r for all three channels); then s = light_sum + bsdf_sum and t = (radiance[l] * s) *
 * (1 / spp_n^2); the first light assigns, later lights add.  rlGgx then applies diffuse *= KdColor * Kd, specular *= Ks
 * (src/rlGgx.cpp:304-305): c (only c->materials is read) and sh as the emit took them.  lights, n_lights, spp_n: those of the
 * emit.  visibility: 3 planes of offsets[n] values, indexed by ray. */
rls_status rls_trace_ggx_direct_resolve(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                        const rls_sphere_light *lights, int n_lights, int spp_n, const rls_shadow_queue *q,
                                        rls_crgb visibility, rls_rgb direct_diffuse, rls_rgb direct_specular);
rls_status rls_trace_disney_direct_resolve(rls_context *ctx, int64_t n, const rls_sphere_light *lights, int n_lights,
                                           int spp_n, const rls_shadow_queue *q, rls_crgb visibility,
                                           rls_rgb direct_diffuse, rls_rgb direct_specular);

/* ------------------------------------------------------------------------------------------
 * rlSss: shadeProbeSample's shading of the probe hits (src/rlSss.h:415-418) cut where it traces: evalLightSample (:439-454),
 * an Oren-Nayar MIS light loop at roughness 0, and integrateDiffuse (:456-484), one cosine-weighted ray.  With these the
 * renderer traces only: the probe rays; the shadow rays and diffuse rays leaving the hits; and rls_trace_sss_scatter_resolve /
 * rls_trace_skin_resolve, unchanged, run on the E planes filled here.
 *
 *   1. rls_trace_sss_hits_emit: lists the hits the scatter resolves count as shaded and emits, per listed hit, the light
 *      loop's shadow rays and (trace_diffuse) the diffuse ray, into two compacted queues over the LIST;
 *   2. (the renderer traces the shadow rays from the hit's position P[hit_element[point]] for a visibility, the diffuse rays
 *      for a radiance);
 *   3. rls_trace_sss_hits_resolve: E at every element of the hit planes.
 *
 * Which hits are listed: exactly those rls_trace_sss_scatter_resolve counts as shaded, by the one copy of its gate.  Per ray j,
 * with prev = P of the ray's point and the slots k < min(count[j], max_hits) in order, a hit is kept if |prev - hit| >
 * AI_EPSILON (then prev = hit), |hit - P| <= maxRadius and, where use_cavity_fade is set, fade > AI_EPSILON: the reference's
 * condition for calling evalLightSample / integrateDiffuse (:386, :415).  hit_element holds the kept hits' elements
 * k * stride + j, ray-major: j ascending, k ascending within a ray.
 *
 * Overflow: hits past hit_capacity are not listed and nothing is written past any capacity; hit_count still holds the true
 * number, and offsets[h] = offsets[min(hit_count, hit_capacity)] for every later h, so that offsets[hit_capacity] is the ray
 * count, as offsets[n] is elsewhere.
 *
 * Samples: the listed hit with element e draws from hash(seed, hit_first_index + e) -- by its element, not by its place in
 * the list -- the context's math mode applies, and light l uses the scramble streams 6 l .. 6 l + 5 exactly as
 * rls_trace_ggx_direct_emit does: segment 0 the light strategy (streams +0/1), segment 1 the diffuse BSDF strategy (streams
 * +4/5); there is no specular segment; mis_mode applies per light.  The closure is AiOrenNayarMISCreateData(sg, 0.0f) about the
 * hit's normal, its view along that normal (at roughness 0 the lobe reads the view only to test its side).  The frame is
 * (hitN, hitT, hitN x hitT); with hitT NULL the tangent is T = (1 + sg Nx Nx a, sg (Nx Ny a), -sg Nx), sg = copysign(1, Nz),
 * a = -1 / (sg + Nz), in IEEE float32 operations in either math mode: a stand-in for the closed AiBuildLocalFramePolar, which
 * this library takes as an input everywhere else.  maxdist, kind, the order of a hit's rays (lights ascending; within a light
 * segment 0, then 1; samples ascending) and sample are rls_shadow_queue's; point is the hit's index in the LIST.  So the rays of
 * element e are the diffuse-carrying rays rls_trace_ggx_direct_emit queues for a point with P = hitP[e], N = wo = hitN[e],
 * T = hitT[e], diffuseRoughness 0 and a KdColor * Kd that is not small, first_index = hit_first_index + e.
 *
 * Diffuse ray (trace_diffuse != 0; the reference asserts one sample, :481): dir = sampleDiffuseDirection(rx, ry, hitN) in the
 * frame above (rls_sss_sample_diffuse_direction), (rx, ry) the first point of the scrambled (0,2) sequence at stream pair 24 of
 * the same hash (what the nodes' indirect loops draw at spp_n = 1); weight.r = CLAMP(N . dir, 0, 1); queued unless the weight is
 * 0.  point is the hit's list index, sample 0; kind is not meaningful.
 *
 * Resolve: E is written at every one of the max_hits * stride elements, exactly 0 where the hit is not listed.  At a listed
 * hit direct = the light loop's diffuse sum exactly as rls_trace_ggx_direct_resolve forms it before its KdColor * Kd tail (four
 * sums a light, (radiance[l] * s) * (1 / hit_spp_n^2), the first light assigns, later lights add; black at n_lights == 0), and
 * E_c = direct_c + (radiance_c * weight) * AI_ONEOVERPI where the hit has a diffuse ray, else direct_c.  A term absent from a
 * queue never meets a visibility or a radiance.
 *
 * No call synchronises the host; both can be recorded into an rls_graph.  The list's length stays on the device: the emit
 * and the resolve run over hit_capacity entries and skip those past hit_count.
 * ---------------------------------------------------------------------------------------- */

typedef struct rls_hit_queues {
    int64_t hit_capacity;    /* shaded hits the lists below hold (at most 2^32 - 1) */
    int64_t *hit_count;      /* [1], device, required: the TRUE number of shaded hits, also when it exceeds hit_capacity */
    int64_t *hit_element;    /* [hit_capacity], required: element k * stride + j of rls_probe_hits, ray-major */
    rls_shadow_queue shadow; /* offsets [hit_capacity + 1], CSR over the hit LIST; point = list index; weight_diffuse.r only,
                                weight_specular NULL-able and never written; capacity >= hit_capacity * n_lights * 2 *
                                hit_spp_n^2; its scratch members are not read.  Not read at all when n_lights == 0 */
    rls_ray_queue diffuse;   /* integrateDiffuse's ray: offsets [hit_capacity + 1], dir, weight.r; at most one per listed hit:
                                capacity >= hit_capacity; its scratch members are not read.  Unused when trace_diffuse == 0 */
    void *scratch;           /* device, >= rls_trace_sss_hits_scratch_bytes(...) bytes: the list's and both emits' staging */
    size_t scratch_bytes;
} rls_hit_queues;

/* Device scratch a hits emit of n points at spp_n^2 probe rays needs for this list capacity, light count and hit_spp_n. */
rls_status rls_trace_sss_hits_scratch_bytes(int64_t n, int spp_n, int max_hits, int64_t hit_capacity, int n_lights,
                                            int hit_spp_n, size_t *bytes);

/* c, P, spp_n, q, use_cavity_fade: those of the scatter resolve the hits go to (q: only the capacity is read).  h: count, P
 * and N are read, irradiance is not.  hitT: the tangent at each hit in the hit planes' layout, all three planes NULL for the
 * library's own.  lights: n_lights in 0 .. RLS_MAX_LIGHTS.  hit_spp_n: the light loop's samples per hit are hit_spp_n^2. */
rls_status rls_trace_sss_hits_emit(rls_context *ctx, int64_t n, const rls_sss_closure *c, rls_cvec3 P, int spp_n,
                                   const rls_probe_queue *q, const rls_probe_hits *h, rls_cvec3 hitT, int use_cavity_fade,
                                   const rls_sphere_light *lights, int n_lights, int hit_spp_n, int trace_diffuse,
                                   uint32_t seed, uint64_t hit_first_index, const rls_hit_queues *hq);

/* h: max_hits and stride are read.  lights, n_lights, hit_spp_n, trace_diffuse, hq: those of the emit.  visibility: 3 planes
 * indexed by shadow ray (not read when n_lights == 0); radiance: 3 planes indexed by diffuse ray, NULL when !trace_diffuse.
 * E: 3 planes of max_hits * stride floats, the layout of rls_probe_hits.irradiance. */
rls_status rls_trace_sss_hits_resolve(rls_context *ctx, const rls_probe_hits *h, const rls_sphere_light *lights, int n_lights,
                                      int hit_spp_n, int trace_diffuse, const rls_hit_queues *hq, rls_crgb visibility,
                                      rls_crgb radiance, rls_rgb E);

/* ------------------------------------------------------------------------------------------
 * Whole nodes: shader_evaluate of rlGgx and rlDisney (src/rlGgx.cpp:248-327, src/rlDisney.cpp:685-727) cut at every
 * place it traces.  rls_ggx_shade / rls_disney_shade (rlshaders_amd.h) run the light loop and the indirect loops back to
 * back with no occluders and a uniform environment; here the node's emit fills one queue per loop, the renderer traces
 * them, and ONE resolve composes the node's AOVs and sg->out.RGB.
 *
 * The samples are the whole-node calls' own, NOT the stand-alone integrators': light l draws from scramble streams
 * 6 l .. 6 l + 5, and the indirect loops from the stream pairs after the lights' (pair p = streams 2 p, 2 p + 1):
 *   rlGgx:    pair 24 integrateGlossy, pair 25 integrateRefract, pair 26 indirect diffuse (AiBRDFIntegrate over the
 *             Oren-Nayar closure, src/rlGgx.cpp:315-319);
 *   rlDisney: pair 24 integrateDiffuse, pair 25 integrateGlossy.
 * (rls_trace_ggx_glossy_emit, rls_trace_ggx_refract_emit and rls_trace_disney_emit draw from pairs 0 and 1: their
 * queues are not a node's.)  The node's gates are applied by the emit and again by the resolve:
 *   rlGgx glossy:    a point whose KsColor is small (every channel below AI_EPSILON, src/rlGgx.h:174-176) has no rays;
 *   rlGgx refract:   a point with small KtColor * Kt has no rays (src/rlGgx.cpp:307-309).  traced != 0: the samples of
 *                    integrateRefract's traced branch (dir, weight.r, kind).  traced == 0: the ONE ray of the untraced
 *                    branch (src/rlGgx.h:213-222), the refraction of the view about the shading normal, weight.r =
 *                    SQR(iorOut / iorIn) * |N . dir|, sample 0, kind RLS_RAY_TRANSMITTED; no ray on total internal
 *                    reflection;
 *   rlGgx diffuse:   a point with sampleDiffuse false (small KdColor * Kd, src/rlGgx.cpp:279-281) has no rays; else per
 *                    sample a cosine-weighted direction about the shading normal and weight.r = brdf / pdf of the
 *                    Oren-Nayar closure where pdf > 0, queued unless it is 0;
 *   rlDisney:        both lobes as rls_trace_disney_emit queues them (valid: pdf > 1e-4; f / pdf not 0 in all channels).
 * The shadow member is exactly what rls_trace_ggx_direct_emit / rls_trace_disney_direct_emit produce.
 *
 * Every queue is laid out as above (point-major CSR, deterministic, no atomics); the emit fills the node's queues one
 * after another on the context's stream, one emit kernel per queue (each builds the point's closure again), and never
 * synchronises the host.  Each queue brings its own scratch of rls_trace_scratch_bytes / rls_trace_shadow_scratch_bytes;
 * the queues of ONE node emit may all point at the same scratch block, sized to the largest of them.
 *
 * Resolve, one launch: per point the light loop's sums as rls_trace_*_direct_resolve forms them and, per ray queue and
 * channel c, S_c = (sum radiance_c w) * inv with inv = 1 / spp_n^2 (1 for the refraction queue when traced == 0); then
 *   rlGgx:    direct_diffuse, direct_specular: as rls_trace_ggx_direct_resolve (black when n_lights == 0);
 *             refraction_c        = S_c(refract) * (KtColor_c * Kt)
 *             indirect_diffuse_c  = (KdColor_c * Kd) * S_c(diffuse)
 *             indirect_specular_c = S_c(glossy) * Ks
 *             out = ((direct_diffuse + direct_specular) + refraction) + (indirect_diffuse + indirect_specular)
 *   rlDisney: indirect_diffuse_c = S_c(diffuse), indirect_specular_c = S_c(specular);
 *             out = (direct_diffuse + direct_specular) + (indirect_diffuse + indirect_specular)
 * S is summed about a reference radiance, so that a uniform environment reproduces the analytic call: with Lref_c the
 * radiance of smallest magnitude among the point's rays (a property of the set of rays, not of their order), A = sum w and
 * B_c = sum (radiance_c - Lref_c) w, both grown in queue order (a ray whose radiance_c IS Lref_c adds nothing to B_c, also
 * where its weight is infinite),
 *             S_c = (A * inv) * Lref_c + B_c * inv
 * which in exact arithmetic is (sum radiance_c w) * inv; in float32 it is within (k + 3) 2^-24 inv (|Lref_c| sum |w| +
 * sum |radiance_c - Lref_c| |w|) of it for a point with k rays, and since |Lref_c| <= |radiance_c| on every ray, within
 * 3 (k + 3) 2^-24 inv sum |radiance_c| |w| (2 for radiances of one sign): a bound relative to the sum of the terms' magnitudes,
 * as a plain sum's, however bright a single ray is.  Where every ray of a point carries the same radiance, B is
 * exactly 0 and S = (sum w * inv) * radiance: the analytic loops' own expression.  An AOV whose gate is shut is exactly 0.
 * With a visibility of 1 and the same radiance env on every ray of the ray queues the resolve returns rls_ggx_shade /
 * rls_disney_shade at that env bit for bit -- env = {1, 1, 1} or any other: every AOV and out, EXACT and FAST, traced 0 and 1.
 * ---------------------------------------------------------------------------------------- */

typedef struct rls_ggx_node_queues {
    const rls_shadow_queue *shadow;  /* the light loop; NULL if and only if n_lights == 0 */
    const rls_ray_queue *glossy;     /* integrateGlossy, pair 24: dir, weight (3 planes) */
    const rls_ray_queue *refract;    /* integrateRefract, pair 25: dir, weight.r, kind */
    const rls_ray_queue *diffuse;    /* Oren-Nayar indirect diffuse, pair 26: dir, weight.r */
} rls_ggx_node_queues;

/* what the renderer traced: per queue 3 planes of offsets[n] values, indexed by ray */
typedef struct rls_ggx_node_traced {
    rls_crgb visibility;             /* the shadow queue's; not read when n_lights == 0 */
    rls_crgb glossy, refract, diffuse;   /* the radiance along each ray queue's rays */
} rls_ggx_node_traced;

typedef struct rls_disney_node_queues {
    const rls_shadow_queue *shadow;  /* the light loop; NULL if and only if n_lights == 0 */
    const rls_ray_queue *diffuse;    /* integrateDiffuse, pair 24: dir, weight (3 planes) */
    const rls_ray_queue *specular;   /* integrateGlossy, pair 25: dir, weight (3 planes) */
} rls_disney_node_queues;

typedef struct rls_disney_node_traced {
    rls_crgb visibility;             /* the shadow queue's; not read when n_lights == 0 */
    rls_crgb diffuse, specular;
} rls_disney_node_traced;

/* The rays of rls_ggx_shade: the arguments are that call's (without env).  n == 0 writes empty queues. */
rls_status rls_trace_ggx_shade_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                    rls_cvec3 P, const rls_sphere_light *lights, int n_lights, int traced, int spp_n,
                                    uint32_t seed, uint64_t first_index, const rls_ggx_node_queues *q);

/* rls_ggx_shade's AOVs and sg->out.RGB from what the renderer traced.  c, sh, lights, n_lights, traced, spp_n: those of the
 * emit.  The five AOV planes of out are required, out->out may be NULL (all three planes). */
rls_status rls_trace_ggx_shade_resolve(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                       const rls_sphere_light *lights, int n_lights, int traced, int spp_n,
                                       const rls_ggx_node_queues *q, const rls_ggx_node_traced *t,
                                       const rls_ggx_shade_out *out);

/* The rays of rls_disney_shade, and its AOVs and sg->out.RGB from what the renderer traced. */
rls_status rls_trace_disney_shade_emit(rls_context *ctx, int64_t n, const rls_disney_closure *c, rls_cvec3 P,
                                       const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                       uint64_t first_index, const rls_disney_node_queues *q);
rls_status rls_trace_disney_shade_resolve(rls_context *ctx, int64_t n, const rls_sphere_light *lights, int n_lights,
                                          int spp_n, const rls_disney_node_queues *q, const rls_disney_node_traced *t,
                                          const rls_disney_shade_out *out);

/* ------------------------------------------------------------------------------------------
 * Whole node: rlSkin.  shader_evaluate of rlSkin (src/rlSkin.cpp:174-254) cut at every place it traces.  rls_skin_integrate
 * (rlshaders_amd.h) lights the node with no occluders, a uniform environment and an analytic plane or sphere; here the emit
 * fills five queues, the renderer traces them, and ONE resolve composes the three AOVs and sg->out.RGB.
 *
 * Samples: exactly rls_skin_integrate's -- hash(seed, first_index + i), the same (0,2) table, the math mode of the context;
 * stream pair 0 the sheen lobe's integrateGlossy, 1 the specular lobe's, 2 integrateScatter; light l of the sheen lobe pairs
 * 3 + 4 l (light samples) and 4 + 4 l (BSDF samples), of the specular lobe 5 + 4 l and 6 + 4 l.  The closures are built as
 * rls_skin_integrate builds them: both lobes share one local view, neither has anisotropy.
 *
 * Emit, on the context's stream, never synchronising the host; n == 0 writes empty queues:
 *   shadow queues (sheen_shadow, specular_shadow; the light loops of :193-198 / :217-222), one per lobe, in rls_shadow_queue:
 *       weight_diffuse may be NULL and is not written; only weight_specular carries terms; kind = light | (RLS_SHADOW_BSDF for a
 *       BSDF-strategy ray) | RLS_SHADOW_SPECULAR.  A ray is queued unless its term is 0 in all three channels.  ORDER WITHIN A
 *       POINT DIFFERS FROM THE rlGgx QUEUE'S: the loop grows ONE sum per light, sample by sample, the light sample's term and
 *       then the BSDF sample's; so lights ascend, within a light samples ascend, and within a sample the light-strategy ray
 *       comes before the BSDF-strategy ray.  capacity >= n * n_lights * 2 * spp_n^2; rls_trace_shadow_scratch_bytes(n, n_lights,
 *       spp_n) is enough scratch; maxdist as in the light loops' queue.  A light whose cone is not valid (P inside it) draws
 *       nothing; a lobe whose weight is <= AI_EPSILON (:191, :214) has no rays.
 *   glossy queues (sheen_glossy, specular_glossy), one per lobe: the rays rls_trace_ggx_glossy_emit queues for a rlGgx closure
 *       with the lobe's colour, ior and roughness, at the lobe's stream pair.  A lobe with weight <= AI_EPSILON or a small
 *       colour (every channel below AI_EPSILON, src/rlGgx.h:174-176) has no rays.
 *   the mean Fresnel hand-down (src/rlSkin.cpp:204, 228, 238).  getAvgReflectWeight (src/rlGgx.h:181-184) is ONE running float
 *       sum: first over the light loops' BSDF samples (all lights, sample order), then over integrateGlossy's samples, divided
 *       by their count; with a small colour the light loops' part alone; 1 when nothing was drawn.  The emit forms that sum in
 *       that order: a lobe's shadow emit leaves (sum, count) per point in the lobe's Fresnel plane and in sssWeight, the lobe's
 *       glossy emit starts its fold there.  So the hand-over lives in the three scalar planes, never in a queue's scratch: the
 *       five queues may share one scratch block sized to the largest, and are filled one after another.  At the end
 *       sheenFresnel = avg_sheen * sheen_weight (0 for a sheen_weight <= AI_EPSILON), specularFresnel likewise, sssWeight =
 *       sss_weight * (1 - specularFresnel * (1 - sheenFresnel)): rls_skin_integrate's optional outputs bit for bit.  None of
 *       the three depends on what the renderer traces.
 *       (The three planes are the emit's working storage too: after an emit that was refused or failed their contents are
 *       undefined, and the emit's launches must stay in order on the context's stream.)
 *   probe queue (probes): rls_trace_sss_probe_emit's dense queue for scatterDist = sss_scatter_dist * sss_dist_multiplier and the
 *       frame sss_frame(N, T, dPdu = T), at pair 2; no scratch.  A point with sssWeight < AI_EPSILON (:244) has its rays
 *       written with maxdist = 0 -- the renderer finds nothing along them -- and the resolve does not read that point's hits.
 *
 * Resolve, ONE launch.  Per point, with inv = 1 / spp_n^2 and per channel c:
 *     lit_c      = +0; per light l in order: s_c = the sum in queue order of visibility_c[k] * weight_specular_c[k];
 *                  lit_c += (radiance_c[l] * s_c) * inv
 *     lobe_c     = lit_c + S_c(glossy), S_c about a reference radiance exactly as in the rlGgx / rlDisney node resolves above
 *     sheen_c    = lobe_c(sheen) * sheen_weight                            (0 * weight where the lobe's gate is shut)
 *     specular_c = lobe_c(specular) * (specular_weight * (1 - sheenFresnel))
 *     sss_c      = sssWeight < AI_EPSILON ? 0 : scatter_c * sssWeight,
 *                  scatter_c = rls_trace_sss_scatter_resolve's result, (sss_color_c * sum_c) * inv
 *     out_c      = (sheen_c + specular_c) + sss_c
 * sheenFresnel, specularFresnel and sssWeight are read from the queues struct and copied to `out` where its optional planes are
 * given.  Sums and products only, but for the scatter resolve's profile and MIS arithmetic, which follows the context's math
 * mode.  With a visibility of 1, the same radiance env on every glossy ray and the probe rays traced through
 * rls_skin_integrate's scene with E = light_color * (AI_ONEOVERPI * max(0, N.L)), the resolve returns rls_skin_integrate(env,
 * scene, lights) bit for bit: the three AOVs, out and the three scalars, EXACT and FAST.
 *
 * Both calls return RLS_ERR_INVALID_ARGUMENT, before the context is read, for: a NULL struct or required plane; shadow queues
 * that are not both present exactly when n_lights > 0; n_lights outside 0 .. RLS_MAX_LIGHTS; spp_n outside 1 .. 16; a capacity
 * or scratch too small; hits->max_hits outside 1 .. RLS_MAX_PROBE_HITS or hits->stride < n * spp_n^2.
 * ---------------------------------------------------------------------------------------- */

typedef struct rls_skin_node_queues {
    const rls_shadow_queue *sheen_shadow, *specular_shadow; /* light loops of :193-198 / :217-222; both NULL iff n_lights == 0 */
    const rls_ray_queue    *sheen_glossy, *specular_glossy; /* integrateGlossy per lobe: dir, weight (3 planes) */
    const rls_probe_queue  *probes;                         /* integrateScatter's probe rays, dense */
    float *sheenFresnel, *specularFresnel, *sssWeight;      /* [n] each, required: written by the emit, read by the resolve */
} rls_skin_node_queues;

typedef struct rls_skin_node_traced {
    rls_crgb sheen_visibility, specular_visibility;         /* not read when n_lights == 0 */
    rls_crgb sheen_glossy, specular_glossy;                 /* radiance per ray */
    const rls_probe_hits *hits;                             /* as rls_trace_sss_scatter_resolve takes them */
} rls_skin_node_traced;

/* The rays of rls_skin_integrate: the arguments are that call's (without scene and env). */
rls_status rls_trace_skin_emit(rls_context *ctx, int64_t n, const rls_skin_closure *c, rls_cvec3 P,
                               const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                               uint64_t first_index, const rls_skin_node_queues *q);

/* rls_skin_integrate's AOVs, sg->out.RGB and hand-down scalars from what the renderer traced.  c, P, lights, n_lights, spp_n:
 * those of the emit; use_cavity_fade, literal_matrix: as rls_trace_sss_scatter_resolve takes them.  The three AOV planes of out
 * are required; out->out (all three planes) and the three scalars are optional. */
rls_status rls_trace_skin_resolve(rls_context *ctx, int64_t n, const rls_skin_closure *c, rls_cvec3 P,
                                  const rls_sphere_light *lights, int n_lights, int use_cavity_fade, int literal_matrix,
                                  int spp_n, const rls_skin_node_queues *q, const rls_skin_node_traced *t,
                                  const rls_skin_integrate_out *out);

/* ------------------------------------------------------------------------------------------
 * Secondary-ray hits: rlGgx and rlDisney shaded at the hits of the rays a node emit queued.  rls_trace_*_shade_emit / _resolve
 * shade every point as a camera ray at depth 0; the rays they emit land on surfaces that carry the same nodes, and there
 * shader_evaluate reads sg->Rt, the sg->Rr* counters and the options' GI_*_depth (src/rlGgx.cpp:264-323,
 * src/rlDisney.cpp:706-725).  The bounce calls take that state PER POINT, so that one wavefront of hits may mix ray types
 * and depths; queue structs, traced structs, output structs, scratch rules and capacities are the node calls' own (a
 * refraction queue still needs n * spp_n^2 slots), and so are the samples: with every point a camera ray at depth 0 and
 * depths that leave every switch open the bounce calls write the node calls' bytes (rlGgx: traced = 1; depths.refraction = 0
 * gives traced = 0).
 *
 * Per point i, with rt = ray_type[i] (tested with & as the reference tests sg->Rt) and d = *depths:
 *   a point with rt & RLS_RT_SHADOW queues nothing and every output plane is +0 there (the reference returns an opacity:
 *   rls_trace_ggx_opacity / rls_trace_disney_opacity, at the end of this header); for every other point, cam = rt & RLS_RT_CAMERA and
 *
 *   rlGgx     sD = !small(KdColor * Kd) && Rr_diff[i] <= d.diffuse            (sampleDiffuse)
 *             sS = Rr_gloss[i] <= d.glossy
 *             tr = Rr_refr[i] < d.refraction && Rr[i] < d.total               (integrateRefract's traced branch)
 *     shadow queue:   rls_trace_ggx_direct_emit's rays, each with the terms of the open lobes only: the diffuse term and the BSDF
 *                     diffuse-lobe segment exist iff sD, the specular term and the BSDF specular-lobe segment iff sS.  A ray whose
 *                     terms are all shut is not queued; kind has the bits of the terms that are left; dir, maxdist and both
 *                     weight planes are what rls_trace_ggx_direct_emit writes for that ray (a weight whose bit is clear is not
 *                     meaningful), and the order is kept.
 *     refract queue:  behind small(KtColor * Kt) as in the node call; a tr point has integrateRefract's samples (pair 25), any
 *                     other the ONE ray of the untraced branch at sample 0, kind RLS_RAY_TRANSMITTED, none on total internal
 *                     reflection.
 *     glossy queue:   the node call's rays iff cam.      diffuse queue: the node call's rays iff cam && sD.
 *     resolve:        direct_diffuse = o_D * (KdColor * Kd), direct_specular = o_S * Ks with o_D / o_S the light loop's sums, +0
 *                     where !sD / !sS; refraction as in the node call with inv = 1 / spp_n^2 at a tr point and 1 at any other;
 *                     indirect_diffuse and indirect_specular as in the node call where cam, else 0;
 *                     out = ((direct_diffuse + direct_specular) + refraction) + (indirect_diffuse + indirect_specular) where
 *                     cam, else (direct_diffuse + direct_specular) + refraction.
 *   rlDisney  the light loop is whole: the shadow queue is rls_trace_disney_direct_emit's.
 *     diffuse queue:  the node call's rays iff cam && Rr_diff[i] < d.diffuse && Rr[i] < d.total     (shouldTraceDiffuse)
 *     specular queue: the node call's rays iff cam && Rr_gloss[i] < d.glossy && Rr[i] < d.total     (shouldTraceGlossy)
 *     resolve:        where rt & (RLS_RT_DIFFUSE | RLS_RT_GLOSSY): direct_diffuse = sum * indirectDiffuseScale, direct_specular
 *                     = sum * indirectSpecularScale, each product rounded to float32 before any sum; the indirect AOVs as in the
 *                     node call where cam, else 0; out = (direct_diffuse + direct_specular) + (indirect_diffuse +
 *                     indirect_specular) where cam, else direct_diffuse + direct_specular.
 * The AOV planes are written for every point: whether a secondary ray's AOVs are kept is the renderer's decision.
 *
 * Both calls return RLS_ERR_INVALID_ARGUMENT before the context is read for a NULL state, a NULL depths or a NULL plane of the
 * state (n > 0), and for whatever the node calls refuse.  Neither synchronises the host; both can be recorded into an
 * rls_graph.  The state planes are indexed by the point's index in THIS call, like P.
 *
 * Not covered: AiShaderGlobalsApplyOpacity's own decisions (a closed service: whether a node returns early on its opacity; the
 * opacity and shadow-ray values themselves are at the end of this header).  rls_trace_sss_hits_emit's trace_diffuse
 * (shouldTraceDiffuse at the probe hits) stays a per-call flag.  rlSkin's bounce calls are below, after the state's types.
 * ---------------------------------------------------------------------------------------- */

/* sg->Rt */
enum { RLS_RT_CAMERA = 0x01, RLS_RT_SHADOW = 0x02, RLS_RT_REFLECTED = 0x04, RLS_RT_REFRACTED = 0x08,
       RLS_RT_DIFFUSE = 0x20, RLS_RT_GLOSSY = 0x40 };
/* the options' GI_total_depth, GI_diffuse_depth, GI_glossy_depth, GI_refraction_depth */
typedef struct rls_gi_depths { int total, diffuse, glossy, refraction; } rls_gi_depths;
/* sg->Rt, sg->Rr, sg->Rr_diff, sg->Rr_gloss, sg->Rr_refr per point: [n] each, device, all five required */
typedef struct rls_ray_state {
    const uint8_t *ray_type, *Rr, *Rr_diff, *Rr_gloss, *Rr_refr;
} rls_ray_state;

/* rls_trace_ggx_shade_emit / _resolve with the per-point state in place of the call-level `traced`. */
rls_status rls_trace_ggx_bounce_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                     rls_cvec3 P, const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                     uint64_t first_index, const rls_ray_state *state, const rls_gi_depths *depths,
                                     const rls_ggx_node_queues *q);
rls_status rls_trace_ggx_bounce_resolve(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                        const rls_sphere_light *lights, int n_lights, int spp_n, const rls_ray_state *state,
                                        const rls_gi_depths *depths, const rls_ggx_node_queues *q,
                                        const rls_ggx_node_traced *t, const rls_ggx_shade_out *out);

/* rls_trace_disney_shade_emit / _resolve with the per-point state.  The resolve takes the node's indirectDiffuseScale and
 * indirectSpecularScale, parameters like the closure's: per-point planes, uniform values, or looked up through c->materials
 * (of c the resolve reads nothing else). */
rls_status rls_trace_disney_bounce_emit(rls_context *ctx, int64_t n, const rls_disney_closure *c, rls_cvec3 P,
                                        const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                        uint64_t first_index, const rls_ray_state *state, const rls_gi_depths *depths,
                                        const rls_disney_node_queues *q);
rls_status rls_trace_disney_bounce_resolve(rls_context *ctx, int64_t n, const rls_disney_closure *c,
                                           rls_param indirectDiffuseScale, rls_param indirectSpecularScale,
                                           const rls_sphere_light *lights, int n_lights, int spp_n,
                                           const rls_ray_state *state, const rls_gi_depths *depths,
                                           const rls_disney_node_queues *q, const rls_disney_node_traced *t,
                                           const rls_disney_shade_out *out);

/* The state of the hits of a queue's rays.  point: the queue's point plane (rls_ray_queue.point / rls_shadow_queue.point), rays:
 * its ray count, which the caller has read (offsets[n]); parent: the state of the points the queue was emitted for; ray_type:
 * the RLS_RT_* bits of the queue's rays; child: five WRITABLE planes of `rays` bytes.  Per ray k, with p = point[k]:
 *     child.ray_type[k] = ray_type;  child.Rr[k] = min(255, parent.Rr[p] + 1);
 *     child.Rr_diff / Rr_gloss / Rr_refr[k] = min(255, parent's + 1) where ray_type has RLS_RT_DIFFUSE / _GLOSSY / _REFRACTED,
 *     else the parent's.
 * rays == 0 launches nothing.  Never synchronises the host. */
rls_status rls_trace_ray_state_advance(rls_context *ctx, int64_t rays, const uint32_t *point, const rls_ray_state *parent,
                                       int ray_type, const rls_ray_state *child);

/* ------------------------------------------------------------------------------------------
 * Secondary-ray hits: rlSkin.  rls_trace_skin_emit / _resolve with the per-point state; shader_evaluate's switches
 * (src/rlSkin.cpp:165-256, src/rlSss.h:170-186, src/rlGgx.h:172-184) change which rays are queued AND the mean-Fresnel
 * hand-down, so sssWeight and every AOV.  Per point i, rt = ray_type[i], d = *depths:
 *   rt & RLS_RT_SHADOW:  the node returns before it shades (:169-172).  No ray in any queue, the probe rays written with
 *                        maxdist = 0, the three scalars and every output plane +0.  The opacity: rls_trace_skin_opacity.
 *   sS = Rr_gloss[i] <= d.glossy (:185) gates both GGX lobes together.  Shut: neither lobe has a shadow ray or a glossy ray;
 *                        sheen = specular = +0 (AI_RGB_BLACK, not 0 * weight); sheenFresnel = specularFresnel = 0, and sssWeight
 *                        is :238 with both at 0.
 *   first = Rr[i] == 0 (:200, :224; Rr, not the camera bit) gates each lobe's integrateGlossy.  Shut, with sS open: the lobe's
 *                        light loop still runs, its glossy queue has no ray for the point, and the lobe's mean Fresnel is the
 *                        running sum over the light loops' BSDF samples alone divided by their count -- 1 when nothing was
 *                        drawn (no lights, every light RLS_MIS_LIGHT_ONLY, no valid cone): what the node call forms for a small
 *                        lobe colour.  sheenFresnel, specularFresnel and sssWeight follow from it.
 *   dif = rt & RLS_RT_DIFFUSE (src/rlSss.h:172-186): integrateScatter is sss_color * sum_l (irradiance_l * light diffuse), an
 *                        Oren-Nayar MIS light loop at roughness 0 about the point's own normal, without probes.  The point's
 *                        probe rays get maxdist = 0 and its hits are not read (as at sssWeight < AI_EPSILON); the loop's shadow
 *                        rays go into diffuse_shadow.
 * The AOV planes are written for every point.
 *
 * q.node, t.node, out, capacities and scratch are the node calls'.  diffuse_shadow (NULL if and only if n_lights == 0) needs
 * capacity >= n * n_lights * 2 * spp_n^2; of its weight planes only weight_diffuse.r is written (weight_specular and the other two
 * may be NULL); rls_trace_shadow_scratch_bytes(n, n_lights, spp_n) is enough scratch, and it may be the node queues' shared block.
 * The emit fills it last, after the probe emit has written sssWeight.  At a point with dif, not a shadow ray's, and sssWeight >=
 * AI_EPSILON it holds the diffuse-carrying rays rls_trace_ggx_direct_emit queues for a point with this P, N, T and wo, diffuseRoughness = 0, a KdColor *
 * Kd that is not small, this first_index and the seed (seed ^ RLS_SKIN_DIFFUSE_SEED): order, kind (light | RLS_SHADOW_BSDF |
 * RLS_SHADOW_DIFFUSE), maxdist, point and sample as in rls_shadow_queue, lights ascending, per light the light-strategy segment
 * and then the BSDF-strategy segment; no specular segment.  sss_color does not gate it.  The seed is derived because the lobes'
 * light loops at the same point draw from streams 6 .. 69 of hash(seed, .) already, and the diffuse loop's 6 l .. 6 l + 5 would
 * repeat them.  Every other point has no ray in it.
 *
 * Resolve at a dif point:  sss_c = sssWeight < AI_EPSILON ? 0 : (sss_color_c * D_c) * sssWeight, D the light loop's diffuse sum
 * exactly as rls_trace_sss_hits_resolve forms its direct term: per light the light-strategy and the BSDF-strategy sum of
 * visibility_c * weight_diffuse.r in queue order, (radiance_c[l] * (their sum)) * (1 / spp_n^2), the first light assigning, the
 * later ones adding; black when n_lights == 0.  Everything else is rls_trace_skin_resolve's arithmetic behind the switches above;
 * out = (sheen + specular) + sss.
 *
 * With every point a camera ray, every counter 0 and depths >= 0 both calls write rls_trace_skin_emit / _resolve's bytes into
 * q.node and out, and diffuse_shadow is empty.  Refused, before the context is read: what the node calls refuse; a NULL state,
 * depths or (n > 0) state plane; diffuse_shadow not present exactly when n_lights > 0, or with a NULL offsets, required plane,
 * too small a capacity or scratch; a NULL diffuse_visibility plane (resolve, n_lights > 0).  Neither call synchronises the host;
 * both can be recorded into an rls_graph.
 * ---------------------------------------------------------------------------------------- */

#define RLS_SKIN_DIFFUSE_SEED 0x9E3779B9u

typedef struct rls_skin_bounce_queues {
    rls_skin_node_queues node;               /* as rls_trace_skin_emit takes them */
    const rls_shadow_queue *diffuse_shadow;  /* integrateScatter's light loop at diffuse rays' points; NULL iff n_lights == 0 */
} rls_skin_bounce_queues;

typedef struct rls_skin_bounce_traced {
    rls_skin_node_traced node;
    rls_crgb diffuse_visibility;             /* not read when n_lights == 0 */
} rls_skin_bounce_traced;

rls_status rls_trace_skin_bounce_emit(rls_context *ctx, int64_t n, const rls_skin_closure *c, rls_cvec3 P,
                                      const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                      uint64_t first_index, const rls_ray_state *state, const rls_gi_depths *depths,
                                      const rls_skin_bounce_queues *q);
rls_status rls_trace_skin_bounce_resolve(rls_context *ctx, int64_t n, const rls_skin_closure *c, rls_cvec3 P,
                                         const rls_sphere_light *lights, int n_lights, int use_cavity_fade,
                                         int literal_matrix, int spp_n, const rls_ray_state *state,
                                         const rls_gi_depths *depths, const rls_skin_bounce_queues *q,
                                         const rls_skin_bounce_traced *t, const rls_skin_integrate_out *out);

/* ------------------------------------------------------------------------------------------
 * Routing a queue's hits to the nodes.  A queue's rays land on surfaces that carry different nodes, or on nothing; every node
 * call above takes a batch of points of ONE node.  The five calls below take a traced queue from "a hit per ray" to "a dense
 * batch per node" and back:
 *
 *   rls_trace_route_hits     bin[k] (one byte per ray, written by the tracer: the node bin of the surface ray k hit, any value
 *                            >= bins -- 255 by convention -- a miss) -> a STABLE partition of the ray indices by bin:
 *                              key(k) = bin[k] < bins ? bin[k] : bins
 *                              order  = the ray indices sorted by key, ASCENDING within a key (numpy: argsort(key, kind="stable"))
 *                              offsets[b] = the number of rays with key < b, b = 0 .. bins + 1  (offsets[0] = 0, offsets[bins + 1] = rays)
 *                              slot   = the inverse permutation, order[slot[k]] == k  (where asked)
 *                            Bin b's rays are order[offsets[b] .. offsets[b + 1]); the misses are bin index `bins`.
 *   rls_trace_route_gather   dst[j] = src[index[j]], j < m, for every plane: a bin's hit data (P, N, T, wo, material ids, the
 *                            advanced rls_ray_state) out of the per-ray planes into the dense batch a node call takes.
 *                            index = order + offsets[b], m = offsets[b + 1] - offsets[b].
 *   rls_trace_route_scatter  dst[index[j]] = src[j]: a child batch's `out` back to its rays' places in the parent's radiance planes.
 *   rls_trace_route_fill     dst[p][index[j]] = value[p]: the misses' environment radiance (or a visibility).
 *
 * The caller reads offsets once with rls_copy_to_host (bins + 2 values): the bin sizes are the host argument n of the node
 * calls.  Word planes move as 32-bit patterns and byte planes as bytes: NaN payloads, -0, denormals and integer ids come through
 * bit for bit, and EXACT and FAST contexts write the same bytes.  Every position is a function of the inputs alone (a counting
 * sort from wavefront ballots and the queues' scan: no atomic), so a replay writes the same order.
 *
 * Scatter and fill write each index once where the index has no duplicate (a range of `order` has none); with duplicates which
 * write lasts is not defined.  Nothing is written outside index's elements (scatter, fill), dst[0, m) (gather), order[0, rays),
 * slot[0, rays) and offsets[0, bins + 2).  Finer routing than a node bin -- many instances of one node -- is rls_material_index's.
 *
 * All pointers are the caller's device memory except rls_trace_route_fill's dst and value, host arrays read during the call
 * (the plane structs travel by value: nothing of the host's is read after a call returns).  Nothing is allocated, no call
 * synchronises the host, every call can be recorded into an rls_graph.  m == 0 launches nothing; rls_trace_route_hits at
 * rays == 0 writes offsets (all 0) and nothing else.  Refused with RLS_ERR_INVALID_ARGUMENT before the context is read: a NULL
 * ctx, routes, offsets, scratch or planes, a NULL bin or order (rays > 0) or index (m > 0); bins outside 1 .. 16; scratch_bytes below
 * rls_trace_route_scratch_bytes(rays, bins); rays < 0 or m < 0; n_w32 outside 0 .. RLS_ROUTE_MAX_W32, n_u8 outside 0 ..
 * RLS_ROUTE_MAX_U8 or no plane at all; n_planes outside 1 .. RLS_ROUTE_MAX_W32; a NULL plane below its count; dst == src for
 * the same plane of a gather or scatter (the result would depend on scheduling).  rays > 2^32 - 1: RLS_ERR_UNSUPPORTED (order
 * is 32-bit; route in chunks).
 * ---------------------------------------------------------------------------------------- */

enum { RLS_ROUTE_MAX_BINS = 16, RLS_ROUTE_MAX_W32 = 24, RLS_ROUTE_MAX_U8 = 8 };

typedef struct rls_hit_routes {
    int bins;                /* node bins 0 .. bins - 1, 1 <= bins <= 16; bin index `bins` collects the misses */
    int64_t *offsets;        /* [bins + 2]: bin b owns order[offsets[b], offsets[b + 1]); offsets[bins + 1] == rays */
    uint32_t *order;         /* [rays]: ray indices grouped by bin, ascending within a bin */
    uint32_t *slot;          /* [rays], NULL-able: the inverse, order[slot[k]] == k */
    void *scratch;           /* >= rls_trace_route_scratch_bytes(rays, bins) */
    size_t scratch_bytes;
} rls_hit_routes;

typedef struct rls_route_planes {
    int n_w32, n_u8;                             /* planes of 32-bit words (float, uint32 ids) and of bytes (rls_ray_state) */
    const void *src_w32[RLS_ROUTE_MAX_W32];
    void *dst_w32[RLS_ROUTE_MAX_W32];
    const uint8_t *src_u8[RLS_ROUTE_MAX_U8];
    uint8_t *dst_u8[RLS_ROUTE_MAX_U8];
} rls_route_planes;

rls_status rls_trace_route_scratch_bytes(int64_t rays, int bins, size_t *bytes);
rls_status rls_trace_route_hits(rls_context *ctx, int64_t rays, const uint8_t *bin, const rls_hit_routes *r);
rls_status rls_trace_route_gather(rls_context *ctx, int64_t m, const uint32_t *index, const rls_route_planes *p);
rls_status rls_trace_route_scatter(rls_context *ctx, int64_t m, const uint32_t *index, const rls_route_planes *p);
rls_status rls_trace_route_fill(rls_context *ctx, int64_t m, const uint32_t *index, int n_planes, float *const *dst,
                                const float *value);

/* ------------------------------------------------------------------------------------------
 * Shadow rays' hits: the opacity each node returns, and the visibility of a shadow ray folded from the opacities of the surfaces
 * it crosses -- the plane every light-loop and node resolve above reads ("1 - sg->Lo in Arnold's terms").
 *
 * sg->out_opacity of the three shader_evaluate, per point i and channel c, every operation rounded to float32 by itself (no
 * math-mode form: EXACT and FAST contexts write the same bytes).  o = opacity * opacity_color_c (rlGgx, rlSkin) or opacity_c
 * (rlDisney); clamp(v) = MAX(0, MIN(v, 1)) with MIN(a, b) = a < b ? a : b and MAX(a, b) = a > b ? a : b, so a NaN gives 1 and
 * -0 stays -0 (AiColorClamp); shadow: ray_type[i] & RLS_RT_SHADOW, ray_type the rls_ray_state.ray_type plane, NULL: no point is a
 * shadow ray's.
 *                 a shadow ray's point                                        any other point
 *   rlGgx         1 - KtColor_c * Kt            (src/rlGgx.cpp:264-268)        clamp(o)   (:250, :326)
 *   rlDisney      o, NOT clamped                (src/rlDisney.cpp:685-687)     clamp(o)   (:679, :728)
 *   rlSkin        incoming_c * clamp(o)         (src/rlSkin.cpp:169-172)       clamp(o)   (:167, :255)
 * rlSkin multiplies into the sg->out_opacity it finds: `incoming`, all three planes or none (none reads as 1); it may alias
 * out_opacity plane for plane.  The parameters travel like every node parameter: per-point planes, uniform values, or columns
 * looked up through materials (entry min(id[i], count - 1)).
 *
 * AiShaderGlobalsApplyOpacity (src/rlGgx.cpp:252, src/rlDisney.cpp:681) is a closed service and stays the renderer's: whether a
 * point is skipped, made stochastically transparent or ends its shadow ray on the opacity is decided there, before any of the
 * values above is formed.  A caller whose service ends shadow rays itself passes those hits WITHOUT the shadow bit: they then
 * take the clamp(o) column, the opacity the service was handed.
 *
 * rls_trace_shadow_visibility, per shadow ray j < rays and channel c:
 *     T = base ? base_c[j] : 1;   for k = 0 .. min(count[j], max_hits) - 1, in order:  T = T * (1 - o_c(e)),  e = k * stride + j;
 *     visibility_c[j] = T
 * with o_c(e) = opacity_c[e], or opacity_c[min(index[e], table_count - 1)] where index is given (a table of out_opacity values,
 * one per distinct surface, e.g. what an opacity call wrote for table_count points).  No clamp and no early exit: a non-finite
 * opacity propagates as IEEE arithmetic gives it, and an opacity outside [0, 1] -- rlDisney's shadow branch is not clamped, and
 * rlGgx's 1 - KtColor * Kt leaves [0, 1] with KtColor * Kt -- gives a factor outside [0, 1]: bounding it is the renderer's job.  A
 * ray with no hit gets base, or 1.  base: all three planes or none; it may alias visibility plane for plane.  Nothing is written
 * at j >= rays.  The result is what rls_trace_*_direct_resolve, the node resolves and rls_trace_sss_hits_resolve take as
 * visibility.
 *
 * All four: n == 0 / rays == 0 launches nothing; never synchronise the host; can be recorded into an rls_graph.  Refused with
 * RLS_ERR_INVALID_ARGUMENT before the context is read: a NULL struct; a NULL or partly NULL output plane set; a partly NULL
 * incoming / base / rgb parameter; materials.id set with materials.count == 0; n < 0 / rays < 0; max_hits outside 1 .. 255;
 * stride < rays; a NULL count or opacity plane; index set with table_count == 0.
 * ---------------------------------------------------------------------------------------- */

typedef struct rls_ggx_opacity    { rls_param opacity; rls_param_rgb opacity_color, KtColor; rls_param Kt;
                                    rls_material_index materials; } rls_ggx_opacity;
typedef struct rls_disney_opacity { rls_param_rgb opacity; rls_material_index materials; } rls_disney_opacity;
typedef struct rls_skin_opacity   { rls_param opacity; rls_param_rgb opacity_color;
                                    rls_material_index materials; } rls_skin_opacity;

rls_status rls_trace_ggx_opacity(rls_context *ctx, int64_t n, const rls_ggx_opacity *p, const uint8_t *ray_type,
                                 rls_rgb out_opacity);
rls_status rls_trace_disney_opacity(rls_context *ctx, int64_t n, const rls_disney_opacity *p, const uint8_t *ray_type,
                                    rls_rgb out_opacity);
rls_status rls_trace_skin_opacity(rls_context *ctx, int64_t n, const rls_skin_opacity *p, const uint8_t *ray_type,
                                  rls_crgb incoming, rls_rgb out_opacity);

typedef struct rls_shadow_hits {
    int max_hits;            /* 1 .. 255: hit slots per shadow ray */
    int64_t stride;          /* >= rays: hit k of ray j is element e = k * stride + j */
    const uint8_t *count;    /* [rays], required; values above max_hits read as max_hits */
    rls_crgb opacity;        /* required: out_opacity per element (index == NULL), or a table of table_count entries */
    const uint32_t *index;   /* NULL-able: [max_hits * stride]; element e reads entry min(index[e], table_count - 1) */
    uint32_t table_count;    /* read only with index; >= 1 */
} rls_shadow_hits;

rls_status rls_trace_shadow_visibility(rls_context *ctx, int64_t rays, const rls_shadow_hits *h, rls_crgb base,
                                       rls_rgb visibility);

#ifdef __cplusplus
}
#endif

#endif /* RLSHADERS_AMD_TRACE_H */
