/*
 * rlshaders_amd_walk.h -- rlSss's probe walk on the device (companion library librls_walk.so).
 *
 * rls_trace_sss_probe_emit (rlshaders_amd_trace.h) queues integrateScatter's probe rays, and rls_trace_sss_scatter_resolve /
 * rls_trace_sss_hits_emit / rls_trace_skin_resolve take the hits of every ray as a list (rls_probe_hits).  Between them the
 * reference walks each ray through the object: SssSampler::traceProbe (src/rlSss.h:288-357, the stackless variant, compiled
 * in because STACKLESS_PROBE_TRACING is defined at :17) with the parts of shadeProbeSample that steer it (:379-399).  The calls
 * below are that walk, so that the renderer's part is a NEAREST-hit query and nothing else:
 *
 *   rls_trace_sss_probe_emit -> rls_walk_begin -> { the renderer's nearest hits -> rls_walk_step } x at most 12
 *                            -> rls_trace_sss_scatter_resolve (or _sss_hits_emit, _skin_resolve) on the hits the walk wrote
 *
 * The state of probe ray j (point i = j / spp, or point[j]):
 *   prev    the last ACCEPTED position; starts at P[i] (sg->P, not the probe's origin)
 *   left    msgData->maxDist; starts at the queue's maxdist[j]
 *   trials  trialCount; starts at RLS_WALK_TRIALS (kMaxProbeDepth)
 *   origin  ray.origin; starts at the queue's origin[j];     count[j] = 0
 * rls_walk_begin lists ray j as active iff maxdist[j] > 0 (a NaN is not active).
 *
 * rls_walk_step takes for every active ray the renderer's nearest hit in (0, maxdist] from the step's origin -- hit (0 / 1),
 * t (sg->Rl, measured from the step's origin), P, N, Ns, object -- and decides as the reference does:
 *   1. no hit: the ray retires.
 *   2. trials -= 1.
 *   3. a hit on another object (object != own[i]; own and object both NULL: one object everywhere):
 *        RLS_WALK_FOREIGN_STOPS  the ray retires.  This is what the COMPILED reference does: the stackless loop continues
 *                                before it moves the ray (:301-313), the identical ray finds the identical hit until the trials
 *                                run out, and nothing more is shaded.
 *        RLS_WALK_FOREIGN_SKIPS  the recursive path's behaviour (:373-377, :426-436), also what rlshaders_amd_trace.h's
 *                                wording describes: origin = hit.P, left unchanged, on to 6.
 *      (AiTraceProbe is closed: which of its hits a renderer's tracer reproduces is the renderer's matter.)
 *   4. dist = sqrt((dx dx + dy dy) + dz dz) of prev - hit.P in float32.  dist > AI_EPSILON (1e-4f): the hit is ACCEPTED --
 *      prev = hit.P, left = left - t, slot k = count[j] of the hits receives P = hit.P and N = Ns, negated when N . Ns < 0
 *      (alignDir, :393-399), count[j] = k + 1.
 *   5. origin = hit.P and maxdist = left, accepted or not (:345-346).
 *   6. the ray survives iff trials > 0 and !(left <= 0) and count[j] < max_hits (a NaN left does not stop the reference).
 * The radius cut-off, the cavity fade, evalProfile and the MIS pdf stay in rls_trace_sss_scatter_resolve, which repeats the
 * distance test on the same floats with the same outcome.
 *
 * The active list (rls_walk_rays) is what the renderer traces: a device-side count, the queue index ray[] and origin, dir,
 * maxdist compacted, survivors in ascending ray order (a stable compaction: the list depends on the inputs alone).  Two
 * lists, ping-ponged by the caller: a step reads one and writes the other.  trials travels with the list; prev is the last
 * hit the walk stored (or P[i]), so hits.count / hits.P / hits.N are both the walk's state and its result, valid after every
 * step in the layout rls_probe_hits reads.  No call but rls_walk_active synchronises the host: a step's grid is sized by the
 * caller's bound on the active count, lanes past the device count idle, so a whole walk can be recorded into an rls_graph.
 *
 * All pointers are device pointers owned by the caller.  Link librls_walk.so (it needs librlshaders_amd.so, which holds the
 * context and error calls).  Every refusal leaves "<entry point>: <text>" in rls_last_error.
 */
#ifndef RLSHADERS_AMD_WALK_H
#define RLSHADERS_AMD_WALK_H

#include "rlshaders_amd_trace.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the walk's budget of trials: kMaxProbeDepth, src/rlSss.h:105 */
#define RLS_WALK_TRIALS 12

/* rls_walk.foreign: a hit on another object than the shading point's own */
enum {
    RLS_WALK_FOREIGN_STOPS = 0,   /* the compiled (stackless) reference: the walk of that ray ends */
    RLS_WALK_FOREIGN_SKIPS = 1    /* the recursive path: the ray continues behind the hit, nothing stored */
};

/* An active list.  Every plane holds `capacity` entries; entry k < *count is one active ray. */
typedef struct rls_walk_rays {
    int64_t capacity;      /* >= the rays of the probe queue the walk began on */
    int64_t *count;        /* device, one value, required: the active rays */
    uint32_t *ray;         /* the ray's index j in the probe queue, ascending */
    rls_vec3 origin;       /* where the renderer's nearest-hit query starts */
    rls_vec3 dir;          /* the probe direction (the queue's, unchanged) */
    float *maxdist;        /* the query's reach: what is left of the queue's maxdist */
    uint8_t *trials;       /* carried state: the trials left */
} rls_walk_rays;

/* The renderer's nearest hit of every entry of the list a step reads, indexed like that list. */
typedef struct rls_walk_found {
    const uint8_t *hit;    /* required: 0 no hit in (0, maxdist], else a hit; the planes below are read only where set */
    const float *t;        /* required: sg->Rl, the distance from the step's origin */
    rls_cvec3 P;           /* required: sg->P at the hit */
    rls_cvec3 N;           /* required: sg->N at the hit */
    rls_cvec3 Ns;          /* required: sg->Ns at the hit */
    const uint32_t *object; /* NULL-able together with rls_walk.own: an id of sg->Op at the hit */
} rls_walk_found;

/* The hits the walk writes: the members of rls_probe_hits without the irradiance, writable.  Slots at or beyond count[j] are
 * never touched. */
typedef struct rls_walk_hits {
    int max_hits;          /* 1 .. RLS_MAX_PROBE_HITS */
    int64_t stride;        /* >= rays: hit k of ray j is element k * stride + j */
    uint8_t *count;        /* [rays] */
    rls_vec3 P;            /* max_hits * stride floats a plane */
    rls_vec3 N;
} rls_walk_hits;

/* One walk: what begin fixes and every step reads. */
typedef struct rls_walk {
    int64_t rays;          /* the probe queue's rays, n * spp */
    int spp;               /* spp_n^2: ray j belongs to point j / spp unless `point` is given */
    const uint32_t *point; /* NULL-able: the queue's point plane */
    rls_cvec3 P;           /* sg->P per point */
    const uint32_t *own;   /* NULL-able together with found.object: the id of each point's own object */
    int foreign;           /* RLS_WALK_FOREIGN_STOPS / _SKIPS */
    rls_walk_hits hits;
    void *scratch;         /* device, >= rls_walk_scratch_bytes(rays): an opaque block the calls of one walk share */
    size_t scratch_bytes;
} rls_walk;

/* Device scratch a walk over `rays` probe rays needs. */
rls_status rls_walk_scratch_bytes(int64_t rays, size_t *bytes);

/* Start the walk w on the dense probe queue q (origin, dir, maxdist of w->rays rays): count[j] = 0 for every ray, and the
 * rays with maxdist > 0 listed in `out` with trials = RLS_WALK_TRIALS. */
rls_status rls_walk_begin(rls_context *ctx, const rls_walk *w, const rls_probe_queue *q, const rls_walk_rays *out);

/* One step: the decision above for every entry of `in` with its nearest hit, the accepted hits stored, the survivors listed
 * in `out` (not `in`).  bound: an upper bound on *in->count that sizes the grid, or < 0 for in->capacity; entries at or
 * beyond it are not walked. */
rls_status rls_walk_step(rls_context *ctx, const rls_walk *w, const rls_walk_rays *in, const rls_walk_found *found,
                         int64_t bound, const rls_walk_rays *out);

/* The one call that waits: *host_count = *rays->count once the stream has caught up. */
rls_status rls_walk_active(rls_context *ctx, const rls_walk_rays *rays, int64_t *host_count);

#ifdef __cplusplus
}
#endif

#endif
