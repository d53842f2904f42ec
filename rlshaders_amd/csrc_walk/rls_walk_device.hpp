// rls_walk_device.hpp -- rlSss's probe walk (part of walk.hip, included there inside its anonymous namespace): the decision of
// one step for one ray, written once (walk_decide: SssSampler::traceProbe, src/rlSss.h:288-357, with the parts of
// shadeProbeSample that steer it, :379-399), and the three kernels around it.  Control flow and a handful of float operations:
// mode-free like the route and opacity kernels of the trace library, one code object in IEEE arithmetic.
//
// A step on the context's stream:
//   1. walk_step_kernel: per entry of the input list the decision, the accepted hit stored, and for the entry a flag byte
//      (survives | trials << 1) and the new maxdist; per tile of kWalkTile entries the survivors counted from wavefront ballots.
//   2. the trace library's scan (trace_scan_{block,totals,add}_kernel, csrc_trace/rls_trace_queue.hpp) over the tile counts:
//      every tile's first position in the output list; the grand total is the output list's count, written where it lives.
//   3. walk_place_kernel: the stable compaction, route_place_kernel's scheme (csrc_trace/rls_trace_route.hpp) -- a survivor's
//      place is the tile's base + the earlier wavefronts' survivors (LDS) + the survivors on the lanes below it (v_mbcnt) -- and
//      in the same pass the move of ray, origin, dir, maxdist and trials: no separate gather.
// rls_walk_begin is steps 2 and 3 behind walk_begin_kernel, which zeroes the hit counts and flags the rays with maxdist > 0.
// No atomic, no workgroup waits on another; every position is a function of the inputs alone.
//
// A tile is kBlock entries, one per lane (kWalkTile, kWalkWaves and the tile's survivor count, tile_count, are in
// rls_walk_list.hpp, which walk.hip includes ahead of this file and the shadow rays' walk shares).  The lists' count lives on the device: every kernel is launched over the caller's
// bound on it and reads the count itself, lanes past it idle, tiles past it count 0 survivors.
//
// What a ray carries from step to step: trials (a plane of the list) and maxdist = msgData->maxDist (the list's own plane:
// ray.maxdist is reset to it after every hit, :346).  prev -- sg->P, the last accepted position -- is the hit the walk stored
// last, or the shading point: it is read back from the hits, not carried.

constexpr int kWalkSurvives = 1;             // bit 0 of an entry's flag; the trials left above it

struct WalkRay { V3 prev; float left; int trials, count; };
struct WalkHit { bool hit, foreign; float t; V3 P, N, Ns; };
struct WalkVerdict { bool survives, accepted; float left; int trials; V3 N; };

// One trial of traceProbe's loop for one ray (the numbered steps of include/rlshaders_amd_walk.h).
__device__ __forceinline__ WalkVerdict walk_decide(const WalkRay &s, const WalkHit &h, int foreign, int max_hits)
{
    WalkVerdict v = { false, false, s.left, s.trials, h.Ns };
    if (!h.hit) return v;                                        // AiTraceProbe found nothing: the loop ends (:298)
    v.trials = s.trials - 1;                                     // :299
    int count = s.count;
    if (h.foreign) {
        if (foreign == RLS_WALK_FOREIGN_STOPS) return v;         // :301-313: the same ray again until the trials run out
    } else if (length(s.prev - h.P) > kEps) {                    // :316-317
        v.accepted = true;
        v.left = s.left - h.t;                                   // :383
        if (dot(h.N, h.Ns) < 0.0f) v.N = -h.Ns;                  // alignDir, :393-399
        count++;
    }
    // :298, :350 and shadeProbeSample's `probeDepth >= kMaxProbeDepth` for the caller's slots
    v.survives = v.trials > 0 && !(v.left <= 0.0f) && count < max_hits;
    return v;
}

struct WalkIO {
    rls_walk w;
    rls_probe_queue q;           // begin: the queue the walk starts on
    rls_walk_rays in, out;       // step: the list read; both: the list written
    rls_walk_found f;
    int64_t bound;               // entries walked at most (begin: w.rays)
    int64_t tiles;               // of `bound` entries, at least 1
    uint8_t *flag;               // [bound]
    float *left;                 // [bound]
    int64_t *counts;             // [tiles + 1]: the tiles' survivors, scanned in place
};

// the entries of the list read: the device count, held to the bound the planes were checked for
__device__ __forceinline__ int64_t walk_entries(const WalkIO &a)
{
    const int64_t m = *a.in.count;
    return m < 0 ? 0 : m < a.bound ? m : a.bound;
}

__global__ __launch_bounds__(rlsh::kBlock) void walk_begin_kernel(WalkIO a)
{
    __shared__ int wtot[kWalkWaves];
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t j = tile * kWalkTile + threadIdx.x;
        bool active = false;
        if (j < a.bound) {
            active = a.q.maxdist[j] > 0.0f;                      // (a NaN is not active)
            a.w.hits.count[j] = 0;
            a.flag[j] = (uint8_t)(active ? kWalkSurvives | RLS_WALK_TRIALS << 1 : 0);
        }
        int below;
        const int total = tile_count(wtot, active, below);
        if (threadIdx.x == 0) a.counts[tile] = total;
    }
}

__global__ __launch_bounds__(rlsh::kBlock) void walk_step_kernel(WalkIO a)
{
    __shared__ int wtot[kWalkWaves];
    const int64_t m = walk_entries(a);
    const rls_walk_hits &h = a.w.hits;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t k = tile * kWalkTile + threadIdx.x;
        bool survives = false;
        const int64_t j = k < m ? (int64_t)a.in.ray[k] : a.w.rays;
        if (j < a.w.rays) {                                      // (an index past the queue is no ray of this walk)
            const int64_t i = a.w.point ? (int64_t)a.w.point[j] : j / a.w.spp;
            WalkRay s;
            s.count = h.count[j];
            s.prev = s.count > 0 ? mk(h.P.x[(int64_t)(s.count - 1) * h.stride + j], h.P.y[(int64_t)(s.count - 1) * h.stride + j],
                                      h.P.z[(int64_t)(s.count - 1) * h.stride + j])
                                 : ld3(a.w.P, i);
            s.left = a.in.maxdist[k];
            s.trials = a.in.trials[k];
            WalkHit hit = {};
            hit.hit = a.f.hit[k] != 0;
            if (hit.hit) {
                hit.t = a.f.t[k];
                hit.P = ld3(a.f.P, k); hit.N = ld3(a.f.N, k); hit.Ns = ld3(a.f.Ns, k);
                hit.foreign = a.w.own != nullptr && a.f.object[k] != a.w.own[i];
            }
            const WalkVerdict v = walk_decide(s, hit, a.w.foreign, h.max_hits);
            if (v.accepted && s.count < h.max_hits) {            // (a listed ray has a free slot: it survived on count < max_hits)
                const int64_t at = (int64_t)s.count * h.stride + j;
                h.P.x[at] = hit.P.x; h.P.y[at] = hit.P.y; h.P.z[at] = hit.P.z;
                h.N.x[at] = v.N.x; h.N.y[at] = v.N.y; h.N.z[at] = v.N.z;
                h.count[j] = (uint8_t)(s.count + 1);
            }
            survives = v.survives;
            a.flag[k] = (uint8_t)((survives ? kWalkSurvives : 0) | v.trials << 1);
            a.left[k] = v.left;
        }
        int below;
        const int total = tile_count(wtot, survives, below);
        if (threadIdx.x == 0) a.counts[tile] = total;
    }
}

// BEGIN: entry k of the list read is ray k of the probe queue, as it was emitted; else a survivor of the step, behind its hit
template <bool BEGIN>
__global__ __launch_bounds__(rlsh::kBlock) void walk_place_kernel(WalkIO a)
{
    __shared__ int wtot[kWalkWaves];
    const int64_t m = BEGIN ? a.bound : walk_entries(a);
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t k = tile * kWalkTile + threadIdx.x;
        const int64_t j = BEGIN ? k : k < m ? (int64_t)a.in.ray[k] : a.w.rays;
        const bool live = BEGIN ? k < m : j < a.w.rays;
        const int fl = live ? a.flag[k] : 0;
        const bool survives = (fl & kWalkSurvives) != 0;
        int below;
        tile_count(wtot, survives, below);
        if (!survives) continue;
        const int64_t at = a.counts[tile] + below;
        a.out.ray[at] = (uint32_t)j;
        a.out.trials[at] = (uint8_t)(fl >> 1);
        if (BEGIN) {
            a.out.origin.x[at] = a.q.origin.x[k]; a.out.origin.y[at] = a.q.origin.y[k]; a.out.origin.z[at] = a.q.origin.z[k];
            a.out.dir.x[at] = a.q.dir.x[k]; a.out.dir.y[at] = a.q.dir.y[k]; a.out.dir.z[at] = a.q.dir.z[k];
            a.out.maxdist[at] = a.q.maxdist[k];
        } else {
            a.out.origin.x[at] = a.f.P.x[k]; a.out.origin.y[at] = a.f.P.y[k]; a.out.origin.z[at] = a.f.P.z[k];   // :345
            a.out.dir.x[at] = a.in.dir.x[k]; a.out.dir.y[at] = a.in.dir.y[k]; a.out.dir.z[at] = a.in.dir.z[k];
            a.out.maxdist[at] = a.left[k];                                                                         // :346
        }
    }
}
