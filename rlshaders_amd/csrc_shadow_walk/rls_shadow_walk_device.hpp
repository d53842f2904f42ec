// rls_shadow_walk_device.hpp -- the shadow rays' walk (part of shadow_walk.hip, included there inside its anonymous namespace):
// the decision of one step for one ray, written once (shadow_decide: the numbered steps of
// include/rlshaders_amd_shadow_walk.h), and the three kernels around it.  Control flow, one subtraction and one product a
// channel: mode-free like the probe walk and the opacity kernels, one code object in IEEE arithmetic.
//
// A step on the context's stream:
//   1. shadow_step_kernel: per entry of the input list the decision, T updated in the caller's visibility planes, and for the
//      entry its state (survives | steps left << 1, 16 bits: a budget of 255 does not fit the probe walk's flag byte) and the new
//      maxdist; per tile of kWalkTile entries the survivors counted from wavefront ballots.
//   2. the trace library's scan (trace_scan_{block,totals,add}_kernel, csrc_trace/rls_trace_queue.hpp) over the tile counts:
//      every tile's first position in the output list; the grand total is the output list's count, written where it lives.
//   3. shadow_place_kernel: the stable compaction of the probe walk's walk_place_kernel (csrc_walk/rls_walk_device.hpp) -- a
//      survivor's place is the tile's base + the earlier wavefronts' survivors (LDS) + the survivors on the lanes below it
//      (v_mbcnt) -- and in the same pass the move of ray, origin, dir, maxdist and the steps left: no separate gather.
// rls_shadow_walk_begin is steps 2 and 3 behind shadow_begin_kernel, which writes T = base or 1 and flags the rays with
// maxdist > 0.  No atomic, no workgroup waits on another; every position is a function of the inputs alone.
//
// A tile is kBlock entries, one per lane: kWalkTile, kWalkWaves and the tile's survivor count, tile_count, are the probe walk's
// (csrc_walk/rls_walk_list.hpp, included ahead of this file and compiled into this code object: a header both units include
// changes neither library's machine code).  The counts live on the device: every kernel is launched over the caller's bound and
// reads the count itself, lanes past it idle, tiles past it count 0 survivors.

constexpr int kShadowSurvives = 1;           // bit 0 of an entry's state; the steps left above it

struct ShadowVerdict { bool survives; float T[3], left; int steps; };

// One surface on one ray's way.  T, left, steps: the ray's state; o, t: the hit's opacity and distance.
__device__ __forceinline__ ShadowVerdict shadow_decide(const float (&T)[3], float left, int steps, bool hit, const float (&o)[3],
                                                       float t)
{
    ShadowVerdict v = { false, { T[0], T[1], T[2] }, left, steps };
    if (!hit) return v;                                          // 1.
    v.steps = steps - 1;                                         // 2.
#pragma unroll
    for (int c = 0; c < 3; c++) v.T[c] = T[c] * (1.0f - o[c]);   // 3. the fold's operation (trace.hip, shadow_visibility_kernel)
    v.left = left - t;                                           // 4.
    const bool black = v.T[0] == 0.0f && v.T[1] == 0.0f && v.T[2] == 0.0f;
    v.survives = v.steps > 0 && !(v.left <= 0.0f) && !black;     // 5.
    return v;
}

struct ShadowWalkIO {
    rls_shadow_walk w;
    rls_shadow_queue q;          // begin: the queue the walk starts on
    rls_walk_rays in, out;       // step: the list read; both: the list written
    rls_shadow_walk_found f;
    int64_t bound;               // entries walked at most (begin: w.rays)
    int64_t tiles;               // of `bound` entries, at least 1
    uint16_t *state;             // [bound]
    float *left;                 // [bound]
    int64_t *counts;             // [tiles + 1]: the tiles' survivors, scanned in place
};

// the device count `count` (NULL: the bound itself), held to the bound the planes were checked for
__device__ __forceinline__ int64_t shadow_entries(const int64_t *count, int64_t bound)
{
    if (!count) return bound;
    const int64_t m = *count;
    return m < 0 ? 0 : m < bound ? m : bound;
}

__global__ __launch_bounds__(rlsh::kBlock) void shadow_begin_kernel(ShadowWalkIO a)
{
    __shared__ int wtot[kWalkWaves];
    const int64_t m = shadow_entries(a.w.count, a.bound);
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t j = tile * kWalkTile + threadIdx.x;
        bool active = false;
        if (j < m) {
            active = a.q.maxdist[j] > 0.0f;                      // (a NaN is not active)
            float T[3] = { 1.0f, 1.0f, 1.0f };
            if (a.w.base.r) { T[0] = a.w.base.r[j]; T[1] = a.w.base.g[j]; T[2] = a.w.base.b[j]; }
            a.w.visibility.r[j] = T[0]; a.w.visibility.g[j] = T[1]; a.w.visibility.b[j] = T[2];
            a.state[j] = (uint16_t)(active ? kShadowSurvives | a.w.max_steps << 1 : 0);
        }
        int below;
        const int total = tile_count(wtot, active, below);
        if (threadIdx.x == 0) a.counts[tile] = total;
    }
}

__global__ __launch_bounds__(rlsh::kBlock) void shadow_step_kernel(ShadowWalkIO a)
{
    __shared__ int wtot[kWalkWaves];
    const int64_t m = shadow_entries(a.in.count, a.bound);
    const rls_rgb &vis = a.w.visibility;
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t k = tile * kWalkTile + threadIdx.x;
        bool survives = false;
        const int64_t j = k < m ? (int64_t)a.in.ray[k] : a.w.rays;
        if (j < a.w.rays) {                                      // (an index past the queue is no ray of this walk)
            const bool hit = a.f.hit[k] != 0;
            float o[3] = { 0.0f, 0.0f, 0.0f }, t = 0.0f;
            const float T[3] = { vis.r[j], vis.g[j], vis.b[j] };
            if (hit) {
                int64_t e = k;
                if (a.f.index) {
                    const uint32_t ix = a.f.index[k];
                    e = ix < a.f.table_count ? ix : a.f.table_count - 1;
                }
                o[0] = a.f.opacity.r[e]; o[1] = a.f.opacity.g[e]; o[2] = a.f.opacity.b[e];
                t = a.f.t[k];
            }
            const ShadowVerdict v = shadow_decide(T, a.in.maxdist[k], a.in.trials[k], hit, o, t);
            if (hit) { vis.r[j] = v.T[0]; vis.g[j] = v.T[1]; vis.b[j] = v.T[2]; }
            survives = v.survives;
            a.state[k] = (uint16_t)((survives ? kShadowSurvives : 0) | v.steps << 1);
            a.left[k] = v.left;
        }
        int below;
        const int total = tile_count(wtot, survives, below);
        if (threadIdx.x == 0) a.counts[tile] = total;
    }
}

// BEGIN: entry k of the list read is ray k of the shadow queue, as it was emitted; else a survivor of the step, behind its hit
template <bool BEGIN>
__global__ __launch_bounds__(rlsh::kBlock) void shadow_place_kernel(ShadowWalkIO a)
{
    __shared__ int wtot[kWalkWaves];
    const int64_t m = shadow_entries(BEGIN ? a.w.count : a.in.count, a.bound);
    for (int64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const int64_t k = tile * kWalkTile + threadIdx.x;
        const int64_t j = BEGIN ? k : k < m ? (int64_t)a.in.ray[k] : a.w.rays;
        const bool live = BEGIN ? k < m : j < a.w.rays;
        const int st = live ? a.state[k] : 0;
        const bool survives = (st & kShadowSurvives) != 0;
        int below;
        tile_count(wtot, survives, below);
        if (!survives) continue;
        const int64_t at = a.counts[tile] + below;
        a.out.ray[at] = (uint32_t)j;
        a.out.trials[at] = (uint8_t)(st >> 1);
        if (BEGIN) {
            int64_t from = (int64_t)a.q.point[k];
            if (a.w.via) from = a.w.via[from];
            a.out.origin.x[at] = a.w.O.x[from]; a.out.origin.y[at] = a.w.O.y[from]; a.out.origin.z[at] = a.w.O.z[from];
            a.out.dir.x[at] = a.q.dir.x[k]; a.out.dir.y[at] = a.q.dir.y[k]; a.out.dir.z[at] = a.q.dir.z[k];
            a.out.maxdist[at] = a.q.maxdist[k];
        } else {
            a.out.origin.x[at] = a.f.P.x[k]; a.out.origin.y[at] = a.f.P.y[k]; a.out.origin.z[at] = a.f.P.z[k];
            a.out.dir.x[at] = a.in.dir.x[k]; a.out.dir.y[at] = a.in.dir.y[k]; a.out.dir.z[at] = a.in.dir.z[k];
            a.out.maxdist[at] = a.left[k];
        }
    }
}
