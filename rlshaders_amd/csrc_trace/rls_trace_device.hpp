// rls_trace_device.hpp -- device helpers of the caller-traced integrators (trace.hip): the launch descriptors, the staging
// format of the emits, a sample's rank among the kept samples of its point, and the int64 scan of the per-point ray counts.
#pragma once
#include "../csrc/rls_loops.hpp"
#include "../../include/rlshaders_amd_trace.h"

namespace {

// The staging of an emit: sample s of point i has slot s * n + i of every staging plane (sample-major: the lanes of a
// wavefront store to consecutive words) and a tag there: its rank among the point's kept samples | its kind << 8 (the ray's
// RLS_RAY_* bits), or kDropped where it is not queued.
constexpr uint16_t kDropped = 0xFFFF;
__device__ __forceinline__ int64_t staging_slot(int s, int64_t n, int64_t i) { return (int64_t)s * n + i; }
__device__ __forceinline__ uint16_t staging_tag(bool keep, int rank, int kind)
{
    return keep ? (uint16_t)(rank | kind << 8) : kDropped;
}
__device__ __forceinline__ int tag_rank(uint16_t tag) { return tag & 0xFF; }
__device__ __forceinline__ int tag_kind(uint16_t tag) { return tag >> 8; }

// emit: one G-lane group per point stages every sample of the point (above), and writes the point's count of kept samples
// into offsets[i] (scanned in place afterwards) and its side output
template <class Closure>
struct EmitIO {
    Closure c;
    float *dir[3];
    float *w[3];             // rlGgx glossy, rlDisney: 3 planes; rlGgx refraction: w[0]
    uint16_t *tag;
    int64_t *count;          // = the queue's offsets
    float *side;             // avg_reflect_weight / tir_fraction / valid_count, NULL-able
    int64_t n;
    int spp;
    uint32_t seed;
    uint64_t first;
};

struct TraceCompactIO {
    const float *sdir[3];
    const float *sw[3];
    const uint16_t *tag;
    const int64_t *offsets;
    rls_ray_queue q;
    int64_t n;
    int spp;
    int tile_points;         // points per compaction tile: min(kCompactMaxPoints, kCompactSlots / spp)
};
constexpr int kCompactSlots = 4096;          // samples per compaction tile (LDS: 4 B each for the position and one plane)
constexpr int kCompactMaxPoints = 256;       // (a point's local index in a tile is 8 bits)

struct TraceResolveIO {
    const int64_t *offsets;
    const float *w[3];
    rls_crgb L;
    rls_rgb out;
    float scale;             // refraction: 1 / spp (applied after the sum); glossy: unused
    int64_t n;
};
constexpr int kResolveTile = 1024;           // rays per tile of a resolve's walk (ray_sums, rls_trace_queue.hpp)

// The light loops (rls_shadow_queue).  A point has n_lights x 3 x spp slots: slot (l * 3 + segment) * spp + s is sample s of
// light l's segment (0 the light-strategy samples, 1 the BSDF diffuse-lobe samples, 2 the BSDF specular-lobe samples), staged
// sample-major like the other emits: slot t of point i at t * n + i.  With up to kShadowMaxSlots slots per point the rank
// needs 13 bits: the tag is 32 bits wide, rank | kind << 16 (kind: the queue's RLS_SHADOW_* byte), or kShadowDropped.
constexpr uint32_t kShadowDropped = 0xFFFFFFFFu;
constexpr int kShadowSegments = 3;
constexpr int kShadowMaxSlots = RLS_MAX_LIGHTS * kShadowSegments * kMaxSpp;      // 6144: also the slots of a compaction tile
constexpr int kShadowPlanes = 10;            // staged floats per slot: dir[3], maxdist, weight_specular[3], weight_diffuse[3]
__device__ __forceinline__ uint32_t shadow_tag(bool keep, int rank, int kind)
{
    return keep ? (uint32_t)rank | (uint32_t)kind << 16 : kShadowDropped;
}

// Secondary-ray hits (rls_trace_*_bounce_emit / _resolve): the caller's per-point ray state and the options' depth limits, and
// the ray-depth switches of the two shader_evaluate read off them at point i -- each switch written here once, for the emits
// that gate a queue by it and the resolve that gates the AOV.  A point of a shadow ray (sg->Rt & AI_RAY_SHADOW,
// src/rlGgx.cpp:264-269) shades nothing: every switch is shut.
struct BounceState {
    rls_ray_state s;
    rls_gi_depths d;
};
struct BounceGates {
    bool lit;                // not a shadow ray's point: the light loop runs
    bool cam;                // sg->Rt & AI_RAY_CAMERA: the indirect loops and their AOVs (src/rlGgx.cpp:307, src/rlDisney.cpp:713)
    bool diffuse;            // rlGgx: Rr_diff <= GI_diffuse_depth, sampleDiffuse's depth half (src/rlGgx.cpp:280)
    bool specular;           // rlGgx: Rr_gloss <= GI_glossy_depth (:292)
    bool traced;             // rlGgx: Rr_refr < GI_refraction_depth && Rr < GI_total_depth, integrateRefract's branch (src/rlGgx.h:210)
    bool scaled;             // rlDisney: sg->Rt & (AI_RAY_DIFFUSE | AI_RAY_GLOSSY), the direct terms' scales (src/rlDisney.cpp:706)
    bool trace_diffuse;      // rlDisney: cam && Rr_diff < GI_diffuse_depth && Rr < GI_total_depth (shouldTraceDiffuse, :75-83)
    bool trace_glossy;       // rlDisney: cam && Rr_gloss < GI_glossy_depth && Rr < GI_total_depth
};
__device__ __forceinline__ BounceGates bounce_gates(const BounceState &b, int64_t i)
{
    const int rt = b.s.ray_type[i], rr = b.s.Rr[i], rd = b.s.Rr_diff[i], rg = b.s.Rr_gloss[i], rf = b.s.Rr_refr[i];
    BounceGates g;
    g.lit = !(rt & RLS_RT_SHADOW);
    g.cam = g.lit && (rt & RLS_RT_CAMERA);
    g.diffuse = g.lit && rd <= b.d.diffuse;
    g.specular = g.lit && rg <= b.d.glossy;
    g.traced = rf < b.d.refraction && rr < b.d.total;
    g.scaled = (rt & (RLS_RT_DIFFUSE | RLS_RT_GLOSSY)) != 0;
    g.trace_diffuse = g.cam && rd < b.d.diffuse && rr < b.d.total;
    g.trace_glossy = g.cam && rg < b.d.glossy && rr < b.d.total;
    return g;
}

// rlSkin's shader_evaluate (src/rlSkin.cpp:165-256) reads two switches the other nodes lack, beside lit and specular (its sS,
// :185).  They are written here, once, and not as members of BounceGates: with two more members there the rlGgx and rlDisney
// bounce kernels that read their gates in a loop body (the light loop's emit, the refraction emit, both resolves) compile to
// other code.
struct SkinGates : BounceGates {
    bool first;              // sg->Rr == 0, each lobe's integrateGlossy (:200, :224): Rr, not the camera bit
    bool sss_diffuse;        // sg->Rt & AI_RAY_DIFFUSE off a shadow ray: integrateScatter's Oren-Nayar light loop (src/rlSss.h:172-186)
};
__device__ __forceinline__ SkinGates skin_gates(const BounceState &b, int64_t i)
{
    SkinGates g = {};
    static_cast<BounceGates &>(g) = bounce_gates(b, i);
    g.first = b.s.Rr[i] == 0;
    g.sss_diffuse = g.lit && (b.s.ray_type[i] & RLS_RT_DIFFUSE);
    return g;
}
// the gates at point i in a body two kernels share: STATE, the bounce call's kernel, whose argument struct carries the state
template <bool STATE, class IO>
__device__ __forceinline__ SkinGates state_gates(const IO &a, int64_t i)
{
    if constexpr (STATE) return skin_gates(a.st, i);
    else return SkinGates{};
}

struct NoShader {};
template <class Closure, class Shader>
struct ShadowEmitIO {
    Closure c;
    Shader sh;               // rlGgx: the node parameters the light loop reads (sampleDiffuse, Oren-Nayar's roughness)
    rls_cvec3 P;
    rls_sphere_light lights[RLS_MAX_LIGHTS];
    int nl;
    float *dir[3];
    float *maxdist;
    float *ws[3];
    float *wd[3];            // rlGgx: wd[0] only
    uint32_t *tag;
    int64_t *count;          // = the queue's offsets
    int64_t n;
    int spp;
    uint32_t seed;
    uint64_t first;
    BounceState st;          // the bounce calls' kernels alone read it
};

struct ShadowCompactIO {
    const float *src[kShadowPlanes];     // the staging planes, in the order of kShadowPlanes above
    const uint32_t *tag;
    const int64_t *offsets;
    rls_shadow_queue q;
    int64_t n;
    int spp;
    int slots;               // per point: n_lights * 3 * spp
    int tile_points;         // min(kCompactMaxPoints, kShadowMaxSlots / slots)
};

struct ShadowResolveIO {
    const int64_t *offsets;
    const float *ws[3];
    const float *wd[3];      // rlGgx: wd[0] only
    const uint8_t *kind;
    rls_crgb vis;
    rls_rgb dd, ds;
    float rad[RLS_MAX_LIGHTS][3];
    int nl;
    float inv;               // 1 / spp
    rls_material_index materials;        // rlGgx: the tail diffuse *= KdColor * Kd, specular *= Ks
    rls_ggx_shader sh;
    int64_t n;
};
constexpr int kShadowTile = 1024;            // rays per tile of a light-loop resolve's walk (shadow_sums, rls_trace_queue.hpp)
static_assert(kShadowTile == kResolveTile, "the node resolves walk both kinds of queue through one product store");

// Whole nodes (rls_trace_*_shade_emit / _resolve).  The node's indirect loops draw from the stream pairs after the lights'
// (shade.hip, kShadeStream): kNodeStream is their first scramble stream, relative to kScrambleStream like a lobe's kStream.
constexpr int kNodeStream = 2 * 3 * RLS_MAX_LIGHTS;      // pair 24

// a ray emit of the rlGgx node: the closure's emit with the node parameters its gates read
struct GgxNodeEmitIO : EmitIO<rls_ggx_closure> {
    rls_ggx_shader sh;
    int traced;              // the refraction queue: integrateRefract's traced branch, or (0) the one ray of the untraced one
};

// the node resolves: the light loop as shadow_resolve_kernel takes it (s.nl == 0: no queue; s.dd / s.ds: the two direct AOVs;
// s.materials, s.sh: rlGgx's tails), a TraceResolveIO per ray queue (out: the queue's AOV), sg->out.RGB (NULL-able)
struct GgxNodeResolveIO {
    ShadowResolveIO s;
    TraceResolveIO glossy, refract, diffuse;
    rls_param_rgb KsColor;   // integrateGlossy's gate
    rls_rgb out;
    float inv;               // 1 / spp
    int traced;              // (the bounce call: per point, off st)
    int64_t n;
    BounceState st;          // the bounce call's kernel alone reads it
};
struct DisneyNodeResolveIO {
    ShadowResolveIO s;
    TraceResolveIO diffuse, specular;
    rls_rgb out;
    float inv;
    int64_t n;
    BounceState st;          // the bounce call's kernel alone reads these: the state, and the node's two scales on the direct
    rls_material_index materials;                // terms (indirectDiffuseScale, indirectSpecularScale)
    rls_param diffuse_scale, specular_scale;
};

// the bounce calls' ray emits: the node emits' argument structs with the state (the light loops' emit and the resolves carry it
// in their own structs: one body serves both of their kernels)
struct GgxBounceEmitIO : GgxNodeEmitIO {
    BounceState st;
};
struct DisneyBounceEmitIO : EmitIO<rls_disney_closure> {
    BounceState st;
};
// rls_trace_ray_state_advance
struct StateAdvanceIO {
    const uint32_t *point;
    rls_ray_state parent;
    uint8_t *child[5];       // ray_type, Rr, Rr_diff, Rr_gloss, Rr_refr
    int ray_type;
    int64_t rays;
};

// rlSkin's node (rls_trace_skin_emit / _resolve).  A lobe's light loop (ggx_light_loops, rls_loops.hpp) draws a light sample and a
// BSDF sample of the ONE GGX lobe per light and sample: two segments a light (0 the light-strategy ray, 1 the BSDF-strategy
// ray), slot (l * 2 + segment) * spp + s, seven staged planes (no diffuse term), the tag and the compaction of the light loops.
constexpr int kSkinShadowSegments = 2;
constexpr int kSkinShadowPlanes = 7;         // dir[3], maxdist, weight_specular[3]
struct SkinShadowEmitIO {
    rls_skin_closure c;
    rls_cvec3 P;
    rls_sphere_light lights[RLS_MAX_LIGHTS];
    int nl;
    int lobe;                // 0 sheen (stream pairs 3 + 4 l, 4 + 4 l), 1 specular (5 + 4 l, 6 + 4 l)
    float *dir[3];
    float *maxdist;
    float *ws[3];
    uint32_t *tag;
    int64_t *count;          // = the queue's offsets
    float *fsum, *fcnt;      // the hand-over to the lobe's glossy emit: the Fresnel sum and count of the loop's BSDF samples
    int64_t n;
    int spp;
    uint32_t seed;
    uint64_t first;
};
// a lobe's integrateGlossy: fsum / fcnt as the lobe's light loop left them (NULL without lights); side: the lobe's Fresnel plane
struct SkinGlossyEmitIO : EmitIO<rls_skin_closure> {
    const float *fsum, *fcnt;
};
struct SkinProbeEmitIO {
    rls_skin_closure c;
    rls_cvec3 P;
    rls_probe_queue q;
    const float *sheenFresnel, *specularFresnel;
    float *sssWeight;        // written: sss_weight * (1 - specularFresnel * (1 - sheenFresnel))
    int64_t n;
    int spp;
    int tile_points;
    uint32_t seed;
    uint64_t first;
};
// the node's resolve: per lobe the light loop's queue (ShadowResolveIO: offsets, ws, kind, vis, rad, nl, inv) and the glossy
// queue; the probe hits; the three scalars of the emit; the AOVs
struct SkinNodeResolveIO {
    rls_skin_closure c;
    rls_cvec3 P;
    ShadowResolveIO sheen_s, spec_s;
    TraceResolveIO sheen_g, spec_g;
    rls_probe_hits h;
    const float *sheenFresnel, *specularFresnel, *sssWeight;
    rls_skin_integrate_out o;
    float inv;               // 1 / spp
    int spp;
    int tile_points;         // of the scatter walk: sss_resolve_tile_points(spp)
    int cavity, literal;
    int64_t n;
};

// rlSkin's bounce calls (rls_trace_skin_bounce_emit / _resolve): the node's argument structs with the state behind them -- the node
// kernels keep their own structs, and with them their kernel arguments -- and the Oren-Nayar light loop that stands in for
// integrateScatter at a diffuse ray's point (skin_diffuse_emit_kernel, rls_trace_hits.hpp): the hit list's staging (HitEmitIO)
// over points, rays only where the point's state and its sssWeight (as the probe emit left it) open the loop.
struct SkinBounceShadowEmitIO : SkinShadowEmitIO {
    BounceState st;
};
struct SkinBounceGlossyEmitIO : SkinGlossyEmitIO {
    BounceState st;
};
struct SkinBounceProbeEmitIO : SkinProbeEmitIO {
    BounceState st;
};
struct SkinDiffuseEmitIO {
    rls_cvec3 wo, N, T;      // the closure's
    rls_cvec3 P;
    const float *sssWeight;
    rls_sphere_light lights[RLS_MAX_LIGHTS];
    int nl;
    float *dir[3];
    float *maxdist;
    float *wd[3];            // wd[0] only
    uint32_t *tag;
    int64_t *count;          // = the queue's offsets
    int64_t n;
    int spp;
    uint32_t seed;
    uint64_t first;
    BounceState st;
};
// dif_s: the Oren-Nayar loop's queue (offsets, wd[0], kind, vis, rad, nl, inv; nl == 0: no queue)
struct SkinBounceResolveIO : SkinNodeResolveIO {
    ShadowResolveIO dif_s;
    BounceState st;
};

// rlSss: the probe-ray emit and the scatter resolve.  Both walk tiles of `tile_points` consecutive points: ray j = i * spp + s
// of the dense queue is ray j - p0 * spp of the tile that starts at point p0.  The emit takes up to kSssEmitRays rays per
// tile (several per thread), the resolve up to kBlock (one per thread: its LDS holds the terms of every hit of the tile).
struct SssEmitIO {
    rls_sss_closure c;
    rls_cvec3 P;
    rls_probe_queue q;
    int64_t n;
    int spp;
    int tile_points;
    uint32_t seed;
    uint64_t first;
};

struct SssResolveIO {
    rls_sss_closure c;
    rls_cvec3 P;
    rls_probe_hits h;
    rls_rgb result;
    float *depth;            // mean_depth, NULL-able
    int64_t n;
    int spp;
    int tile_points;
    int cavity, literal;
};

// rlSss's probe hits shaded through the caller's tracer (rls_trace_sss_hits_emit / _resolve, rls_trace_hits.hpp).  The gate
// pass walks the probe rays in the probe emit's tiles and leaves per ray the mask of its shaded slots and their number (scanned
// in place afterwards); the list pass turns both into hit_element and hit_count.
struct HitGateIO {
    rls_sss_closure c;
    rls_cvec3 P;
    rls_probe_hits h;        // count, P, N read
    uint16_t *mask;          // [rays]: bit k set where slot k of the ray is shaded
    int64_t *count;          // [rays + 1]
    int64_t n;
    int spp;
    int tile_points;
    int cavity;
};
struct HitListIO {
    const uint16_t *mask;
    const int64_t *offsets;  // the scanned counts: offsets[rays] = the shaded hits
    int64_t rays, stride, capacity;
    int64_t *hit_element, *hit_count;
};
// The light loop and the diffuse ray over the hit LIST: "point" i is list entry i of n = hit_capacity, live while i <
// min(*hit_count, n).  The light loop's staging is the light loops' with two segments a light and without the specular
// planes (kStageSpecular below); the diffuse ray's is a sample-ray emit's at one sample: dir, weight.r, 16-bit tags.
struct HitEmitIO {
    rls_probe_hits h;        // P, N read
    rls_cvec3 T;             // hitT, all NULL: the library's own tangent (hit_tangent)
    const int64_t *hit_count, *hit_element;
    rls_sphere_light lights[RLS_MAX_LIGHTS];
    int nl;
    float *dir[3];
    float *maxdist;
    float *wd[3];            // wd[0] only
    uint32_t *tag;
    int64_t *count;          // = the shadow queue's offsets; NULL without lights
    float *ddir[3];          // the diffuse ray's staging; dtag NULL: no diffuse ray
    float *dw;
    uint16_t *dtag;
    int64_t *dcount;         // = the diffuse queue's offsets
    int64_t n;               // hit_capacity
    int spp;
    uint32_t seed;
    uint64_t first;
};
struct HitResolveIO {
    ShadowResolveIO s;       // the light loop over the list (s.n = hit_capacity; s.nl == 0: no queue); ws, dd, ds unused
    const int64_t *hit_count, *hit_element;
    const int64_t *doffsets; // the diffuse queue's offsets, NULL: no diffuse ray
    const float *dw;
    rls_crgb L;              // the diffuse rays' radiance
    rls_rgb E;
    int64_t n;               // hit_capacity
};
constexpr int kHitStagePlanes = 5;           // dir[3], maxdist, weight_diffuse.r

// whether a light-loop emit stages weight_specular (ShadowStage, rls_trace_shadow_emit.hpp): all but the hits' Oren-Nayar loop
template <class IO> constexpr bool kStageSpecular = true;
template <> constexpr bool kStageSpecular<HitEmitIO> = false;
template <> constexpr bool kStageSpecular<SkinDiffuseEmitIO> = false;

constexpr int kSssEmitRays = 4 * rlsh::kBlock;
constexpr int kSssEmitPoints = rlsh::kBlock;       // (one thread per point computes the point's part)
inline int sss_emit_tile_points(int spp) { return kSssEmitRays / spp < kSssEmitPoints ? kSssEmitRays / spp : kSssEmitPoints; }
inline int sss_resolve_tile_points(int spp) { return spp >= rlsh::kBlock ? 1 : rlsh::kBlock / spp; }

// Rank of this lane's sample among the kept samples of its point, in sample order.  The G lanes of a group hold G
// consecutive samples (lane `sub` the sub-th); `run` counts the kept samples of the group's earlier rounds and is advanced
// past this round.  Every lane of the wavefront calls it (ballot).
template <int G>
__device__ __forceinline__ int group_rank(bool keep, int sub, int &run)
{
    const uint64_t m = __builtin_amdgcn_ballot_w64(keep);
    const int base = (int)(threadIdx.x & 63u) & ~(G - 1);
    uint64_t gm = m;
    if constexpr (G < 64) gm = (m >> base) & ((1ull << G) - 1ull);
    const int rank = run + __builtin_popcountll(gm & ((1ull << sub) - 1ull));
    run += __builtin_popcountll(gm);
    return rank;
}

// exclusive scan of one value per thread over the workgroup; `total` = the workgroup's sum
__device__ __forceinline__ int64_t block_excl_scan(int64_t v, int64_t &total)
{
    __shared__ int64_t wsum[rlsh::kBlock / 64];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    int64_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int64_t before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < rlsh::kBlock / 64; w++) {
        if (w < wave) before += wsum[w];
        tot += wsum[w];
    }
    __syncthreads();         // wsum is reused by the next call
    total = tot;
    return before + x - v;
}

constexpr int kScanPer = 8;                               // values per thread of a scan tile
constexpr int64_t kScanTile = (int64_t)rlsh::kBlock * kScanPer;

// exclusive scan of v[0, count) (count <= kScanTile) in place, plus `carry`; returns the tile's sum.  Loads and stores are
// coalesced through LDS; each thread scans kScanPer consecutive values.
__device__ __forceinline__ int64_t scan_tile(int64_t *v, int64_t count, int64_t carry)
{
    __shared__ int64_t t[kScanTile];
    for (int k = threadIdx.x; k < kScanTile; k += rlsh::kBlock) t[k] = k < count ? v[k] : 0;
    __syncthreads();
    int64_t loc[kScanPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; k++) {
        loc[k] = sum;
        sum += t[threadIdx.x * kScanPer + k];
    }
    int64_t total;
    const int64_t pre = carry + block_excl_scan(sum, total);
#pragma unroll
    for (int k = 0; k < kScanPer; k++) t[threadIdx.x * kScanPer + k] = pre + loc[k];
    __syncthreads();
    for (int k = threadIdx.x; k < count; k += rlsh::kBlock) v[k] = t[k];
    __syncthreads();         // t is reused by the next call
    return total;
}

} // namespace
