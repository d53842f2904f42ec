// rls_trace_probe.hpp -- rlSss's integrateScatter (src/rlSss.h:167-280) cut where it traces (part of trace.hip, included there
// inside its anonymous namespace): an emit of every probe ray (sss_probe_emit_kernel, skin_probe_emit_kernel; a dense queue: no
// scan, no compaction) and a resolve of the hits the caller's probe walk reports (sss_scatter_resolve_kernel; its walk is
// rlSkin's node resolve's too).

// integrateScatter's probe rays (getProbeRay, src/rlSss.h:224-228) into the dense queue.  Per tile the points' profile,
// frame, position and scrambles are computed once, by one thread each, into LDS; then each thread takes rays threadIdx.x,
// threadIdx.x + kBlock, ... of the tile, draws the sample and the probe ray as scatter_loop does and stores the ray at
// j = p0 * spp + its place in the tile: the tile's rays are one contiguous range of every plane.
// STREAM: the first scramble stream; point(i, p, fr): the profile and frame of point i, returns whether its rays are to be
// traced (else they are written with maxdist = 0: rlSkin's sssWeight gate).
constexpr int kEmitWords = 20;               // d[3], c1[3], c2[3], maxR, U, V, N, traced (nd_radius reads d, c1, c2, maxR only)
template <int STREAM, class IO, class PointFn>
__device__ __forceinline__ void probe_emit_tiles(const IO &a, PointFn point)
{
    __shared__ uint32_t tab[2][kMaxSpp];
    __shared__ float pt[kEmitWords][kSssEmitPoints];
    __shared__ float po[3][kSssEmitPoints];
    __shared__ uint32_t scr[2][kSssEmitPoints];
    stage_libm_tables();
    stage_table(tab, a.spp);
    const int P = a.tile_points, t = (int)threadIdx.x;
    const int64_t tiles = (a.n + P - 1) / P;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t p0 = tile * P;
        const int pc = a.n - p0 < P ? (int)(a.n - p0) : P;
        __syncthreads();                                         // the previous tile's points are consumed
        if (t < pc) {
            const int64_t i = p0 + t;
            NdProfile p;
            Frame fr;
            const bool traced = point(i, p, fr);
            const V3 Po = ld3(a.P, i);
            for (int k = 0; k < 3; k++) { pt[k][t] = p.d[k]; pt[3 + k][t] = p.c1[k]; pt[6 + k][t] = p.c2[k]; }
            pt[9][t] = p.maxR;
            pt[10][t] = fr.U.x; pt[11][t] = fr.U.y; pt[12][t] = fr.U.z;
            pt[13][t] = fr.V.x; pt[14][t] = fr.V.y; pt[15][t] = fr.V.z;
            pt[16][t] = fr.N.x; pt[17][t] = fr.N.y; pt[18][t] = fr.N.z;
            pt[19][t] = traced ? 1.0f : 0.0f;
            po[0][t] = Po.x; po[1][t] = Po.y; po[2][t] = Po.z;
            scr[0][t] = hash_u32(a.seed, a.first + (uint64_t)i, kScrambleStream + STREAM);
            scr[1][t] = hash_u32(a.seed, a.first + (uint64_t)i, kScrambleStream + STREAM + 1);
            a.q.offsets[i] = i * a.spp;
            if (i == a.n - 1) a.q.offsets[a.n] = a.n * a.spp;
        }
        __syncthreads();
        for (int u = t; u < pc * a.spp; u += rlsh::kBlock) {
            const int lp = u / a.spp, s = u - lp * a.spp;
            NdProfile p = {};
            for (int k = 0; k < 3; k++) { p.d[k] = pt[k][lp]; p.c1[k] = pt[3 + k][lp]; p.c2[k] = pt[6 + k][lp]; }
            p.maxR = pt[9][lp];
            Frame fr;
            fr.U = mk(pt[10][lp], pt[11][lp], pt[12][lp]);
            fr.V = mk(pt[13][lp], pt[14][lp], pt[15][lp]);
            fr.N = mk(pt[16][lp], pt[17][lp], pt[18][lp]);
            const float rx = bits_u01(tab[0][s] ^ scr[0][lp]);
            const float ry = bits_u01(tab[1][s] ^ scr[1][lp]);
            V3 off, dir;
            float maxdist;
            sss_probe_ray(p, fr, rx, ry, off, dir, maxdist);                 // :228
            if (pt[19][lp] == 0.0f) maxdist = 0.0f;
            const V3 O = mk(po[0][lp], po[1][lp], po[2][lp]) + off;
            const int64_t j = p0 * a.spp + u;
            const rls_probe_queue &q = a.q;
            stg(q.origin.x, j, O.x); stg(q.origin.y, j, O.y); stg(q.origin.z, j, O.z);
            stg(q.dir.x, j, dir.x); stg(q.dir.y, j, dir.y); stg(q.dir.z, j, dir.z);
            stg(q.maxdist, j, maxdist);
            if (q.point) q.point[j] = (uint32_t)(p0 + lp);
            if (q.sample) q.sample[j] = (uint8_t)s;
        }
    }
}

template <int FAST_MATH = RLS_FAST>
__global__ __launch_bounds__(rlsh::kBlock) void sss_probe_emit_kernel(SssEmitIO a)
{
    probe_emit_tiles<0>(a, [&](int64_t i, NdProfile &p, Frame &fr) {
        const rls_sss_closure &c = a.c;
        p = scatter_profile(c, pindex(c.materials, i));
        fr = sss_frame(ld3(c.N, i), ld3(c.T, i), c.has_dPdu != 0);
        return true;
    });
}

// rlSkin's integrateScatter (src/rlSkin.cpp:235-246): scatterDist = sss_scatter_dist * sss_dist_multiplier, the frame with
// dPdu, stream pair 2.  sssWeight (:238) is formed here from the two lobes' hand-downs and written; a point whose sssWeight is
// below AI_EPSILON (:244) traces nothing: its rays carry maxdist = 0.
template <int FAST_MATH = RLS_FAST>
__global__ __launch_bounds__(rlsh::kBlock) void skin_probe_emit_kernel(SkinProbeEmitIO a)
{
    constexpr bool STATE = false;
    probe_emit_tiles<4>(a, [&](int64_t i, NdProfile &p, Frame &fr) {
#include "rls_trace_body_skin_probe_point.hpp"
    });
}
// STATE (rls_trace_skin_bounce_emit): a shadow ray's point has sssWeight = +0, and neither it nor a diffuse ray's point -- where
// integrateScatter is a light loop (src/rlSss.h:172-186; skin_diffuse_emit_kernel) -- has probe rays to trace: maxdist = 0.
template <int FAST_MATH = RLS_FAST>
__global__ __launch_bounds__(rlsh::kBlock) void skin_bounce_probe_emit_kernel(SkinBounceProbeEmitIO a)
{
    constexpr bool STATE = true;
    probe_emit_tiles<4>(a, [&](int64_t i, NdProfile &p, Frame &fr) {
#include "rls_trace_body_skin_probe_point.hpp"
    });
}

// integrateScatter's combination (src/rlSss.h:245-279) of the hits the caller traced.  Per tile: one thread per ray walks
// the ray's hits as scatter_loop walks the analytic ones -- duplicate test, radius cut-off, cavity fade, shaded count,
// evalProfile, the MIS pdf -- and leaves each hit's term irr / pdf (+0 for a skipped hit) in LDS; then one thread per point
// adds its rays' terms in sample order and, within a sample, in hit order: the order of the integrator's running sums.  The
// per-point profile and frame are recomputed per ray (the same arithmetic as the integrator's, so the same bits): staged in
// LDS instead, once per point, the kernel ran slower at 2^22 points x 16 rays (2.90 against 2.44 ms; 47 KB of LDS, three
// workgroups per CU instead of four).
// Whether a probe hit is shaded (src/rlSss.h:316-317, 386, 401-415: the condition for calling evalLightSample /
// integrateDiffuse): the duplicate test against the ray's previous hit `prev` (advanced past a hit that passes it), the radius
// cut-off about the shading point Po, the cavity fade against the shading normal No.  d = hit - Po, r = |d| and fade are left
// for a shaded hit.  The one copy of the gate: the scatter resolves' walk below and the hit list (rls_trace_hits.hpp) run it.
__device__ __forceinline__ bool probe_hit_shaded(V3 &prev, V3 Po, V3 hp, V3 hn, float maxR, V3 No, bool cavity, V3 &d, float &r,
                                                 float &fade)
{
    if (!(length(prev - hp) > kEps)) return false;                       // :316-317
    prev = hp;
    d = hp - Po;
    r = length(d);
    if (r > maxR) return false;                                          // :386
    fade = 1.0f;
    if (cavity) fade = sss_cavity_fade(d, r, hn, No);
    return fade > kEps;                                                  // :415
}

// One probe ray's walk (thread t of a tile, ray j of the queue, about the shading point Po with profile p and frame fr): the
// term irr / pdf of each of its hits to term[k][.][t], its hit slots min(count, max_hits) and its shaded hits.
__device__ __forceinline__ void scatter_ray_terms(float (*term)[3][rlsh::kBlock], uint8_t *slots, uint8_t *shaded, int t,
                                                  const NdProfile &p, const Frame &fr, V3 Po, const rls_probe_hits &h, int64_t j,
                                                  bool cavity, bool literal)
{
    const int cnt = h.count[j] < h.max_hits ? (int)h.count[j] : h.max_hits;
    V3 prev = Po;
    int sh = 0;
    for (int k = 0; k < cnt; k++) {
        const int64_t at = (int64_t)k * h.stride + j;
        const V3 hp = ld3(h.P, at), hn = ld3(h.N, at);
        const float eR = ldg(h.irradiance.r, at), eG = ldg(h.irradiance.g, at), eB = ldg(h.irradiance.b, at);
        float tR = 0.0f, tG = 0.0f, tB = 0.0f;
        V3 d;
        float r, fade;
        if (probe_hit_shaded(prev, Po, hp, hn, p.maxR, fr.N, cavity, d, r, fade)) {      // shadeProbeSample, :379-420
            sh++;
            float pr, pg, pb;
            nd_profile(p, r, pr, pg, pb);
            const float iR = eR * pr * fade, iG = eG * pg * fade, iB = eB * pb * fade;
            if (!(iR == 0.0f && iG == 0.0f && iB == 0.0f)) {            // :249
                const float pdf = sss_mis_pdf(p, fr, d, hn, literal);
                tR = R_DIV(iR, pdf); tG = R_DIV(iG, pdf); tB = R_DIV(iB, pdf);
            }
        }
        term[k][0][t] = tR; term[k][1][t] = tG; term[k][2][t] = tB;
    }
    slots[t] = (uint8_t)cnt;
    shaded[t] = (uint8_t)sh;
}
// a point's sums over its spp rays, the tile's rays r0 .. r0 + spp - 1: in sample order and, within a sample, in hit order
__device__ __forceinline__ void scatter_point_sums(const float (*term)[3][rlsh::kBlock], const uint8_t *slots,
                                                   const uint8_t *shaded, int r0, int spp, float (&acc)[3], float &accD)
{
    float accR = 0.0f, accG = 0.0f, accB = 0.0f;
    accD = 0.0f;
    for (int s = 0, r = r0; s < spp; s++, r++) {
        const int cnt = slots[r];
        for (int k = 0; k < cnt; k++) { accR += term[k][0][r]; accG += term[k][1][r]; accB += term[k][2][r]; }
        accD += (float)shaded[r];
    }
    acc[0] = accR; acc[1] = accG; acc[2] = accB;
}

template <int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void sss_scatter_resolve_kernel(SssResolveIO a)
{
    __shared__ float term[RLS_MAX_PROBE_HITS][3][rlsh::kBlock];
    __shared__ uint8_t slots[rlsh::kBlock];        // the ray's hit slots: min(count, max_hits)
    __shared__ uint8_t shaded[rlsh::kBlock];
    stage_libm_tables();
    const int P = a.tile_points, t = (int)threadIdx.x;
    const int64_t tiles = (a.n + P - 1) / P;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t p0 = tile * P;
        const int pc = a.n - p0 < P ? (int)(a.n - p0) : P;
        __syncthreads();                                         // the previous tile's terms are consumed
        if (t < pc * a.spp) {
            const int lp = t / a.spp;
            const int64_t i = p0 + lp, j = p0 * a.spp + t;
            const SssResolveIO al = RLS_INT_ARGS(a);
            const rls_sss_closure &c = al.c;
            const PIndex<int64_t> pk = pindex(c.materials, i);
            const NdProfile p = scatter_profile(c, pk);
            const Frame fr = sss_frame(ld3(c.N, i), ld3(c.T, i), c.has_dPdu != 0);
            scatter_ray_terms(term, slots, shaded, t, p, fr, ld3(al.P, i), al.h, j, al.cavity != 0, al.literal != 0);
        }
        __syncthreads();
        if (t < pc) {
            const int64_t i = p0 + t;
            float acc[3], accD;
            scatter_point_sums(term, slots, shaded, t * a.spp, a.spp, acc, accD);
            const float accR = acc[0], accG = acc[1], accB = acc[2];
            const SssResolveIO al = RLS_INT_ARGS(a);
            float br, bg, bb;
            ldrgb(al.c.sss_color, pindex(al.c.materials, i), br, bg, bb);
            const float inv = 1.0f / (float)a.spp;                              // AiSamplerGetSampleInvCount
            strgb(al.result, i, br * accR * inv, bg * accG * inv, bb * accB * inv);
            if (al.depth) stg(al.depth, i, accD * inv);
        }
    }
}
