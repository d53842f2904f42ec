// rls_trace_hits.hpp -- shadeProbeSample's shading of rlSss's probe hits (src/rlSss.h:415-418) cut where it traces (part of
// trace.hip, included there inside its anonymous namespace, after rls_trace_queue.hpp): evalLightSample's light loop
// (:439-454) and integrateDiffuse's one ray (:456-484) at every hit the scatter resolves count as shaded.  The "points" of
// this family are a sparse, gated set of the caller's hits:
//   1. sss_hits_gate_kernel: one lane per probe ray walks the ray's slots through probe_hit_shaded (rls_trace_probe.hpp: the
//      scatter resolves' own gate) and writes the mask of its shaded slots and their number;
//   2. the scan of the per-ray numbers (trace_scan_*_kernel);
//   3. sss_hits_list_kernel: hit_element (ray-major; within a ray the slots ascend) and hit_count;
//   4. sss_hits_emit_kernel: G lanes per LISTED hit stage the light loop's rays as ggx_direct_emit_kernel stages its diffuse
//      lobe's, and integrateDiffuse's ray; entries past the list's end stage nothing and count 0;
//   5. the scans and compactions of the two queues (hits_compact_kernel, trace_compact_kernel<1>) over the list;
//   6. resolve: sss_hits_fill_kernel (E = 0 everywhere), sss_hits_resolve_kernel (shadow_sums over the list, E at hit_element).
// Every position is a function of the inputs: no atomics.  The list's length lives on the device (hit_count): the kernels of
// steps 4 to 6 are launched over hit_capacity entries and read it there; no call synchronises the host.

// The tangent at a hit where the caller passes none.  The reference's frame there is AiBuildLocalFramePolar's (closed: an
// input wherever this library takes a frame); this stand-in is the first axis of Duff et al.'s branchless basis about N (as
// cone_make builds its own), in plain IEEE operations, the same in both math modes:
//     sg = copysign(1, N.z), a = -1 / (sg + N.z), T = (1 + sg N.x N.x a, sg (N.x N.y a), -sg N.x)
__device__ __forceinline__ V3 hit_tangent(V3 N)
{
    const float sg = __builtin_copysignf(1.0f, N.z);
    const float a = -1.0f / (sg + N.z);
    const float b = N.x * N.y * a;
    return mk(1.0f + sg * N.x * N.x * a, sg * b, -sg * N.x);
}

// Step 1.  Per tile of the probe emit's shape the points' maxRadius, shading normal and position go to LDS, one thread a point
// (the gate reads no more of the profile and the frame); then each thread takes rays threadIdx.x, + kBlock, ... of the tile.
template <int FAST_MATH = RLS_FAST>
__global__ __launch_bounds__(rlsh::kBlock) void sss_hits_gate_kernel(HitGateIO a)
{
    __shared__ float pt[7][kSssEmitPoints];      // maxR, No[3], Po[3]
    stage_libm_tables();
    const int P = a.tile_points, t = (int)threadIdx.x;
    const int64_t tiles = (a.n + P - 1) / P;
    const rls_probe_hits &h = a.h;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t p0 = tile * P;
        const int pc = a.n - p0 < P ? (int)(a.n - p0) : P;
        __syncthreads();                                         // the previous tile's points are consumed
        if (t < pc) {
            const int64_t i = p0 + t;
            const NdProfile p = scatter_profile(a.c, pindex(a.c.materials, i));
            const V3 No = ld3(a.c.N, i), Po = ld3(a.P, i);
            pt[0][t] = p.maxR;
            pt[1][t] = No.x; pt[2][t] = No.y; pt[3][t] = No.z;
            pt[4][t] = Po.x; pt[5][t] = Po.y; pt[6][t] = Po.z;
        }
        __syncthreads();
        for (int u = t; u < pc * a.spp; u += rlsh::kBlock) {
            const int lp = u / a.spp;
            const int64_t j = p0 * a.spp + u;
            const float maxR = pt[0][lp];
            const V3 No = mk(pt[1][lp], pt[2][lp], pt[3][lp]), Po = mk(pt[4][lp], pt[5][lp], pt[6][lp]);
            const int cnt = h.count[j] < h.max_hits ? (int)h.count[j] : h.max_hits;
            V3 prev = Po;
            uint32_t mask = 0;
            for (int k = 0; k < cnt; k++) {
                const int64_t at = (int64_t)k * h.stride + j;
                V3 d;
                float r, fade;
                if (probe_hit_shaded(prev, Po, ld3(h.P, at), ld3(h.N, at), maxR, No, a.cavity != 0, d, r, fade)) mask |= 1u << k;
            }
            a.mask[j] = (uint16_t)mask;
            a.count[j] = __builtin_popcount(mask);
        }
    }
}

#if !RLS_FAST
// Step 3: the listed prefix of the shaded hits, and their true number
__global__ __launch_bounds__(rlsh::kBlock) void sss_hits_list_kernel(HitListIO a)
{
    static_assert(RLS_MAX_PROBE_HITS <= 16, "a ray's shaded slots are a 16-bit mask");
    for (int64_t j = (int64_t)blockIdx.x * rlsh::kBlock + threadIdx.x; j < a.rays; j += (int64_t)gridDim.x * rlsh::kBlock) {
        int64_t at = a.offsets[j];
        for (uint32_t m = a.mask[j]; m != 0 && at < a.capacity; m &= m - 1, at++)
            a.hit_element[at] = (int64_t)__builtin_ctz(m) * a.stride + j;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.hit_count = a.offsets[a.rays];
}
#endif

// the light-sampling strategy's evaluation for the queued requests: ggx_light_eval_run's diffuse term (rls_loops.hpp; its
// lines, to be changed together) about the closure's own normal -- AiOrenNayarMISCreateData(sg, 0) has no view to offer, and
// at roughness 0 the lobe reads the view only to test its side.  VIEW: the caller has a view (rlSkin's diffuse rays' points).
// Whole wavefront.
template <int K, bool VIEW = false>
__device__ __forceinline__ void hit_light_eval_run(SlowLds<K> &Q, int cnt, const OrenNayar &on, V3 view, float conePdf, int mode)
{
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    wave_lds_fence();
    for (int base = 0; base < cnt; base += 64) {
        const int j = base + lane;
        const bool have = j < cnt;
        V3 L = mk(0.0f, 0.0f, 1.0f);
        int src = lane;
        if (have) { L = mk(Q.q[wave][0][j], Q.q[wave][1][j], Q.q[wave][2][j]); src = __float_as_int(Q.q[wave][3][j]) & 63; }
        OrenNayar o;                                            // every lane executes the fetches
        o.N = lane_fetch(on.N, src); o.A = lane_fetch(on.A, src); o.B = lane_fetch(on.B, src);
        const float cp = lane_fetch(conePdf, src);
        V3 wo = o.N;
        if constexpr (VIEW) wo = lane_fetch(view, src);
        if (have) {
            const float fd = oren_nayar_brdf(o, wo, L);
            const float wd = mode == RLS_MIS_LIGHT_ONLY ? 1.0f : power_heuristic(cp, oren_nayar_pdf(o, L));
            Q.q[wave][3][j] = R_DIV(fd * wd, cp);
        }
    }
    wave_lds_fence();
}

// Step 4.  evalLightSample's loop at list entry i, hit element e = hit_element[i]: ggx_direct_emit_kernel's walk with the
// Oren-Nayar closure alone (oren_nayar_make(N_hit, 0), the view along N_hit), the frame (N_hit, T_hit), the samples of
// hash(seed, first + e): segment 0 the light strategy, segment 1 the BSDF strategy, no specular segment.  Then, by the group's
// first lane, integrateDiffuse's ray: the first point of the scrambled (0,2) sequence at stream pair 24 (kNodeStream).
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void sss_hits_emit_kernel(HitEmitIO a)
{
    constexpr int K = RLS_SPEC_BLOCK;
    constexpr int SEGS = kSkinShadowSegments;
    __shared__ uint32_t tab[2][kMaxSpp];
    __shared__ SlowLds<K> slow;
    stage_libm_tables();
    stage_table(tab, a.spp);
    const int64_t count = *a.hit_count, listed = count < a.n ? count : a.n;
    RLS_POINT_WALK(G, a.n)
    const int spp = a.spp, tid = (int)threadIdx.x;
    const float zero[3] = { 0.0f, 0.0f, 0.0f };
    for (int64_t it = 0, i = first; it < rounds; it++, i += stride) {
        const bool live = i < listed;
        if (!live && i < a.n && sub == 0) {                     // past the list's end: no rays
            if (a.count) a.count[i] = 0;
            if (a.dtag) { a.dtag[i] = kDropped; a.dcount[i] = 0; }
        }
        if (__builtin_amdgcn_ballot_w64(live) == 0) continue;   // (wave-uniform: what follows has ballots and shuffles only)
        const int64_t e = live ? a.hit_element[i] : 0;
        V3 N = mk(0.0f, 0.0f, 1.0f), P = mk(0.0f, 0.0f, 0.0f), T = mk(1.0f, 0.0f, 0.0f);
        if (live) {
            N = ld3(a.h.N, e); P = ld3(a.h.P, e);
            T = a.T.x ? ld3(a.T, e) : hit_tangent(N);
        }
        Frame fr;
        fr.N = N; fr.U = T; fr.V = cross(N, T);
        const OrenNayar on = oren_nayar_make(N, 0.0f);           // AiOrenNayarMISCreateData(sg, 0.0f), :443
        constexpr bool kView = false;
        const V3 view = N;
        const uint64_t index = a.first + (uint64_t)e;
        ShadowStage<G, HitEmitIO, SEGS> st = { a, i, live, sub, 0, 0 };
#include "rls_trace_body_hit_light_loop.hpp"
        if (live && sub == 0) {
            if (a.count) a.count[i] = st.run;
            if (a.dtag) {
                // integrateDiffuse, :471-477: one cosine-weighted ray about the hit's normal, weight CLAMP(N . dir, 0, 1)
                const float rx = bits_u01(tab[0][0] ^ hash_u32(a.seed, index, kScrambleStream + kNodeStream));
                const float ry = bits_u01(tab[1][0] ^ hash_u32(a.seed, index, kScrambleStream + kNodeStream + 1));
                const V3 dir = cosine_hemisphere(fr, rx, ry);
                const float w = clampf(dot(N, dir), 0.0f, 1.0f);
                const bool keep = !(w == 0.0f);
                if (keep) {
                    a.ddir[0][i] = dir.x; a.ddir[1][i] = dir.y; a.ddir[2][i] = dir.z;
                    a.dw[i] = w;
                }
                a.dtag[i] = staging_tag(keep, 0, 0);
                a.dcount[i] = keep ? 1 : 0;
            }
        }
    }
}

// integrateScatter at a diffuse ray's point (src/rlSss.h:172-186; rls_trace_skin_bounce_emit): the same light loop over POINTS
// -- the closure oren_nayar_make(N, 0), the frame (N, T), the samples of hash(seed, first + i) -- at the points whose ray state
// is a diffuse ray's (skin_gates) and whose sssWeight, as the probe emit left it, is not below AI_EPSILON, with the point's own
// view, whose side rlGgx's Oren-Nayar lobe tests (oren_nayar_brdf): the terms are those of rls_trace_ggx_direct_emit's diffuse
// lobe at roughness 0.  Every other point counts 0 and stages nothing, its tags included (hits_compact_kernel reads a point
// without rays as dropped).  Most wavefronts hold no such point: the gate is read before anything is built, and a wavefront
// without one goes on to its next round.
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void skin_diffuse_emit_kernel(SkinDiffuseEmitIO a)
{
    constexpr int K = RLS_SPEC_BLOCK;
    constexpr int SEGS = kSkinShadowSegments;
    __shared__ uint32_t tab[2][kMaxSpp];
    __shared__ SlowLds<K> slow;
    stage_libm_tables();
    stage_table(tab, a.spp);
    RLS_POINT_WALK(G, a.n)
    const int spp = a.spp, tid = (int)threadIdx.x;
    const float zero[3] = { 0.0f, 0.0f, 0.0f };
    for (int64_t it = 0, i = first; it < rounds; it++, i += stride) {
        bool live = false;
        V3 N = mk(0.0f, 0.0f, 1.0f), P = mk(0.0f, 0.0f, 0.0f), T = mk(1.0f, 0.0f, 0.0f), view = N;
        if (i < a.n) {
            live = skin_gates(a.st, i).sss_diffuse && !(a.sssWeight[i] < kEps);
            if (!live && sub == 0) a.count[i] = 0;
        }
        if (__builtin_amdgcn_ballot_w64(live) == 0) continue;   // (wave-uniform: what follows has ballots and shuffles only)
        if (live) { N = ld3(a.N, i); P = ld3(a.P, i); T = ld3(a.T, i); view = ld3(a.wo, i); }
        constexpr bool kView = true;
        Frame fr;
        fr.N = N; fr.U = T; fr.V = cross(N, T);
        const OrenNayar on = oren_nayar_make(N, 0.0f);           // AiOrenNayarMISCreateData(sg, 0.0f), src/rlSss.h:175
        const uint64_t index = a.first + (uint64_t)i;
        ShadowStage<G, SkinDiffuseEmitIO, SEGS> st = { a, i, live, sub, 0, 0 };
#include "rls_trace_body_hit_light_loop.hpp"
        if (live && sub == 0) a.count[i] = st.run;
    }
}

#if !RLS_FAST
// Step 6.  E = +0 at every element
__global__ __launch_bounds__(rlsh::kBlock) void sss_hits_fill_kernel(rls_rgb E, int64_t count)
{
    for (int64_t j = (int64_t)blockIdx.x * rlsh::kBlock + threadIdx.x; j < count; j += (int64_t)gridDim.x * rlsh::kBlock) {
        E.r[j] = 0.0f; E.g[j] = 0.0f; E.b[j] = 0.0f;
    }
}

// E at the listed hits: the light loop's diffuse sum over the lights as shadow_resolve_kernel<1> forms it ahead of rlGgx's tail
// (shadow_sums; black without lights), plus (radiance x weight) x AI_ONEOVERPI (:482) where the hit has a diffuse ray.
__global__ __launch_bounds__(rlsh::kBlock) void sss_hits_resolve_kernel(HitResolveIO a)
{
    __shared__ float prod[6][kShadowTile];
    __shared__ uint8_t kinds[kShadowTile];
    __shared__ float rad[RLS_MAX_LIGHTS][3];
    stage_radiance(rad, a.s);
    const int64_t count = *a.hit_count, listed = count < a.n ? count : a.n;
    for (int64_t p0 = (int64_t)blockIdx.x * rlsh::kBlock; p0 < listed; p0 += (int64_t)gridDim.x * rlsh::kBlock) {
        const int64_t i = p0 + threadIdx.x;
        float oS[3], oD[3] = { 0.0f, 0.0f, 0.0f };
        if (a.s.nl > 0) shadow_sums<1, false>(prod, kinds, rad, a.s, p0, oS, oD);
        if (i < listed) {
            if (a.doffsets) {
                const int64_t r = a.doffsets[i];
                if (a.doffsets[i + 1] > r) {
                    const float w = a.dw[r];
                    oD[0] += (a.L.r[r] * w) * kInvPi; oD[1] += (a.L.g[r] * w) * kInvPi; oD[2] += (a.L.b[r] * w) * kInvPi;
                }
            }
            const int64_t e = a.hit_element[i];
            a.E.r[e] = oD[0]; a.E.g[e] = oD[1]; a.E.b[e] = oD[2];
        }
    }
}
#endif
