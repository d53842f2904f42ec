// rls_trace_node_resolve.hpp -- the whole nodes' resolves (part of trace.hip, included there inside its anonymous namespace,
// after rls_trace_queue.hpp and rls_trace_probe.hpp): one launch per node (ggx_node_resolve_kernel,
// disney_node_resolve_kernel, skin_node_resolve_kernel) that walks every queue with the two resolves' tile walks (shadow_sums;
// ray_sums_about_reference, ray_sums' walk about a reference radiance) and composes the AOVs in registers.

#if !RLS_FAST
// The node resolves: one launch composes rls_ggx_shade's / rls_disney_shade's AOVs and sg->out.RGB.  A workgroup takes kBlock
// consecutive points and walks their contiguous ray range of each queue in turn -- the light loop's (shadow_sums), then each
// indirect loop's (ray_sums_about_reference) -- through ONE LDS store (the light loop's six product planes; a ray queue keeps
// its radiance and weight planes there), lane i keeping its point's sums in registers; then the composition of
// ggx_shade_kernel / disney_shade_kernel (csrc/shade.hip) line by line, with the traced sum S where they have
// (sum x inv) x env.  No per-queue sum goes to memory.  LDS: 25.1 KB a workgroup, as shadow_resolve_kernel: six workgroups
// (24 waves) a CU; the walks' LDS access patterns are the two existing kernels'.
// STATE (rls_trace_ggx_bounce_resolve): the same walks; per point the ray-depth switches of shader_evaluate (bounce_gates) shut
// a direct sum (o_D / o_S = +0), pick the refraction queue's factor (1 / spp on the traced branch, 1 on the one-ray branch)
// and, off a camera ray, leave the indirect AOVs 0 and out without them (src/rlGgx.cpp:280, 292, 307-323; src/rlGgx.h:210-222).
// A shadow ray's point is +0 everywhere.
__global__ __launch_bounds__(rlsh::kBlock) void ggx_node_resolve_kernel(GgxNodeResolveIO a)
{
    constexpr bool STATE = false;
#include "rls_trace_body_ggx_node_resolve.hpp"
}
__global__ __launch_bounds__(rlsh::kBlock) void ggx_bounce_resolve_kernel(GgxNodeResolveIO a)
{
    constexpr bool STATE = true;
#include "rls_trace_body_ggx_node_resolve.hpp"
}

// STATE (rls_trace_disney_bounce_resolve): on a diffuse or glossy ray the direct sums x indirectDiffuseScale /
// indirectSpecularScale, each product rounded before the sum that follows (src/rlDisney.cpp:706-711); off a camera ray the
// indirect AOVs are 0 and out is without them (:713-725) -- the queues' own gates (shouldTraceDiffuse / shouldTraceGlossy) are
// the emit's: a lobe without rays sums to 0.  A shadow ray's point is +0 everywhere.
__global__ __launch_bounds__(rlsh::kBlock) void disney_node_resolve_kernel(DisneyNodeResolveIO a)
{
    constexpr bool STATE = false;
#include "rls_trace_body_disney_node_resolve.hpp"
}
__global__ __launch_bounds__(rlsh::kBlock) void disney_bounce_resolve_kernel(DisneyNodeResolveIO a)
{
    constexpr bool STATE = true;
#include "rls_trace_body_disney_node_resolve.hpp"
}

// rls_trace_ray_state_advance: the state of the hits of a queue's rays.  Ray k leaves point[k] as a ray of `ray_type`: sg->Rr
// and the counter of its type grow by one (saturating at 255, the counters' range), the other counters are the parent's.
__global__ __launch_bounds__(rlsh::kBlock) void state_advance_kernel(StateAdvanceIO a)
{
    for (int64_t k = (int64_t)blockIdx.x * rlsh::kBlock + threadIdx.x; k < a.rays; k += (int64_t)gridDim.x * rlsh::kBlock) {
        const int64_t p = a.point[k];
        const int rt = a.ray_type;
        auto up = [](int v, bool grow) { return (uint8_t)(grow && v < 255 ? v + 1 : v); };
        a.child[0][k] = (uint8_t)rt;
        a.child[1][k] = up(a.parent.Rr[p], true);
        a.child[2][k] = up(a.parent.Rr_diff[p], (rt & RLS_RT_DIFFUSE) != 0);
        a.child[3][k] = up(a.parent.Rr_gloss[p], (rt & RLS_RT_GLOSSY) != 0);
        a.child[4][k] = up(a.parent.Rr_refr[p], (rt & RLS_RT_REFRACTED) != 0);
    }
}

// The node resolves as the EXISTING resolve kernels plus a compose pass (RLS_NODE_RESOLVE=separate; for measurement,
// tools/trace_bench.py): shadow_resolve_kernel leaves the direct AOVs, trace_resolve_kernel one PLAIN sum of radiance x weight
// per ray queue in that queue's AOV plane (refraction and the Oren-Nayar queue already x inv, the three-plane queues not), and
// these kernels turn the planes into the AOVs in place and add sg->out.RGB.  Not the default: a plain sum rounds a uniform
// radiance into every term, so this path does not return the analytic call's bits for env other than 1.
__global__ __launch_bounds__(rlsh::kBlock) void ggx_node_compose_kernel(GgxNodeResolveIO a)
{
    for (int64_t i = (int64_t)blockIdx.x * rlsh::kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * rlsh::kBlock) {
        const GgxTail t = ggx_tail(a.s.materials, a.s.sh, i, true);
        float kr, kg, kb;
        ldrgb(a.KsColor, pindex(a.s.materials, i), kr, kg, kb);
        float dD[3], dS[3], tx[3] = { 0.0f, 0.0f, 0.0f }, iD[3] = { 0.0f, 0.0f, 0.0f }, iS[3] = { 0.0f, 0.0f, 0.0f };
        float *const pd[3] = { a.s.dd.r, a.s.dd.g, a.s.dd.b }, *const ps[3] = { a.s.ds.r, a.s.ds.g, a.s.ds.b };
        float *const pt[3] = { a.refract.out.r, a.refract.out.g, a.refract.out.b };
        float *const pi[3] = { a.diffuse.out.r, a.diffuse.out.g, a.diffuse.out.b };
        float *const pg[3] = { a.glossy.out.r, a.glossy.out.g, a.glossy.out.b };
#pragma unroll
        for (int c = 0; c < 3; c++) {
            dD[c] = a.s.nl > 0 ? pd[c][i] : 0.0f * t.d[c];
            dS[c] = a.s.nl > 0 ? ps[c][i] : 0.0f * t.ks;
        }
        if (!color_is_small(t.t[0], t.t[1], t.t[2]))
            for (int c = 0; c < 3; c++) tx[c] = pt[c][i] * t.t[c];
        if (!color_is_small(t.d[0], t.d[1], t.d[2]))
            for (int c = 0; c < 3; c++) iD[c] = t.d[c] * pi[c][i];
        if (!color_is_small(kr, kg, kb))
            for (int c = 0; c < 3; c++) iS[c] = pg[c][i] * a.inv * t.ks;
#pragma unroll
        for (int c = 0; c < 3; c++) { pd[c][i] = dD[c]; ps[c][i] = dS[c]; pt[c][i] = tx[c]; pi[c][i] = iD[c]; pg[c][i] = iS[c]; }
        if (a.out.r) strgb(a.out, i, ((dD[0] + dS[0]) + tx[0]) + (iD[0] + iS[0]), ((dD[1] + dS[1]) + tx[1]) + (iD[1] + iS[1]),
                           ((dD[2] + dS[2]) + tx[2]) + (iD[2] + iS[2]));
    }
}

__global__ __launch_bounds__(rlsh::kBlock) void disney_node_compose_kernel(DisneyNodeResolveIO a)
{
    for (int64_t i = (int64_t)blockIdx.x * rlsh::kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * rlsh::kBlock) {
        float *const pd[3] = { a.s.dd.r, a.s.dd.g, a.s.dd.b }, *const ps[3] = { a.s.ds.r, a.s.ds.g, a.s.ds.b };
        float *const pi[3] = { a.diffuse.out.r, a.diffuse.out.g, a.diffuse.out.b };
        float *const pg[3] = { a.specular.out.r, a.specular.out.g, a.specular.out.b };
        float o[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float dD = a.s.nl > 0 ? pd[c][i] : 0.0f, dS = a.s.nl > 0 ? ps[c][i] : 0.0f;
            const float iD = pi[c][i] * a.inv, iS = pg[c][i] * a.inv;
            pd[c][i] = dD; ps[c][i] = dS; pi[c][i] = iD; pg[c][i] = iS;
            o[c] = (dD + dS) + (iD + iS);
        }
        if (a.out.r) strgb(a.out, i, o[0], o[1], o[2]);
    }
}
#endif

// rlSkin's node resolve: ONE launch composes rls_skin_integrate's three AOVs and sg->out.RGB (src/rlSkin.cpp:249-254).  A
// workgroup takes kBlock consecutive points and walks, through ONE LDS store, per lobe the light loop's queue (shadow_sums<0>)
// and the glossy queue (ray_sums_about_reference), then the points' probe rays in sub-tiles of tile_points points -- one thread
// per ray (scatter_ray_terms), then the point's own lane sums its rays (scatter_point_sums): sss_scatter_resolve_kernel's two
// steps -- and composes as skin_integrate_kernel does (csrc/shade.hip:61-63, 79-82, 95, 101).  Sums and products only, but for
// the scatter walk's profile and MIS arithmetic, which is per math mode: built in both units like sss_scatter_resolve_kernel.
// A point whose sssWeight is below AI_EPSILON has its hits left unread and sss = 0.  LDS: 37.9 KB a workgroup (the scatter
// terms, as sss_scatter_resolve_kernel; the light loop's product planes and a ray queue's planes lie in the same store): four
// workgroups (16 waves) a CU.
template <int FAST_MATH = RLS_FAST>
__global__ __launch_bounds__(rlsh::kBlock) void skin_node_resolve_kernel(SkinNodeResolveIO a)
{
    __shared__ float lds[RLS_MAX_PROBE_HITS * 3 * rlsh::kBlock];
    __shared__ uint8_t kinds[kShadowTile];
    __shared__ float rad[RLS_MAX_LIGHTS][3];
    __shared__ uint8_t slots[rlsh::kBlock];
    __shared__ uint8_t shaded[rlsh::kBlock];
    static_assert(RLS_MAX_PROBE_HITS * 3 * rlsh::kBlock >= 6 * kShadowTile, "the scatter terms' store holds the product planes");
    float (*prod)[kShadowTile] = (float (*)[kShadowTile])lds;
    float (*term)[3][rlsh::kBlock] = (float (*)[3][rlsh::kBlock])lds;
    stage_libm_tables();
    stage_radiance(rad, a.sheen_s);                              // (both lobes: the same lights)
    const int t = (int)threadIdx.x, P = a.tile_points;
    for (int64_t p0 = (int64_t)blockIdx.x * rlsh::kBlock; p0 < a.n; p0 += (int64_t)gridDim.x * rlsh::kBlock) {
        const int64_t i = p0 + t;
        float litA[3] = { 0.0f, 0.0f, 0.0f }, litB[3] = { 0.0f, 0.0f, 0.0f }, none[3], gA[3], gB[3];
        if (a.sheen_s.nl > 0) shadow_sums<0>(prod, kinds, rad, a.sheen_s, p0, litA, none);              // :193-198
        ray_sums_about_reference<3>(prod, a.sheen_g, p0, a.n, a.inv, gA);
        if (a.spec_s.nl > 0) shadow_sums<0>(prod, kinds, rad, a.spec_s, p0, litB, none);                // :217-222
        ray_sums_about_reference<3>(prod, a.spec_g, p0, a.n, a.inv, gB);
        // integrateScatter, :244-246
        const int bc = a.n - p0 < rlsh::kBlock ? (int)(a.n - p0) : rlsh::kBlock;
        float sc[3] = { 0.0f, 0.0f, 0.0f };
        for (int q0 = 0; q0 < bc; q0 += P) {
            const int pc = bc - q0 < P ? bc - q0 : P;
            __syncthreads();                                     // the store's previous contents are consumed
            if (t < pc * a.spp) {
                const int lp = t / a.spp;
                const int64_t pi = p0 + q0 + lp, j = (p0 + q0) * a.spp + t;
                const SkinNodeResolveIO al = RLS_INT_ARGS(a);
                if (al.sssWeight[pi] < kEps) {
                    slots[t] = 0; shaded[t] = 0;
                } else {
                    const rls_skin_closure &c = al.c;
                    const PIndex<int64_t> pk = pindex(c.materials, pi);
                    const float mult = ldp(c.sss_dist_multiplier, pk);
                    const NdProfile p = nd_make<true>(ldp(c.sss_scatter_dist[0], pk) * mult, ldp(c.sss_scatter_dist[1], pk) * mult,
                                                      ldp(c.sss_scatter_dist[2], pk) * mult);
                    const Frame fr = sss_frame(ld3(c.N, pi), ld3(c.T, pi), true);
                    scatter_ray_terms(term, slots, shaded, t, p, fr, ld3(al.P, pi), al.h, j, al.cavity != 0, al.literal != 0);
                }
            }
            __syncthreads();
            if (t >= q0 && t < q0 + pc) {
                float depth;
                scatter_point_sums(term, slots, shaded, (t - q0) * a.spp, a.spp, sc, depth);
            }
        }
        if (i < a.n) {
            const SkinNodeResolveIO al = RLS_INT_ARGS(a);
            const rls_skin_closure &c = al.c;
            const PIndex<int64_t> pk = pindex(c.materials, i);
            const float sheenWeight = ldp(c.sheen_weight, pk), specWeight = ldp(c.specular_weight, pk);
            const float sheenFresnel = al.sheenFresnel[i], specularFresnel = al.specularFresnel[i], sssWeight = al.sssWeight[i];
            float br, bg, bb;
            ldrgb(c.sss_color, pk, br, bg, bb);
            const float bc3[3] = { br, bg, bb };
            const float sw = specWeight * (1.0f - sheenFresnel);                      // :231
            float sh[3], sp[3], ss[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                sh[k] = (sheenWeight > kEps ? litA[k] + gA[k] : 0.0f) * sheenWeight;  // :191, :207
                sp[k] = (specWeight > kEps ? litB[k] + gB[k] : 0.0f) * sw;            // :214, :231
                ss[k] = sssWeight < kEps ? 0.0f : bc3[k] * sc[k] * a.inv * sssWeight; // :244-246
            }
            const rls_skin_integrate_out &o = al.o;
            strgb(o.sheen, i, sh[0], sh[1], sh[2]);
            strgb(o.specular, i, sp[0], sp[1], sp[2]);
            strgb(o.sss, i, ss[0], ss[1], ss[2]);
            if (o.out.r) strgb(o.out, i, sh[0] + sp[0] + ss[0], sh[1] + sp[1] + ss[1], sh[2] + sp[2] + ss[2]);   // :254
            if (o.sheenFresnel) stg(o.sheenFresnel, i, sheenFresnel);
            if (o.specularFresnel) stg(o.specularFresnel, i, specularFresnel);
            if (o.sssWeight) stg(o.sssWeight, i, sssWeight);
        }
    }
}
