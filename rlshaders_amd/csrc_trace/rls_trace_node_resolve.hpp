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
// (the Oren-Nayar loop's queue, which the bounce call's argument struct alone has)
template <bool STATE, class IO>
__device__ __forceinline__ const ShadowResolveIO &skin_diffuse_loop(const IO &a)
{
    if constexpr (STATE) return a.dif_s;
    else return a.sheen_s;
}
template <int FAST_MATH = RLS_FAST>
__global__ __launch_bounds__(rlsh::kBlock) void skin_node_resolve_kernel(SkinNodeResolveIO a)
{
    constexpr bool STATE = false;
#include "rls_trace_body_skin_node_resolve.hpp"
}
// STATE (rls_trace_skin_bounce_resolve): a FIFTH walk, over the Oren-Nayar loop's queue (shadow_sums<1, false>, as
// sss_hits_resolve_kernel forms its direct term) through the same store; per point the switches of shader_evaluate
// (bounce_gates): sheen = specular = +0 where !(Rr_gloss <= GI_glossy_depth); at a diffuse ray's point the probe hits are not
// read and sss = (sss_color * D) * sssWeight with D the loop's diffuse sum (src/rlSss.h:172-186).  integrateGlossy's Rr == 0
// switch is the emit's: a lobe without glossy rays sums to +0.  A shadow ray's point is +0 everywhere: its sssWeight is 0.
template <int FAST_MATH = RLS_FAST>
__global__ __launch_bounds__(rlsh::kBlock) void skin_bounce_resolve_kernel(SkinBounceResolveIO a)
{
    constexpr bool STATE = true;
#include "rls_trace_body_skin_node_resolve.hpp"
}
