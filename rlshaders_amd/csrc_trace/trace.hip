// trace.hip -- caller-traced rlGgx, rlDisney and rlSss integrators and light loops (include/rlshaders_amd_trace.h; the light
// loops: the section "The light loops" below): integrateGlossy and
// integrateRefract's traced branch (src/rlGgx.h:172-184, 228-244), rlDisney's integrateDiffuse / integrateGlossy
// (src/rlDisney.cpp:240-243, 279-283) cut where the reference traces, into an emit of every sample ray and a resolve of
// the radiance the caller traced for them; rlSss's integrateScatter (src/rlSss.h:167-280) into an emit of every probe ray
// (sss_probe_emit_kernel, a dense queue: no scan, no compaction) and a resolve of the hits the caller's probe walk
// reports (sss_scatter_resolve_kernel).
//
// Emit, three steps on the context's stream:
//   1. ggx_{glossy,refract}_emit_kernel, disney_{diffuse,specular}_emit_kernel: the sample loop of rls_ggx_integrate /
//      rls_ggx_integrate_refract / one lobe of rls_disney_integrate (one G-lane group per point, the same packed
//      sampling), each sample computed ONCE: its record goes to a fixed staging slot s * n + i (sample-major: the lanes of
//      a wavefront store to consecutive words) with a tag (its rank among the point's kept samples, or "dropped"), the
//      point's kept count to offsets[i].  A count pass and a write pass would run the sample arithmetic twice.
//   2. trace_scan_{block,totals,add}_kernel: offsets[0, n) scanned in place (exclusive), offsets[n] = the ray count.  A
//      multi-kernel scan (tiles, then the tile sums in one workgroup, then the add-back): no workgroup waits on another.
//   3. trace_compact_kernel: per tile of points, the kept records move from their staging slots to offsets[i] + rank,
//      transposed through LDS (staging rows in, the tile's contiguous queue range out).
// Steps 2 and 3 are the same for every closure (emit() below).  Every position is a function of the inputs: no atomics
// anywhere.
// The light loops' emit has the same three steps with a queue of its own (rls_shadow_queue): ggx_direct_emit_kernel /
// disney_direct_emit_kernel, the scan, shadow_compact_kernel; the host side shares the staging's carve (staging) and the
// launch of steps 1 and 2 (emit_and_scan) with the sample-ray emits.
//
// Resolve (trace_resolve_kernel): per point the sequential sum over its rays in queue order; the products
// radiance x weight of a tile of rays are formed with coalesced loads into LDS, then each lane adds its point's ones.  The
// glossy resolve serves the rlGgx glossy and both rlDisney queues.
//
// Whole nodes (rls_trace_*_shade_emit / _resolve; the section "Whole nodes" below): one emit kernel per queue of
// rls_ggx_shade / rls_disney_shade -- the lobes above at the node's stream pairs, behind the node's gates -- and one resolve
// launch per node (ggx_node_resolve_kernel, disney_node_resolve_kernel) that walks every queue with the two resolves' tile
// walks (shadow_sums; ray_sums_about_reference, ray_sums' walk about a reference radiance) and composes the AOVs in registers.
//
// Built twice like the closure units of librlshaders_amd.so (rlshaders_amd/build.py, build_trace_library): RLS_FAST=0
// carries the C ABI, the EXACT emit kernels and the mode-free scan / compact / resolve kernels; RLS_FAST=1 the FAST emit
// kernels behind hidden symbols.
#include <string.h>

#include "rls_trace_device.hpp"

namespace {

// One sample as a lobe's sample() leaves it: the ray's direction, its weights (refraction: w[0] only) and kind bits; all
// zero past spp.
struct EmitRay {
    V3 dir;
    float w[3];
    int kind;
};

// The emit of every closure: the sample loop of the integrator (one G-lane group per point, the same packed sampling) with
// each sample staged instead of summed (staging_slot, staging_tag), the point's kept count to offsets[i] and its side output.
// A lobe policy supplies the rest, per point:
//   Lobe(a, ii)              the closure at point ii
//   kStream                  its scramble streams: kScrambleStream + kStream, + kStream + 1
//   kGated, open             a node's gate (kGated): a point whose gate is shut (!open) draws nothing and queues nothing
//   kPush, push(...)         the first sweep of the packed rare branches (SlowLds), if it has one
//   kWeights, sample(...)    the per-sample term, in every lane of every round; returns whether the ray is queued
//   side(spp)                the point's side output, in every lane (group reductions)
template <int G, class Lobe, class IO>
__device__ __forceinline__ void emit_points(const IO &a)
{
    constexpr int K = RLS_SPEC_BLOCK;
    __shared__ uint32_t tab[2][kMaxSpp];
    __shared__ SlowLds<K> slow;                                  // (not allocated where no lobe code uses it)
    stage_libm_tables();
    stage_table(tab, a.spp);
    RLS_POINT_WALK(G, a.n)
    for (int64_t it = 0, i = first; it < rounds; it++, i += stride) {
        const bool live = i < a.n;
        const int64_t ii = live ? i : a.n - 1;
        Lobe lobe(a, ii);
        const uint32_t sx = hash_u32(a.seed, a.first + (uint64_t)ii, kScrambleStream + Lobe::kStream);
        const uint32_t sy = hash_u32(a.seed, a.first + (uint64_t)ii, kScrambleStream + Lobe::kStream + 1);
        int run = 0;
        bool open = true;
        if constexpr (Lobe::kGated) open = lobe.open;
        for (int s0 = sub; s0 - sub < a.spp; s0 += K * G) {      // the same trip count in every lane
            if constexpr (Lobe::kPush) {
                int cnt = 0;
#pragma unroll 1
                for (int k = 0; k < K; k++) {
                    const int s = s0 + k * G;
                    const int sc = s < a.spp ? s : 0;
                    lobe.push(slow, k, cnt, s < a.spp && open, bits_u01(tab[0][sc] ^ sx), bits_u01(tab[1][sc] ^ sy));
                }
                slow_run<K>(slow, cnt);
            }
#pragma unroll 1
            for (int k = 0; k < K; k++) {
                const int s = s0 + k * G;
                const bool in = s < a.spp, ok = in && open;
                float rx = 0.0f, ry = 0.0f;                             // a lobe without a push phase draws here
                if (!Lobe::kPush && ok) { rx = bits_u01(tab[0][s] ^ sx); ry = bits_u01(tab[1][s] ^ sy); }
                EmitRay r = {};
                const bool keep = lobe.sample(slow, k, ok, rx, ry, r) && ok;      // (sample() first: every lane runs it)
                const int rank = group_rank<G>(keep, sub, run);
                if (live && in) {
                    const int64_t slot = staging_slot(s, a.n, i);
                    if (keep) {
                        a.dir[0][slot] = r.dir.x; a.dir[1][slot] = r.dir.y; a.dir[2][slot] = r.dir.z;
#pragma unroll
                        for (int c = 0; c < Lobe::kWeights; c++) a.w[c][slot] = r.w[c];
                    }
                    a.tag[slot] = staging_tag(keep, rank, r.kind);
                }
            }
        }
        const float side = lobe.side(a.spp);
        if (live && sub == 0) {
            a.count[i] = run;
            if (a.side) stg(a.side, i, side);
        }
    }
}

// rlGgx, both emits: the closure, the VNDF sampler and its packed uniform-slope fallback (ggx_vndf_push / _pop)
struct GgxLobe {
    static constexpr int kStream = 0;
    static constexpr bool kPush = true;
    static constexpr bool kGated = false;
    Ggx g;
    VndfView w;
    GgxLobe() = default;                                         // (rlSkin's lobes build g and w themselves: SkinGlossy)
    __device__ GgxLobe(const EmitIO<rls_ggx_closure> &a, int64_t ii)
    {
        RLS_GGX_LOAD(loaded, a.c, ii)
        g = loaded;
        w = vndf_view(g.view, g.fr, g.ax, g.ay);
    }
    template <int K>
    __device__ void push(SlowLds<K> &slow, int k, int &cnt, bool ok, float rx, float ry)
    {
        ggx_vndf_push<K>(slow, k, cnt, ok, w, rx, ry);
    }
};

// ggx_glossy_loop (rls_loops.hpp): f / pdf in three planes, queued where not all three are 0; the Fresnel sum folded in
// sample order exactly as there
template <int G>
struct GgxGlossy : GgxLobe {
    static constexpr int kWeights = 3;
    float accF = 0.0f;
    using GgxLobe::GgxLobe;
    template <int K>
    __device__ bool sample(const SlowLds<K> &slow, int k, bool ok, float, float, EmitRay &r)
    {
        float tF = 0.0f;
        if (ok) {
            const V3 M = ggx_vndf_pop<K>(slow, k, w, g.fr);
            r.dir = reflect_direction(g.view, M);
            tF = ggx_fresnel(g, r.dir, M);                          // mReflectWeight, src/rlGgx.h:103
            float fr, fg, fb, pdf;
            ggx_eval_pdf<true, true>(g, r.dir, fr, fg, fb, pdf);
            r.w[0] = fr / pdf; r.w[1] = fg / pdf; r.w[2] = fb / pdf;
        }
        fold<G>(accF, tF);
        return !(r.w[0] == 0.0f && r.w[1] == 0.0f && r.w[2] == 0.0f);
    }
    __device__ float side(int spp) const { return accF / (float)spp; }      // getAvgReflectWeight, src/rlGgx.h:181-184
};

// ggx_refract_loop (rls_loops.hpp): the weight in one plane, queued where it is not 0; a total internal reflection is a
// mirror ray (kind RLS_RAY_TIR_MIRROR) and counts towards tir_fraction
template <int G>
struct GgxRefract : GgxLobe {
    static constexpr int kWeights = 1;
    float tir = 0.0f;
    using GgxLobe::GgxLobe;
    template <int K>
    __device__ bool sample(const SlowLds<K> &slow, int k, bool ok, float, float, EmitRay &r)
    {
        if (ok) {
            const V3 M = ggx_vndf_pop<K>(slow, k, w, g.fr);
            if (!ggx_refract(g, M, r.dir)) { tir += 1.0f; r.kind = RLS_RAY_TIR_MIRROR; }
            r.w[0] = ggx_sample_weight(g, g.view, r.dir, M);         // src/rlGgx.h:241
        }
        return !(r.w[0] == 0.0f);
    }
    __device__ float side(int spp)
    {
        if (G > 1) tir = group_sum<G>(tir);                          // a count: integers, any order
        return tir * (1.0f / (float)spp);                            // as ggx_refract_loop: tir *= inv
    }
};

// One lobe of rls_disney_integrate's sample loop (integrate.hip, disney_integrate_body): SPEC = 0 the diffuse lobe
// (scramble streams +0/1, no rare branches: no push phase, no SlowLds), SPEC = 1 the specular lobe (+2/3, its rare branches
// packed through SlowLds as there).  A sample is valid where pdf > 1e-4 (src/rlDisney.cpp:309) and queued where it is valid
// and f / pdf is not 0 in all three channels: what it would add to the integrator's sum is then not +0.  The side output is
// the lobe's valid count.
// STREAM: the lobe's first scramble stream; the node's loops draw from kNodeStream on (disney_shade_kernel).
template <int G, bool SPEC, int STREAM = (SPEC ? 2 : 0)>
struct DisneyLobe {
    static constexpr int kStream = STREAM;
    static constexpr bool kPush = SPEC;
    static constexpr bool kGated = false;
    static constexpr int kWeights = 3;
    Disney d;
    VndfView w;
    float valid = 0.0f;
    __device__ DisneyLobe(const EmitIO<rls_disney_closure> &a, int64_t ii)
    {
        const EmitIO<rls_disney_closure> al = RLS_INT_ARGS(a);      // the closure's planes re-read per point, as there
        const rls_disney_closure &c = al.c;
        const PIndex<int64_t> pk = pindex(c.materials, ii);
        V3 wo = ld3(c.wo, ii), N = ld3(c.N, ii), T = ld3(c.T, ii);
        float br, bg, bb;
        ldrgb(c.base_color, pk, br, bg, bb);
        float sc[10];
        sc[0] = ldp(c.subsurface, pk); sc[1] = ldp(c.metallic, pk); sc[2] = ldp(c.specular, pk);
        sc[3] = ldp(c.specular_tint, pk); sc[4] = ldp(c.roughness, pk); sc[5] = ldp(c.anisotropic, pk);
        sc[6] = ldp(c.sheen, pk); sc[7] = ldp(c.sheen_tint, pk); sc[8] = ldp(c.clearcoat, pk);
        sc[9] = ldp(c.clearcoat_gloss, pk);
        d = disney_make(wo, N, T, br, bg, bb, sc);
        disney_prepare(d);
        w = vndf_view(d.view, d.fr, d.ax, d.ay);
    }
    template <int K>
    __device__ void push(SlowLds<K> &slow, int k, int &cnt, bool ok, float rx, float ry)
    {
        disney_spec_push<K>(slow, k, cnt, ok, d, w, rx, ry);
    }
    template <int K>
    __device__ bool sample(const SlowLds<K> &slow, int k, bool ok, float rx, float ry, EmitRay &t)
    {
        if (ok) {
            float r, g, b, pdf;
            if constexpr (SPEC) {
                t.dir = disney_spec_pop<K>(slow, k, d, w);
                disney_eval_pdf<false, true, true>(d, t.dir, r, g, b, pdf);
            } else {
                t.dir = cosine_hemisphere(d.fr, rx, ry);
                disney_eval_pdf<true, true, true>(d, t.dir, r, g, b, pdf);
            }
            if (pdf > kEps) { t.w[0] = r / pdf; t.w[1] = g / pdf; t.w[2] = b / pdf; valid += 1.0f; }
        }
        return !(t.w[0] == 0.0f && t.w[1] == 0.0f && t.w[2] == 0.0f);
    }
    __device__ float side(int)
    {
        if (G > 1) valid = group_sum<G>(valid);                      // a count: integers, any order
        return valid;
    }
};

template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void ggx_glossy_emit_kernel(EmitIO<rls_ggx_closure> a)
{
    emit_points<G, GgxGlossy<G>>(a);
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void ggx_refract_emit_kernel(EmitIO<rls_ggx_closure> a)
{
    emit_points<G, GgxRefract<G>>(a);
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void disney_diffuse_emit_kernel(EmitIO<rls_disney_closure> a)
{
    emit_points<G, DisneyLobe<G, false>>(a);
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void disney_specular_emit_kernel(EmitIO<rls_disney_closure> a)
{
    emit_points<G, DisneyLobe<G, true>>(a);
}

// ---------------------------------------------------------------------------------------------
// Whole nodes: the indirect loops of ggx_shade_kernel / disney_shade_kernel (csrc/shade.hip) as queues.  The lobes above with
// the node's stream pairs (kNodeStream: 24 glossy, 25 refraction, 26 Oren-Nayar for rlGgx; 24 diffuse, 25 specular for
// rlDisney) and, for rlGgx, the node's gates.  One emit kernel per queue: each builds the point's closure again.

// integrateGlossy as the node calls it: black for a small KsColor without sampling (src/rlGgx.h:174-176)
template <int G>
struct GgxNodeGlossy : GgxGlossy<G> {
    static constexpr int kStream = kNodeStream;
    static constexpr bool kGated = true;
    bool open;
    __device__ GgxNodeGlossy(const GgxNodeEmitIO &a, int64_t ii) : GgxGlossy<G>(a, ii)
    {
        float kr, kg, kb;
        ldrgb(a.c.KsColor, pindex(a.c.materials, ii), kr, kg, kb);
        open = !color_is_small(kr, kg, kb);
    }
};

// integrateRefract behind transmission's gate (src/rlGgx.cpp:307-309).  traced: ggx_refract_loop's samples; else the host
// launches with one sample per point, and that sample is ggx_refract_untraced's ray (rls_loops.hpp): the refraction about the
// shading normal, eta2 * |N . dir|, nothing on total internal reflection.
template <int G>
struct GgxNodeRefract : GgxRefract<G> {
    static constexpr int kStream = kNodeStream + 2;
    static constexpr bool kGated = true;
    bool open, traced;
    __device__ GgxNodeRefract(const GgxNodeEmitIO &a, int64_t ii) : GgxRefract<G>(a, ii)
    {
        const PIndex<int64_t> pk = pindex(a.c.materials, ii);
        const float kt = ldp(a.sh.Kt, pk);
        float tr, tg, tb;
        ldrgb(a.sh.KtColor, pk, tr, tg, tb);
        open = !color_is_small(tr * kt, tg * kt, tb * kt);
        traced = a.traced != 0;
    }
    template <int K>
    __device__ void push(SlowLds<K> &slow, int k, int &cnt, bool ok, float rx, float ry)
    {
        GgxLobe::template push<K>(slow, k, cnt, ok && traced, rx, ry);
    }
    template <int K>
    __device__ bool sample(const SlowLds<K> &slow, int k, bool ok, float rx, float ry, EmitRay &r)
    {
        if (traced) return GgxRefract<G>::template sample<K>(slow, k, ok, rx, ry, r);
        const Ggx &g = this->g;
        if (ok && ggx_refract(g, g.fr.N, r.dir)) r.w[0] = g.eta2 * absf(dot(g.fr.N, r.dir));      // src/rlGgx.h:216
        return !(r.w[0] == 0.0f);
    }
};

// the indirect diffuse loop of ggx_shade_kernel (src/rlGgx.cpp:315-319): cosine-weighted directions about the shading
// normal, brdf / pdf of the Oren-Nayar closure where pdf > 0, in one plane; queued where it is not 0
template <int G>
struct GgxNodeDiffuse {
    static constexpr int kStream = kNodeStream + 4;
    static constexpr bool kPush = false;
    static constexpr bool kGated = true;
    static constexpr int kWeights = 1;
    Frame fr;
    OrenNayar on;
    V3 view;
    bool open;
    __device__ GgxNodeDiffuse(const GgxNodeEmitIO &a, int64_t ii)
    {
        RLS_GGX_LOAD(g, a.c, ii)
        fr = g.fr;
        view = wo;
        on = oren_nayar_make(N, ldp(a.sh.diffuseRoughness, pk));
        const float kd = ldp(a.sh.Kd, pk);
        float dr, dg, db;
        ldrgb(a.sh.KdColor, pk, dr, dg, db);
        open = !color_is_small(dr * kd, dg * kd, db * kd);          // sampleDiffuse, src/rlGgx.cpp:279-281
    }
    template <int K>
    __device__ bool sample(const SlowLds<K> &, int, bool ok, float rx, float ry, EmitRay &r)
    {
        if (ok) {
            r.dir = cosine_hemisphere(fr, rx, ry);
            const float pd = oren_nayar_pdf(on, r.dir);
            if (pd > 0.0f) r.w[0] = R_DIV(oren_nayar_brdf(on, view, r.dir), pd);
        }
        return !(r.w[0] == 0.0f);
    }
    __device__ float side(int) const { return 0.0f; }
};

template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void ggx_node_glossy_emit_kernel(GgxNodeEmitIO a)
{
    emit_points<G, GgxNodeGlossy<G>>(a);
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void ggx_node_refract_emit_kernel(GgxNodeEmitIO a)
{
    emit_points<G, GgxNodeRefract<G>>(a);
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void ggx_node_diffuse_emit_kernel(GgxNodeEmitIO a)
{
    emit_points<G, GgxNodeDiffuse<G>>(a);
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void disney_node_diffuse_emit_kernel(EmitIO<rls_disney_closure> a)
{
    emit_points<G, DisneyLobe<G, false, kNodeStream>>(a);
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void disney_node_specular_emit_kernel(EmitIO<rls_disney_closure> a)
{
    emit_points<G, DisneyLobe<G, true, kNodeStream + 2>>(a);
}

// ---------------------------------------------------------------------------------------------
// The light loops: ggx_direct_loops / disney_direct_loops (rls_loops.hpp) with every term staged instead of folded.  Where
// they interleave the two lobes of the BSDF strategy in one pass over the samples, here each lobe is a pass of its own (the
// queue's segments 1 and 2), so that one running count ranks a point's rays in queue order:
//   segment 0 = the loops' first pass, the light strategy (RLS_LIGHT_SAMPLE_PUSH, *_light_eval_run, eval_pop);
//   segment 1 = the BSDF strategy's diffuse lobe: rlGgx's Oren-Nayar sample, rlDisney's packed cosine-weighted one;
//   segment 2 = the BSDF strategy's specular lobe (RLS_HIT_SAMPLE_EVAL, eval_pop).
// The two macros are the analytic loops' own lines (rls_loops.hpp).  Still written there and here, to be changed together
// (tests/test_gpu_trace_lights.py holds the copies together bit for bit): the pick-up sweeps after the evaluations, the
// Oren-Nayar sample, rlDisney's diffuse-lobe sweeps, and rlGgx's RLS_HIT_SAMPLE_EVAL lines, written out in ggx_direct_loops.
// The two kernels stay written out: with their common walk in a force-inlined shadow_emit_points<G, Node> (the argument
// struct by reference or by value, the segments as members of a node policy) rlDisney's kernel spilled 8 more vector
// registers at every G (scratch 56 -> 96 B at G = 1) and ran 0.8 % slower; rlDisney's body alone behind a force-inlined
// function taking the struct by reference went from 56 to 144 B.

// rlGgx's lobe for RLS_HIT_SAMPLE_EVAL: the VNDF sampler, the reflected direction (streams +2/3)
struct GgxHitLobe {
    const Ggx &g;
    const VndfView &w;
    V3 N;
    template <int K>
    RLS_DEV void push(SlowLds<K> &slow, int k, int &qn, bool ok, float rx, float ry) const { ggx_vndf_push<K>(slow, k, qn, ok, w, rx, ry); }
    template <int K>
    RLS_DEV V3 pop(const SlowLds<K> &slow, int k) const { return reflect_direction(g.view, ggx_vndf_pop<K>(slow, k, w, g.fr)); }
    RLS_DEV bool hit(V3 L) const { return !is_zero(L) && dot(L, N) > 0.0f; }
    template <int K>
    RLS_DEV void run(SlowLds<K> &slow, int qn, float conePdf, int mode) const { ggx_hit_eval_run<K>(slow, qn, g, conePdf, mode); }
};

// One point's place in the staging and its running ray count; SEGS: the segments of a light
template <int G, class IO, int SEGS = kShadowSegments>
struct ShadowStage {
    const IO &a;
    int64_t i;
    bool live;
    int sub, run;
    // sample s of segment `seg` of light l, in every lane of the wavefront (group_rank ballots): dir and the two lobes' terms
    // (zeros where the ray carries none); NWD: the planes of the diffuse term
    template <int NWD>
    __device__ __forceinline__ void put(const LightCone &cone, int l, int seg, int s, bool ok, V3 dir, const float (&ws)[3],
                                        const float (&wd)[3])
    {
        const bool bs = !(ws[0] == 0.0f && ws[1] == 0.0f && ws[2] == 0.0f);
        bool bd = !(wd[0] == 0.0f);
        if (NWD == 3) bd = !(wd[0] == 0.0f && wd[1] == 0.0f && wd[2] == 0.0f);
        const bool keep = ok && (bs || bd);
        const int rank = group_rank<G>(keep, sub, run);
        store<NWD>(cone, l, seg, s, ok, keep, rank, bs, bd, dir, ws, wd);
    }
    // rlSkin's light loops grow ONE sum per light, sample by sample, the light sample's term and then the BSDF sample's
    // (fold2 in ggx_light_loops): sample s's two rays, A the light-strategy one (segment 0) and B the BSDF-strategy one
    // (segment 1), ranked by a prefix count over the PAIRS of the point's earlier samples; A before B.  Specular terms only.
    __device__ __forceinline__ void put_pair(const LightCone &cone, int l, int s, bool ok, V3 dirA, const float (&wa)[3], V3 dirB,
                                             const float (&wb)[3])
    {
        const bool ka = ok && !(wa[0] == 0.0f && wa[1] == 0.0f && wa[2] == 0.0f);
        const bool kb = ok && !(wb[0] == 0.0f && wb[1] == 0.0f && wb[2] == 0.0f);
        const uint64_t ma = __builtin_amdgcn_ballot_w64(ka), mb = __builtin_amdgcn_ballot_w64(kb);
        const int base = (int)(threadIdx.x & 63u) & ~(G - 1);
        uint64_t ga = ma, gb = mb;
        if constexpr (G < 64) { ga = (ma >> base) & ((1ull << G) - 1ull); gb = (mb >> base) & ((1ull << G) - 1ull); }
        const uint64_t below = (1ull << sub) - 1ull;
        const int rankA = run + __builtin_popcountll(ga & below) + __builtin_popcountll(gb & below);
        const int rankB = rankA + (ka ? 1 : 0);
        run += __builtin_popcountll(ga) + __builtin_popcountll(gb);
        store<0>(cone, l, 0, s, ok, ka, rankA, true, false, dirA, wa, wa);
        store<0>(cone, l, 1, s, ok, kb, rankB, true, false, dirB, wb, wb);
    }
    template <int NWD>
    __device__ __forceinline__ void store(const LightCone &cone, int l, int seg, int s, bool ok, bool keep, int rank, bool bs,
                                          bool bd, V3 dir, const float (&ws)[3], const float (&wd)[3])
    {
        if (live && ok) {
            const int64_t slot = staging_slot((l * SEGS + seg) * a.spp + s, a.n, i);
            const IO al = RLS_INT_ARGS(a);                       // the staging planes' pointers re-read where they are used
            if (keep) {
                // the near intersection of P + t dir with the light's sphere: t^2 |dir|^2 - 2 b t + c2 = 0, in the form that
                // does not cancel; a light sample that rounding puts just outside the cone gets its closest approach
                const float b = dot(cone.d, dir), dd = dot(dir, dir);
                const float disc = maxf(0.0f, b * b - cone.c2 * dd);
                al.dir[0][slot] = dir.x; al.dir[1][slot] = dir.y; al.dir[2][slot] = dir.z;
                al.maxdist[slot] = R_DIV(cone.c2, b + R_SQRT(disc));
#pragma unroll
                for (int c = 0; c < 3; c++) al.ws[c][slot] = ws[c];
                if constexpr (NWD > 0) {
#pragma unroll
                    for (int c = 0; c < NWD; c++) al.wd[c][slot] = wd[c];
                }
            }
            const int kind = l | (seg ? RLS_SHADOW_BSDF : 0) | (bs ? RLS_SHADOW_SPECULAR : 0) | (bd ? RLS_SHADOW_DIFFUSE : 0);
            al.tag[slot] = shadow_tag(keep, rank, kind);
        }
    }
    // a segment the light's mis_mode skips: every slot dropped
    __device__ __forceinline__ void skip(int l, int seg)
    {
        if (!live) return;
        for (int s = sub; s < a.spp; s += G)
            a.tag[staging_slot((l * SEGS + seg) * a.spp + s, a.n, i)] = kShadowDropped;
    }
};

template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void ggx_direct_emit_kernel(ShadowEmitIO<rls_ggx_closure, rls_ggx_shader> a)
{
    constexpr int K = RLS_SPEC_BLOCK;
    __shared__ uint32_t tab[2][kMaxSpp];
    __shared__ SlowLds<K> slow;
    stage_libm_tables();
    stage_table(tab, a.spp);
    RLS_POINT_WALK(G, a.n)
    const int spp = a.spp, tid = (int)threadIdx.x;
    const float zero[3] = { 0.0f, 0.0f, 0.0f };
    for (int64_t it = 0, i = first; it < rounds; it++, i += stride) {
        const bool live = i < a.n;
        const int64_t ii = live ? i : a.n - 1;
        RLS_GGX_LOAD(g, a.c, ii)
        const VndfView w = vndf_view(g.view, g.fr, g.ax, g.ay);
        const OrenNayar on = oren_nayar_make(N, ldp(a.sh.diffuseRoughness, pk));
        const float kd = ldp(a.sh.Kd, pk);
        float dr, dg, db;
        ldrgb(a.sh.KdColor, pk, dr, dg, db);
        const bool sampleDiffuse = !color_is_small(dr * kd, dg * kd, db * kd);      // src/rlGgx.cpp:279-281
        const V3 P = ld3(a.P, ii);
        const uint64_t index = a.first + (uint64_t)ii;
        ShadowStage<G, decltype(a)> st = { a, i, live, sub, 0 };
        for (int l = 0; l < a.nl; l++) {
            const LightRegs lt = light_regs(a.lights[l], P);
            const LightCone &cone = lt.cone;
            const int mode = lt.mode;
            uint32_t scr[6];
#pragma unroll
            for (int k = 0; k < 6; k++) scr[k] = hash_u32(a.seed, index, kScrambleStream + 6 * l + k);

            // segment 0: one light sample, both lobes
            if (mode == RLS_MIS_BSDF_ONLY) st.skip(l, 0);
            for (int s0 = sub; mode != RLS_MIS_BSDF_ONLY && s0 - sub < spp; s0 += K * G) {
                RLS_LIGHT_SAMPLE_PUSH(slow, qn, tab, spp, s0, cone, N, scr[0], scr[1],
                                      slow.st[0][k][tid] = L.x; slow.st[1][k][tid] = L.y; slow.st[2][k][tid] = L.z;)
                ggx_light_eval_run<K>(slow, qn, g, on, cone.pdf, sampleDiffuse, mode);
#pragma unroll 1
                for (int k = 0; k < K; k++) {
                    float t[4], us[3] = { 0.0f, 0.0f, 0.0f }, ud[3] = { 0.0f, 0.0f, 0.0f };
                    if (eval_pop<K>(slow, k, t)) {
                        us[0] = t[0]; us[1] = t[1]; us[2] = t[2];
                        if (sampleDiffuse) ud[0] = t[3];
                    }
                    const V3 L = mk(slow.st[0][k][tid], slow.st[1][k][tid], slow.st[2][k][tid]);
                    st.template put<1>(cone, l, 0, s0 + k * G, s0 + k * G < spp, L, us, ud);
                }
            }
            // segment 1: one BSDF sample of the Oren-Nayar lobe (streams +4/5), where it hits the light
            if (mode == RLS_MIS_LIGHT_ONLY) st.skip(l, 1);
            for (int s0 = sub; mode != RLS_MIS_LIGHT_ONLY && s0 - sub < spp; s0 += G) {
                const int s = s0;
                float ud[3] = { 0.0f, 0.0f, 0.0f };
                V3 Ld = mk(0.0f, 0.0f, 0.0f);
                if (s < spp && cone.valid && sampleDiffuse) {
                    const float rx = bits_u01(tab[0][s] ^ scr[4]), ry = bits_u01(tab[1][s] ^ scr[5]);
                    Ld = cosine_hemisphere(g.fr, rx, ry);
                    const float pd = oren_nayar_pdf(on, Ld);
                    if (pd > 0.0f && cone_hit(cone, Ld)) {
                        const float fd = oren_nayar_brdf(on, wo, Ld);
                        const float wd = mode == RLS_MIS_BSDF_ONLY ? 1.0f : power_heuristic(pd, cone.pdf);
                        ud[0] = R_DIV(fd * wd, pd);
                    }
                }
                st.template put<1>(cone, l, 1, s, s < spp, Ld, zero, ud);
            }
            // segment 2: one BSDF sample of the GGX lobe (streams +2/3); the few that hit the light are evaluated packed
            if (mode == RLS_MIS_LIGHT_ONLY) st.skip(l, 2);
            for (int s0 = sub; mode != RLS_MIS_LIGHT_ONLY && s0 - sub < spp; s0 += K * G) {
                RLS_HIT_SAMPLE_EVAL(slow, (GgxHitLobe{ g, w, N }), tab, spp, s0, cone, scr[2], scr[3], mode)
#pragma unroll 1
                for (int k = 0; k < K; k++) {
                    const int s = s0 + k * G;
                    float t[4], us[3] = { 0.0f, 0.0f, 0.0f };
                    if (s < spp && cone.valid && eval_pop<K>(slow, k, t)) { us[0] = t[0]; us[1] = t[1]; us[2] = t[2]; }
                    const V3 L = mk(slow.st[0][k][tid], slow.st[1][k][tid], slow.st[2][k][tid]);
                    st.template put<1>(cone, l, 2, s, s < spp, L, us, zero);
                }
            }
        }
        if (live && sub == 0) a.count[i] = st.run;
    }
}

template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_DISNEY_LIGHT_ATTR void disney_direct_emit_kernel(ShadowEmitIO<rls_disney_closure, NoShader> a)
{
    constexpr int K = RLS_SPEC_BLOCK;
    __shared__ uint32_t tab[2][kMaxSpp];
    __shared__ SlowLds<K> slow;
    stage_libm_tables();
    stage_table(tab, a.spp);
    RLS_POINT_WALK(G, a.n)
    const int spp = a.spp, tid = (int)threadIdx.x;
    const float zero[3] = { 0.0f, 0.0f, 0.0f };
    for (int64_t it = 0, i = first; it < rounds; it++, i += stride) {
        const bool live = i < a.n;
        const int64_t ii = live ? i : a.n - 1;
        RLS_DISNEY_LOAD(d, a.c, ii)
        const VndfView w = vndf_view(d.view, d.fr, d.ax, d.ay);
        const V3 N = d.fr.N, P = ld3(a.P, ii);
        const uint64_t index = a.first + (uint64_t)ii;
        ShadowStage<G, decltype(a)> st = { a, i, live, sub, 0 };
        for (int l = 0; l < a.nl; l++) {
            const LightRegs lt = light_regs(a.lights[l], P);
            const LightCone &cone = lt.cone;
            const int mode = lt.mode;
            uint32_t scr[6];
#pragma unroll
            for (int k = 0; k < 6; k++) scr[k] = hash_u32(a.seed, index, kScrambleStream + 6 * l + k);

            // segment 0: one light sample, both lobes (the specular lobe's terms come back through st[0..2]: the direction
            // is drawn again in the second sweep)
            if (mode == RLS_MIS_BSDF_ONLY) st.skip(l, 0);
            for (int s0 = sub; mode != RLS_MIS_BSDF_ONLY && s0 - sub < spp; s0 += K * G) {
                RLS_LIGHT_SAMPLE_PUSH(slow, qn, tab, spp, s0, cone, N, scr[0], scr[1], )
                disney_light_eval_run<K>(slow, qn, d, cone.pdf, mode);
#pragma unroll 1
                for (int k = 0; k < K; k++) {
                    const int s = s0 + k * G;
                    const int sc = s < spp ? s : 0;
                    float t[4], us[3] = { 0.0f, 0.0f, 0.0f }, ud[3] = { 0.0f, 0.0f, 0.0f };
                    V3 L = mk(0.0f, 0.0f, 0.0f);
                    if (eval_pop<K>(slow, k, t)) {
                        ud[0] = t[0]; ud[1] = t[1]; ud[2] = t[2];
                        us[0] = slow.st[0][k][tid]; us[1] = slow.st[1][k][tid]; us[2] = slow.st[2][k][tid];
                        L = cone_sample(cone, bits_u01(tab[0][sc] ^ scr[0]), bits_u01(tab[1][sc] ^ scr[1]));
                    }
                    st.template put<3>(cone, l, 0, s, s < spp, L, us, ud);
                }
            }
            // segment 1: the diffuse lobe's BSDF samples (cosine-weighted, streams +2/3) that hit the light
            if (mode == RLS_MIS_LIGHT_ONLY) st.skip(l, 1);
            for (int s0 = sub; mode != RLS_MIS_LIGHT_ONLY && s0 - sub < spp; s0 += K * G) {
                int qn = 0;
#pragma unroll 1
                for (int k = 0; k < K; k++) {
                    const int s = s0 + k * G;
                    const int sc = s < spp ? s : 0;
                    const V3 L = cosine_hemisphere(d.fr, bits_u01(tab[0][sc] ^ scr[2]), bits_u01(tab[1][sc] ^ scr[3]));
                    eval_push<K>(slow, k, qn, s < spp && cone.valid && cone_hit(cone, L), L);
                    slow.st[0][k][tid] = L.x; slow.st[1][k][tid] = L.y; slow.st[2][k][tid] = L.z;
                }
                disney_hit_eval_run<K, true>(slow, qn, d, cone.pdf, mode);
#pragma unroll 1
                for (int k = 0; k < K; k++) {
                    float t[4], ud[3] = { 0.0f, 0.0f, 0.0f };
                    if (eval_pop<K>(slow, k, t) && t[3] != 0.0f) { ud[0] = t[0]; ud[1] = t[1]; ud[2] = t[2]; }
                    const V3 L = mk(slow.st[0][k][tid], slow.st[1][k][tid], slow.st[2][k][tid]);
                    st.template put<3>(cone, l, 1, s0 + k * G, s0 + k * G < spp, L, zero, ud);
                }
            }
            // segment 2: the specular lobe's BSDF samples (streams +4/5): the sampler's rare branches packed, then the
            // reflected directions that hit the light
            if (mode == RLS_MIS_LIGHT_ONLY) st.skip(l, 2);
            for (int s0 = sub; mode != RLS_MIS_LIGHT_ONLY && s0 - sub < spp; s0 += K * G) {
                RLS_HIT_SAMPLE_EVAL(slow, (DisneySpecHitLobe{ d, w }), tab, spp, s0, cone, scr[4], scr[5], mode)
#pragma unroll 1
                for (int k = 0; k < K; k++) {
                    float t[4], us[3] = { 0.0f, 0.0f, 0.0f };
                    if (eval_pop<K>(slow, k, t) && t[3] != 0.0f) { us[0] = t[0]; us[1] = t[1]; us[2] = t[2]; }
                    const V3 L = mk(slow.st[0][k][tid], slow.st[1][k][tid], slow.st[2][k][tid]);
                    st.template put<3>(cone, l, 2, s0 + k * G, s0 + k * G < spp, L, us, zero);
                }
            }
        }
        if (live && sub == 0) a.count[i] = st.run;
    }
}

// ---------------------------------------------------------------------------------------------
// rlSkin's node: shader_evaluate (src/rlSkin.cpp:174-254) as skin_integrate_kernel (csrc/shade.hip) runs it, cut at every place
// it traces.  Per GGX lobe (sheen, then specular) the light loop's shadow rays (skin_shadow_emit_kernel), then integrateGlossy's
// rays (skin_*_glossy_emit_kernel: GgxGlossy on the lobe's closure); then integrateScatter's probe rays
// (skin_probe_emit_kernel).  The mean Fresnel a layer hands down (getAvgReflectWeight, src/rlGgx.h:181-184) is ONE running
// float sum over the light loops' BSDF samples and then integrateGlossy's: the shadow emit leaves (sum, count) per point in
// two of the caller's three scalar planes -- the sum in the lobe's own Fresnel plane, the count in sssWeight -- the glossy emit
// starts its fold there and overwrites the Fresnel plane with avg * weight; the probe emit, last, writes sssWeight.  So the
// hand-over never lives in a queue's scratch, and the five queues may share one scratch block.

// One GGX lobe of the node at point ii, built as skin_integrate_kernel builds it (csrc/shade.hip:36-49, 66-69): both lobes share
// the frame and the local view; ggx_make<true>: no anisotropy.
struct SkinLobe {
    Ggx g;
    VndfView w;
    V3 N;
    float weight;
    bool small;              // integrateGlossy draws nothing (src/rlGgx.h:174-176); the light loop does
};
__device__ __forceinline__ SkinLobe skin_lobe(const rls_skin_closure &c, int64_t ii, int lobe)
{
    SkinLobe r;
    const PIndex<int64_t> pk = pindex(c.materials, ii);
    const V3 wo = ld3(c.wo, ii), N = ld3(c.N, ii), T = ld3(c.T, ii);
    Frame gfr;
    gfr.N = N; gfr.U = T; gfr.V = cross(N, T);
    const V3 local = vndf_local(wo, gfr);
    float cr, cg, cb, ior, rough;
    if (lobe == 0) {
        r.weight = ldp(c.sheen_weight, pk);
        ldrgb(c.sheen_color, pk, cr, cg, cb);
        ior = ldp(c.sheen_ior, pk); rough = ldp(c.sheen_roughness, pk);
    } else {
        r.weight = ldp(c.specular_weight, pk);
        ldrgb(c.specular_color, pk, cr, cg, cb);
        ior = ldp(c.specular_ior, pk); rough = ldp(c.specular_roughness, pk);
    }
    r.g = ggx_make<true>(wo, N, T, false, cr, cg, cb, ior, rough, 0.0f);
    r.w = vndf_view_from(local, r.g.ax, r.g.ay);
    r.N = N;
    r.small = absf(cr) < kEps && absf(cg) < kEps && absf(cb) < kEps;
    return r;
}

// A lobe's light loop: ggx_light_loops (rls_loops.hpp:447-495; its lines restated here, to be changed together --
// tests/test_gpu_trace_skin.py holds the copies together bit for bit) with both terms of a sample staged instead of folded
// into the light's one sum.  The Fresnel sum f grows over every BSDF sample of every light, in sample order (fold), cnt counts
// them; a lobe whose weight is <= AI_EPSILON (src/rlSkin.cpp:191, 214) or a light whose cone is not valid draws nothing.
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void skin_shadow_emit_kernel(SkinShadowEmitIO a)
{
    __shared__ uint32_t tab[2][kMaxSpp];
    stage_libm_tables();
    stage_table(tab, a.spp);
    RLS_POINT_WALK(G, a.n)
    const int spp = a.spp;
    const uint32_t stream = a.lobe ? 5u : 3u;
    for (int64_t it = 0, i = first; it < rounds; it++, i += stride) {
        const bool live = i < a.n;
        const int64_t ii = live ? i : a.n - 1;
        const SkinLobe sl = skin_lobe(a.c, ii, a.lobe);
        const Ggx &g = sl.g;
        const V3 N = sl.N, P = ld3(a.P, ii);
        const uint64_t index = a.first + (uint64_t)ii;
        ShadowStage<G, SkinShadowEmitIO, kSkinShadowSegments> st = { a, i, live, sub, 0 };
        float f = 0.0f, cnt = 0.0f;
        for (int l = 0; l < a.nl; l++) {
            const LightRegs lt = light_regs(a.lights[l], P);
            const LightCone &cone = lt.cone;
            const int mode = lt.mode;
            uint32_t scr[4];
#pragma unroll
            for (int k = 0; k < 4; k++) scr[k] = hash_u32(a.seed, index, kScrambleStream + 2 * (stream + 4 * l) + k);
            const bool draw = sl.weight > kEps && cone.valid;
            for (int s0 = 0; s0 < spp; s0 += G) {               // the same trip count in every lane (ballots, shuffles)
                const int s = s0 + sub;
                const bool ok = s < spp;
                float wa[3] = { 0.0f, 0.0f, 0.0f }, wb[3] = { 0.0f, 0.0f, 0.0f }, tF = 0.0f, tC = 0.0f;
                V3 La = mk(0.0f, 0.0f, 0.0f), Lb = mk(0.0f, 0.0f, 0.0f);
                if (draw && ok && mode != RLS_MIS_BSDF_ONLY) {
                    float rx = bits_u01(tab[0][s] ^ scr[0]), ry = bits_u01(tab[1][s] ^ scr[1]);
                    La = cone_sample(cone, rx, ry);
                    if (dot(La, N) > 0.0f) {
                        float fr, fg, fb, pb;
                        ggx_eval_pdf<true, true>(g, La, fr, fg, fb, pb);
                        float wgt = mode == RLS_MIS_LIGHT_ONLY ? 1.0f : power_heuristic(cone.pdf, pb);
                        wa[0] = R_DIV(fr * wgt, cone.pdf); wa[1] = R_DIV(fg * wgt, cone.pdf); wa[2] = R_DIV(fb * wgt, cone.pdf);
                    }
                }
                if (draw && ok && mode != RLS_MIS_LIGHT_ONLY) {
                    float rx = bits_u01(tab[0][s] ^ scr[2]), ry = bits_u01(tab[1][s] ^ scr[3]);
                    V3 M = vndf_microfacet(sl.w, g.fr, rx, ry);
                    Lb = reflect_direction(g.view, M);
                    tF = ggx_fresnel(g, Lb, M);                     // mReflectWeight += ..., mMisSampleCount += 1
                    tC = 1.0f;
                    if (!is_zero(Lb) && dot(Lb, N) > 0.0f && cone_hit(cone, Lb)) {
                        float fr, fg, fb, pb;
                        ggx_eval_pdf<true, true>(g, Lb, fr, fg, fb, pb);
                        float wgt = mode == RLS_MIS_BSDF_ONLY ? 1.0f : power_heuristic(pb, cone.pdf);
                        wb[0] = R_DIV(fr * wgt, pb); wb[1] = R_DIV(fg * wgt, pb); wb[2] = R_DIV(fb * wgt, pb);
                    }
                }
                st.put_pair(cone, l, s, ok, La, wa, Lb, wb);
                fold<G>(f, tF);
                cnt += G == 1 ? tC : group_sum<G>(tC);
            }
        }
        if (live && sub == 0) {
            a.count[i] = st.run;
            a.fsum[i] = f; a.fcnt[i] = cnt;
        }
    }
}

// A lobe's integrateGlossy (LOBE 0 sheen: stream pair 0; 1 specular: pair 1): GgxGlossy's rays on the lobe's closure, behind
// the lobe's gates -- no rays for a weight <= AI_EPSILON (:191, :214) or a small colour (src/rlGgx.h:174-176).  The Fresnel
// fold starts from the light loop's (sum, count); the side output is the layer's hand-down avg * weight (:204, :228): avg over
// the light loops' samples alone for a small colour, 1 when nothing was drawn, and the scalar 0 where the weight shuts the lobe.
template <int G, int LOBE>
struct SkinGlossy : GgxGlossy<G> {
    static constexpr int kStream = 2 * LOBE;
    static constexpr bool kGated = true;
    bool open, lobe_open;
    float weight, cnt = 0.0f;
    __device__ SkinGlossy(const SkinGlossyEmitIO &a, int64_t ii)
    {
        const SkinLobe sl = skin_lobe(a.c, ii, LOBE);
        this->g = sl.g; this->w = sl.w;
        weight = sl.weight;
        lobe_open = weight > kEps;
        open = lobe_open && !sl.small;
        if (a.fsum) { this->accF = a.fsum[ii]; cnt = a.fcnt[ii]; }
    }
    __device__ float side(int spp) const
    {
        if (!lobe_open) return 0.0f;
        const float fcnt = open ? cnt + (float)spp : cnt;
        const float avg = fcnt > 0.0f ? R_DIV(this->accF, fcnt) : 1.0f;
        return avg * weight;
    }
};
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void skin_sheen_glossy_emit_kernel(SkinGlossyEmitIO a)
{
    emit_points<G, SkinGlossy<G, 0>>(a);
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void skin_specular_glossy_emit_kernel(SkinGlossyEmitIO a)
{
    emit_points<G, SkinGlossy<G, 1>>(a);
}

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
    probe_emit_tiles<4>(a, [&](int64_t i, NdProfile &p, Frame &fr) {
        const rls_skin_closure &c = a.c;
        const PIndex<int64_t> pk = pindex(c.materials, i);
        const float mult = ldp(c.sss_dist_multiplier, pk);                            // :235-236
        float sssWeight = ldp(c.sss_weight, pk);
        sssWeight *= 1.0f - a.specularFresnel[i] * (1.0f - a.sheenFresnel[i]);        // :238
        a.sssWeight[i] = sssWeight;
        p = nd_make<true>(ldp(c.sss_scatter_dist[0], pk) * mult, ldp(c.sss_scatter_dist[1], pk) * mult,
                          ldp(c.sss_scatter_dist[2], pk) * mult);
        fr = sss_frame(ld3(c.N, i), ld3(c.T, i), true);
        return !(sssWeight < kEps);
    });
}

// integrateScatter's combination (src/rlSss.h:245-279) of the hits the caller traced.  Per tile: one thread per ray walks
// the ray's hits as scatter_loop walks the analytic ones -- duplicate test, radius cut-off, cavity fade, shaded count,
// evalProfile, the MIS pdf -- and leaves each hit's term irr / pdf (+0 for a skipped hit) in LDS; then one thread per point
// adds its rays' terms in sample order and, within a sample, in hit order: the order of the integrator's running sums.  The
// per-point profile and frame are recomputed per ray (the same arithmetic as the integrator's, so the same bits): staged in
// LDS instead, once per point, the kernel ran slower at 2^22 points x 16 rays (2.90 against 2.44 ms; 47 KB of LDS, three
// workgroups per CU instead of four).
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
        if (length(prev - hp) > kEps) {                                  // :316-317
            prev = hp;
            // shadeProbeSample, :379-420
            const V3 d = hp - Po;
            const float r = length(d);
            if (!(r > p.maxR)) {
                float fade = 1.0f;
                if (cavity) fade = sss_cavity_fade(d, r, hn, fr.N);
                if (fade > kEps) {
                    sh++;
                    float pr, pg, pb;
                    nd_profile(p, r, pr, pg, pb);
                    const float iR = eR * pr * fade, iG = eG * pg * fade, iB = eB * pb * fade;
                    if (!(iR == 0.0f && iG == 0.0f && iB == 0.0f)) {            // :249
                        const float pdf = sss_mis_pdf(p, fr, d, hn, literal);
                        tR = R_DIV(iR, pdf); tG = R_DIV(iG, pdf); tB = R_DIV(iB, pdf);
                    }
                }
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

#if !RLS_FAST
// exclusive scan of offsets[0, n): each workgroup one tile, its sum to totals[tile]
__global__ __launch_bounds__(rlsh::kBlock) void trace_scan_block_kernel(int64_t *v, int64_t n, int64_t *totals)
{
    const int64_t base = (int64_t)blockIdx.x * kScanTile;
    const int64_t count = n - base < kScanTile ? n - base : kScanTile;
    const int64_t total = scan_tile(v + base, count, 0);
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the tile sums, tile by tile with a carry; the grand total is the ray count, offsets[n]
__global__ __launch_bounds__(rlsh::kBlock) void trace_scan_totals_kernel(int64_t *totals, int64_t tiles, int64_t *ray_count)
{
    int64_t carry = 0;
    for (int64_t b = 0; b < tiles; b += kScanTile) {
        const int64_t count = tiles - b < kScanTile ? tiles - b : kScanTile;
        carry += scan_tile(totals + b, count, carry);
    }
    if (threadIdx.x == 0) *ray_count = carry;
}

__global__ __launch_bounds__(rlsh::kBlock) void trace_scan_add_kernel(int64_t *v, int64_t n, const int64_t *totals)
{
    for (int64_t j = (int64_t)blockIdx.x * rlsh::kBlock + threadIdx.x; j < n; j += (int64_t)gridDim.x * rlsh::kBlock)
        v[j] += totals[j / kScanTile];
}
#endif
// (What follows, down to the node resolves, is templates and inline device functions: the mode-free kernels among them are
// instantiated by the EXACT unit's host code alone; rlSkin's node resolve, built per math mode, uses the walks in both units.)

// A tile of P consecutive points (P * spp <= kCompactSlots): sample (i, s) moves from staging slot s * n + i to queue position
// offsets[i] + rank.  Through LDS, one plane at a time, so that both sides are coalesced: the staging is read in rows (one
// sample of P consecutive points), the tile's rays are one contiguous range of the queue and are written in order.
template <int NW>
__global__ __launch_bounds__(rlsh::kBlock) void trace_compact_kernel(TraceCompactIO a)
{
    constexpr int kPer = kCompactSlots / rlsh::kBlock;         // slots per thread: their loads are issued together
    __shared__ float buf[kCompactSlots];         // one plane of the tile's rays, in queue order
    __shared__ int64_t off[kCompactMaxPoints + 1];
    const rls_ray_queue &q = a.q;
    const int P = a.tile_points;
    const int64_t tiles = (a.n + P - 1) / P;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t p0 = tile * P;
        const int pc = a.n - p0 < P ? (int)(a.n - p0) : P;
        const int slots = pc * a.spp;
        __syncthreads();                                         // the previous tile is written out
        for (int p = threadIdx.x; p <= pc; p += rlsh::kBlock) off[p] = a.offsets[p0 + p];
        __syncthreads();
        const int64_t base = off[0];
        const int rays = (int)(off[pc] - base);
        // slot t = threadIdx.x + u * kBlock = s * pc + p: its staging index and position in the tile's range (-1: dropped)
        int64_t src_at[kPer];
        uint16_t tag[kPer];
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            const int t = (int)threadIdx.x + u * rlsh::kBlock, s = t / pc, p = t - s * pc;
            src_at[u] = staging_slot(s, a.n, p0) + p;
            tag[u] = t < slots ? a.tag[src_at[u]] : kDropped;
        }
        int pos[kPer];
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            const int t = (int)threadIdx.x + u * rlsh::kBlock, s = t / pc, p = t - s * pc;
            pos[u] = tag[u] == kDropped ? -1 : (int)(off[p] - base) + tag_rank(tag[u]);
        }
        for (int plane = 0; plane < 3 + NW; plane++) {
            const float *src = plane < 3 ? a.sdir[plane] : a.sw[plane - 3];
            float *out = plane == 0 ? q.dir.x : plane == 1 ? q.dir.y : plane == 2 ? q.dir.z
                       : plane == 3 ? q.weight.r : plane == 4 ? q.weight.g : q.weight.b;
            float v[kPer];
#pragma unroll
            for (int u = 0; u < kPer; u++) v[u] = pos[u] >= 0 ? src[src_at[u]] : 0.0f;
#pragma unroll
            for (int u = 0; u < kPer; u++) if (pos[u] >= 0) buf[pos[u]] = v[u];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kPer; u++) {
                const int k = (int)threadIdx.x + u * rlsh::kBlock;
                if (k < rays) out[base + k] = buf[k];
            }
            __syncthreads();
        }
        if (q.point || q.sample || q.kind) {
            uint32_t *ib = (uint32_t *)buf;
#pragma unroll
            for (int u = 0; u < kPer; u++) {
                const int t = (int)threadIdx.x + u * rlsh::kBlock, s = t / pc, p = t - s * pc;
                if (pos[u] >= 0) ib[pos[u]] = (uint32_t)p | (uint32_t)s << 8 | (uint32_t)tag_kind(tag[u]) << 16;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kPer; u++) {
                const int k = (int)threadIdx.x + u * rlsh::kBlock;
                if (k >= rays) continue;
                const uint32_t v = ib[k];
                if (q.point) q.point[base + k] = (uint32_t)(p0 + (v & 0xFF));
                if (q.sample) q.sample[base + k] = (uint8_t)(v >> 8);
                if (NW == 1 && q.kind) q.kind[base + k] = (uint8_t)(v >> 16);
            }
        }
    }
}

// per point the sum over its rays [offsets[i], offsets[i+1]) in queue order.  A workgroup takes kBlock consecutive points,
// i.e. one contiguous range of rays, in tiles of kResolveTile rays: coalesced loads form the products L x weight in LDS,
// then lane i adds those of its own rays, in order.
constexpr int kResolveTile = 1024;
// The tile walk over one ray queue for the workgroup's points p0 .. p0 + kBlock - 1 (trace_resolve_kernel and the node
// resolves): acc = the sum over this lane's point's rays of L x weight, in queue order.  Whole workgroup; the walk opens
// with a barrier, so prod may hold an earlier walk's products.  NW: the weight's planes.
template <int NW>
__device__ __forceinline__ void ray_sums(float (*prod)[kResolveTile], const TraceResolveIO &a, int64_t p0, int64_t n,
                                         float (&acc)[3])
{
    const int64_t i = p0 + threadIdx.x;
    const bool live = i < n;
    const int64_t pend = n - p0 < rlsh::kBlock ? n : p0 + rlsh::kBlock;
    const int64_t r0 = a.offsets[p0], r1 = a.offsets[pend];
    const int64_t lo = live ? a.offsets[i] : 0, hi = live ? a.offsets[i + 1] : 0;
    float aR = 0.0f, aG = 0.0f, aB = 0.0f;
    for (int64_t t0 = r0; t0 < r1; t0 += kResolveTile) {
        const int tn = r1 - t0 < kResolveTile ? (int)(r1 - t0) : kResolveTile;
        __syncthreads();                                     // the previous tile's products are consumed
        for (int k = threadIdx.x; k < tn; k += rlsh::kBlock) {
            const int64_t q = t0 + k;
            if (NW == 3) {
                prod[0][k] = a.L.r[q] * a.w[0][q]; prod[1][k] = a.L.g[q] * a.w[1][q]; prod[2][k] = a.L.b[q] * a.w[2][q];
            } else {
                const float wq = a.w[0][q];
                prod[0][k] = a.L.r[q] * wq; prod[1][k] = a.L.g[q] * wq; prod[2][k] = a.L.b[q] * wq;
            }
        }
        __syncthreads();
        const int64_t b = lo > t0 ? lo : t0, e = hi < t0 + tn ? hi : t0 + tn;
        for (int64_t q = b; q < e; q++) {
            aR += prod[0][q - t0]; aG += prod[1][q - t0]; aB += prod[2][q - t0];
        }
    }
    acc[0] = aR; acc[1] = aG; acc[2] = aB;
}

template <int NW>
__global__ __launch_bounds__(rlsh::kBlock) void trace_resolve_kernel(TraceResolveIO a)
{
    __shared__ float prod[3][kResolveTile];
    for (int64_t p0 = (int64_t)blockIdx.x * rlsh::kBlock; p0 < a.n; p0 += (int64_t)gridDim.x * rlsh::kBlock) {
        const int64_t i = p0 + threadIdx.x;
        float acc[3];
        ray_sums<NW>(prod, a, p0, a.n, acc);
        if (i < a.n) {
            if (NW == 1) { acc[0] *= a.scale; acc[1] *= a.scale; acc[2] *= a.scale; }
            a.out.r[i] = acc[0]; a.out.g[i] = acc[1]; a.out.b[i] = acc[2];
        }
    }
}

// The node resolves' walk over one ray queue: the sum over this lane's point's rays of L x weight, x inv, formed about a
// reference radiance so that a UNIFORM radiance gives the analytic call's bits.  Per channel, with Lref = the radiance of
// smallest magnitude among the point's rays (the first such in queue order; a property of the set of rays, not of their order):
//     A = sum w (in queue order: the analytic loop's sum),  B = sum (L - Lref) w,   S = (A inv) Lref + B inv
// In exact arithmetic S = inv sum L w.  Where every ray of the point carries the same radiance env, every term of B is
// exactly 0 -- also where a weight is infinite: a term whose L - Lref is 0 is skipped, which changes no finite sum (B is never
// -0) -- and S = (A inv) env: what ggx_shade_kernel / disney_shade_kernel form from their sum and env (csrc/shade.hip), for
// env = 1 and for any other.  Rounding: with k rays, |S - inv sum L w| <= (k + 3) 2^-24 inv (|Lref| sum |w| +
// sum |L - Lref| |w|); |Lref| <= |L| on every ray, so that is at most 3 (k + 3) 2^-24 inv sum |L| |w| (2 for radiances of one
// sign): a bound relative to the sum of the terms' magnitudes, as the plain sum's, whatever single ray is bright.
// Lref is found in a pass of its own over the lane's rays in global memory (they are read again, coalesced, by the tiles).
// The radiance and the weight of a tile go to LDS side by side (coalesced loads), lane i multiplies.
// planes: 3 + NW rows.  A point without rays: S = 0.
template <int NW>
__device__ __forceinline__ void ray_sums_about_reference(float (*planes)[kResolveTile], const TraceResolveIO &a, int64_t p0,
                                                         int64_t n, float inv, float (&S)[3])
{
    const int64_t i = p0 + threadIdx.x;
    const bool live = i < n;
    const int64_t pend = n - p0 < rlsh::kBlock ? n : p0 + rlsh::kBlock;
    const int64_t r0 = a.offsets[p0], r1 = a.offsets[pend];
    const int64_t lo = live ? a.offsets[i] : 0, hi = live ? a.offsets[i + 1] : 0;
    float ref[3] = { 0.0f, 0.0f, 0.0f };
    if (hi > lo) { ref[0] = a.L.r[lo]; ref[1] = a.L.g[lo]; ref[2] = a.L.b[lo]; }
    for (int64_t q = lo + 1; q < hi; q++) {
        const float v[3] = { a.L.r[q], a.L.g[q], a.L.b[q] };
#pragma unroll
        for (int c = 0; c < 3; c++) if (absf(v[c]) < absf(ref[c])) ref[c] = v[c];
    }
    float A[3] = { 0.0f, 0.0f, 0.0f }, B[3] = { 0.0f, 0.0f, 0.0f };
    for (int64_t t0 = r0; t0 < r1; t0 += kResolveTile) {
        const int tn = r1 - t0 < kResolveTile ? (int)(r1 - t0) : kResolveTile;
        __syncthreads();                                     // the previous tile is consumed
        for (int k = threadIdx.x; k < tn; k += rlsh::kBlock) {
            const int64_t q = t0 + k;
            planes[0][k] = a.L.r[q]; planes[1][k] = a.L.g[q]; planes[2][k] = a.L.b[q];
#pragma unroll
            for (int c = 0; c < NW; c++) planes[3 + c][k] = a.w[c][q];
        }
        __syncthreads();
        const int64_t b = lo > t0 ? lo : t0, e = hi < t0 + tn ? hi : t0 + tn;
        for (int64_t q = b; q < e; q++) {
            const int k = (int)(q - t0);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float w = planes[3 + (NW == 3 ? c : 0)][k];
                if (NW == 3 || c == 0) A[c] += w;
                // (a ray AT the reference adds nothing, whatever its weight: 0 x inf would be NaN where the analytic sum is inf.
                // That is all the skip guarantees -- the uniform radiance of the contract; under a non-uniform radiance an infinite
                // weight may still meet Lref = 0 in (A inv) Lref and give NaN where the plain sum is inf)
                const float d = planes[c][k] - ref[c];
                B[c] += d == 0.0f ? 0.0f : d * w;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) S[c] = (A[NW == 3 ? c : 0] * inv) * ref[c] + B[c] * inv;
}

// trace_compact_kernel for the light loops' queue: a tile of P consecutive points with a.slots slots each (P * slots <=
// kShadowMaxSlots; one point at the limits of 8 lights x 3 segments x 256 samples).  Slot t = sp * pc + p of the tile is slot sp
// of its point p: the staging is read in rows, the tile's rays are one contiguous range of the queue.  The positions are kept
// in LDS (a thread has up to 24 slots), the planes go through buf one at a time.  NWD: the planes of weight_diffuse.
// Limits of this shape: a staging row is pc points wide, so with many slots per point (tile_points = 6144 / slots: 64 at 2
// lights x 16 samples, 1 at the maximum) the tag and plane reads are short runs n words apart rather than full cache lines, and
// every plane's pass walks all the tile's slots (through pos), kept or not.
template <int NWD>
__global__ __launch_bounds__(rlsh::kBlock) void shadow_compact_kernel(ShadowCompactIO a)
{
    __shared__ float buf[kShadowMaxSlots];           // one plane of the tile's rays, in queue order
    __shared__ int16_t pos[kShadowMaxSlots];         // slot -> its ray's place in the tile's range, -1: dropped
    static_assert(kShadowMaxSlots <= 32767, "pos holds a slot's place in 16 bits");
    static_assert(kCompactMaxPoints <= 256 && kMaxSpp <= 256, "ib packs the point's index in the tile and the sample in 8 bits each");
    static_assert(kShadowMaxSlots <= 0x10000, "the tag's rank is 16 bits");
    __shared__ int64_t off[kCompactMaxPoints + 1];
    const rls_shadow_queue &q = a.q;
    const int P = a.tile_points;
    const int64_t tiles = (a.n + P - 1) / P;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t p0 = tile * P;
        const int pc = a.n - p0 < P ? (int)(a.n - p0) : P;
        const int slots = pc * a.slots;
        __syncthreads();                                         // the previous tile is written out
        for (int p = threadIdx.x; p <= pc; p += rlsh::kBlock) off[p] = a.offsets[p0 + p];
        __syncthreads();
        const int64_t base = off[0];
        const int rays = (int)(off[pc] - base);
        // (sp, p) of this thread's slots t = threadIdx.x, + kBlock, ...: advanced without a division per slot
        const int sp0 = (int)threadIdx.x / pc, pp0 = (int)threadIdx.x - sp0 * pc;
        const int dsp = rlsh::kBlock / pc, dp = rlsh::kBlock - dsp * pc;
        uint32_t *ib = (uint32_t *)buf;
        for (int t = threadIdx.x, sp = sp0, p = pp0; t < slots; t += rlsh::kBlock) {
            const uint32_t tag = a.tag[staging_slot(sp, a.n, p0 + p)];
            int at = -1;
            if (tag != kShadowDropped) {
                at = (int)(off[p] - base) + (int)(tag & 0xFFFFu);
                ib[at] = (uint32_t)p | (uint32_t)(sp % a.spp) << 8 | (tag >> 16) << 16;
            }
            pos[t] = (int16_t)at;
            sp += dsp; p += dp;
            if (p >= pc) { p -= pc; sp++; }
        }
        __syncthreads();
        for (int k = threadIdx.x; k < rays; k += rlsh::kBlock) {
            const uint32_t v = ib[k];
            q.kind[base + k] = (uint8_t)(v >> 16);
            if (q.point) q.point[base + k] = (uint32_t)(p0 + (v & 0xFF));
            if (q.sample) q.sample[base + k] = (uint8_t)(v >> 8);
        }
        for (int plane = 0; plane < 7 + NWD; plane++) {
            const float *src = a.src[plane];
            float *out = plane == 0 ? q.dir.x : plane == 1 ? q.dir.y : plane == 2 ? q.dir.z : plane == 3 ? q.maxdist
                       : plane == 4 ? q.weight_specular.r : plane == 5 ? q.weight_specular.g : plane == 6 ? q.weight_specular.b
                       : plane == 7 ? q.weight_diffuse.r : plane == 8 ? q.weight_diffuse.g : q.weight_diffuse.b;
            __syncthreads();                                     // buf's previous contents are written out
            for (int t = threadIdx.x, sp = sp0, p = pp0; t < slots; t += rlsh::kBlock) {
                const int at = pos[t];
                if (at >= 0) buf[at] = src[staging_slot(sp, a.n, p0 + p)];
                sp += dsp; p += dp;
                if (p >= pc) { p -= pc; sp++; }
            }
            __syncthreads();
            for (int k = threadIdx.x; k < rays; k += rlsh::kBlock) out[base + k] = buf[k];
        }
    }
}

// The light loops' sums with the traced visibility.  Like trace_resolve_kernel a workgroup takes kBlock consecutive points, one
// contiguous range of rays, in tiles: coalesced loads form visibility x weight of both lobes in LDS, then lane i walks its own
// point's rays in queue order -- lights ascending -- and keeps the analytic loop's four sums per light (light or BSDF strategy x
// lobe), closing a light with s = light_sum + bsdf_sum, t = (radiance * s) * inv, the first light assigning
// (ggx_direct_loops / disney_direct_loops, rls_loops.hpp).  A light without rays is closed too: it adds radiance * 0 * inv.
// NWD = 1 (rlGgx): weight_diffuse is one plane, and the tail diffuse *= KdColor * Kd, specular *= Ks follows (src/rlGgx.cpp:304-305).
constexpr int kShadowTile = 1024;
static_assert(kShadowTile == kResolveTile, "the node resolves walk both kinds of queue through one product store");

// the lights' radiance into LDS, once per workgroup (the walk below indexes it by a per-lane light)
__device__ __forceinline__ void stage_radiance(float (*rad)[3], const ShadowResolveIO &a)
{
    if (threadIdx.x < RLS_MAX_LIGHTS * 3) rad[threadIdx.x / 3][threadIdx.x % 3] = a.rad[threadIdx.x / 3][threadIdx.x % 3];
    __syncthreads();
}

// The tile walk over the light loops' queue for the workgroup's points p0 .. p0 + kBlock - 1 (shadow_resolve_kernel and the
// node resolves): oS / oD = the point's specular / diffuse sum over the lights, before rlGgx's tail.  Whole workgroup; opens
// with a barrier like ray_sums.
template <int NWD>
__device__ __forceinline__ void shadow_sums(float (*prod)[kShadowTile], uint8_t *kinds, const float (*rad)[3],
                                            const ShadowResolveIO &a, int64_t p0, float (&oS)[3], float (&oD)[3])
{
    // NWD = 0: a lobe of rlSkin (ggx_light_loops, rls_loops.hpp): no diffuse term, and ONE sum per light that takes the rays of
    // both strategies in queue order; the lights' terms are added to +0
    constexpr bool GGX = NWD == 1, ONE = NWD == 0;
    const int64_t i = p0 + threadIdx.x;
    const bool live = i < a.n;
    const int64_t pend = a.n - p0 < rlsh::kBlock ? a.n : p0 + rlsh::kBlock;
    const int64_t r0 = a.offsets[p0], r1 = a.offsets[pend];
    const int64_t lo = live ? a.offsets[i] : 0, hi = live ? a.offsets[i + 1] : 0;
    float lS[3] = { 0.0f, 0.0f, 0.0f }, lD[3] = { 0.0f, 0.0f, 0.0f }, bS[3] = { 0.0f, 0.0f, 0.0f }, bD[3] = { 0.0f, 0.0f, 0.0f };
    for (int c = 0; c < 3; c++) { oS[c] = 0.0f; oD[c] = 0.0f; }
    int l = 0;
    auto close_light = [&]() {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            // (ONE: bS stays +0, and a sum that starts at +0 is never -0: lS + bS is lS)
            const float tS = rad[l][c] * (lS[c] + bS[c]) * a.inv, tD = rad[l][c] * (lD[c] + bD[c]) * a.inv;
            oS[c] = l == 0 && !ONE ? tS : oS[c] + tS;
            oD[c] = l == 0 ? tD : oD[c] + tD;
            lS[c] = 0.0f; lD[c] = 0.0f; bS[c] = 0.0f; bD[c] = 0.0f;
        }
        l++;
    };
    for (int64_t t0 = r0; t0 < r1; t0 += kShadowTile) {
        const int tn = r1 - t0 < kShadowTile ? (int)(r1 - t0) : kShadowTile;
        __syncthreads();                                     // the previous tile's products are consumed
        for (int k = threadIdx.x; k < tn; k += rlsh::kBlock) {
            const int64_t r = t0 + k;
            const float vr = a.vis.r[r], vg = a.vis.g[r], vb = a.vis.b[r];
            prod[0][k] = vr * a.ws[0][r]; prod[1][k] = vg * a.ws[1][r]; prod[2][k] = vb * a.ws[2][r];
            if (GGX) {
                const float wd = a.wd[0][r];
                prod[3][k] = vr * wd; prod[4][k] = vg * wd; prod[5][k] = vb * wd;
            } else if (!ONE) {
                prod[3][k] = vr * a.wd[0][r]; prod[4][k] = vg * a.wd[1][r]; prod[5][k] = vb * a.wd[2][r];
            }
            kinds[k] = a.kind[r];
        }
        __syncthreads();
        const int64_t b = lo > t0 ? lo : t0, e = hi < t0 + tn ? hi : t0 + tn;
        for (int64_t r = b; r < e; r++) {
            const int k = (int)(r - t0), kind = kinds[k];
            const int lk = (kind & RLS_SHADOW_LIGHT_MASK) < a.nl ? (kind & RLS_SHADOW_LIGHT_MASK) : a.nl - 1;
            while (l < lk) close_light();
            if (ONE) {
                lS[0] += prod[0][k]; lS[1] += prod[1][k]; lS[2] += prod[2][k];
            } else if (kind & RLS_SHADOW_BSDF) {
                if (kind & RLS_SHADOW_SPECULAR) { bS[0] += prod[0][k]; bS[1] += prod[1][k]; bS[2] += prod[2][k]; }
                if (kind & RLS_SHADOW_DIFFUSE) { bD[0] += prod[3][k]; bD[1] += prod[4][k]; bD[2] += prod[5][k]; }
            } else {
                if (kind & RLS_SHADOW_SPECULAR) { lS[0] += prod[0][k]; lS[1] += prod[1][k]; lS[2] += prod[2][k]; }
                if (kind & RLS_SHADOW_DIFFUSE) { lD[0] += prod[3][k]; lD[1] += prod[4][k]; lD[2] += prod[5][k]; }
            }
        }
    }
    if (live) {
        while (l < a.nl) close_light();
    }
}

// rlGgx's node parameters at point i, as ggx_shade_kernel forms them (src/rlGgx.cpp:279, 308)
struct GgxTail { float ks, d[3], t[3]; };
__device__ __forceinline__ GgxTail ggx_tail(const rls_material_index &materials, const rls_ggx_shader &sh, int64_t i, bool kt)
{
    GgxTail r = {};
    const PIndex<int64_t> pk = pindex(materials, i);
    const float kd = ldp(sh.Kd, pk);
    r.ks = ldp(sh.Ks, pk);
    ldrgb(sh.KdColor, pk, r.d[0], r.d[1], r.d[2]);
    r.d[0] *= kd; r.d[1] *= kd; r.d[2] *= kd;                // diffuseColor, src/rlGgx.cpp:279
    if (kt) {
        const float k = ldp(sh.Kt, pk);
        ldrgb(sh.KtColor, pk, r.t[0], r.t[1], r.t[2]);
        r.t[0] *= k; r.t[1] *= k; r.t[2] *= k;               // ktColor, :308
    }
    return r;
}

template <int NWD>
__global__ __launch_bounds__(rlsh::kBlock) void shadow_resolve_kernel(ShadowResolveIO a)
{
    constexpr bool GGX = NWD == 1;
    __shared__ float prod[6][kShadowTile];           // visibility x weight_specular, visibility x weight_diffuse
    __shared__ uint8_t kinds[kShadowTile];
    __shared__ float rad[RLS_MAX_LIGHTS][3];
    stage_radiance(rad, a);
    for (int64_t p0 = (int64_t)blockIdx.x * rlsh::kBlock; p0 < a.n; p0 += (int64_t)gridDim.x * rlsh::kBlock) {
        const int64_t i = p0 + threadIdx.x;
        float oS[3], oD[3];
        shadow_sums<NWD>(prod, kinds, rad, a, p0, oS, oD);
        if (i < a.n) {
            if (GGX) {
                const GgxTail t = ggx_tail(a.materials, a.sh, i, false);
                strgb(a.ds, i, oS[0] * t.ks, oS[1] * t.ks, oS[2] * t.ks);
                strgb(a.dd, i, oD[0] * t.d[0], oD[1] * t.d[1], oD[2] * t.d[2]);
            } else {
                strgb(a.ds, i, oS[0], oS[1], oS[2]);
                strgb(a.dd, i, oD[0], oD[1], oD[2]);
            }
        }
    }
}

#if !RLS_FAST
// The node resolves: one launch composes rls_ggx_shade's / rls_disney_shade's AOVs and sg->out.RGB.  A workgroup takes kBlock
// consecutive points and walks their contiguous ray range of each queue in turn -- the light loop's (shadow_sums), then each
// indirect loop's (ray_sums_about_reference) -- through ONE LDS store (the light loop's six product planes; a ray queue keeps
// its radiance and weight planes there), lane i keeping its point's sums in registers; then the composition of
// ggx_shade_kernel / disney_shade_kernel (csrc/shade.hip) line by line, with the traced sum S where they have
// (sum x inv) x env.  No per-queue sum goes to memory.  LDS: 25.1 KB a workgroup, as shadow_resolve_kernel: six workgroups
// (24 waves) a CU; the walks' LDS access patterns are the two existing kernels'.
__global__ __launch_bounds__(rlsh::kBlock) void ggx_node_resolve_kernel(GgxNodeResolveIO a)
{
    __shared__ float prod[6][kShadowTile];
    __shared__ uint8_t kinds[kShadowTile];
    __shared__ float rad[RLS_MAX_LIGHTS][3];
    stage_radiance(rad, a.s);
    for (int64_t p0 = (int64_t)blockIdx.x * rlsh::kBlock; p0 < a.n; p0 += (int64_t)gridDim.x * rlsh::kBlock) {
        const int64_t i = p0 + threadIdx.x;
        float oS[3] = { 0.0f, 0.0f, 0.0f }, oD[3] = { 0.0f, 0.0f, 0.0f }, sG[3], sT[3], sD[3];
        if (a.s.nl > 0) shadow_sums<1>(prod, kinds, rad, a.s, p0, oS, oD);
        ray_sums_about_reference<3>(prod, a.glossy, p0, a.n, a.inv, sG);
        ray_sums_about_reference<1>(prod, a.refract, p0, a.n, a.traced ? a.inv : 1.0f, sT);      // (untraced: no "x inv")
        ray_sums_about_reference<1>(prod, a.diffuse, p0, a.n, a.inv, sD);
        if (i < a.n) {
            const GgxTail t = ggx_tail(a.s.materials, a.s.sh, i, true);
            float kr, kg, kb;
            ldrgb(a.KsColor, pindex(a.s.materials, i), kr, kg, kb);
            float dD[3], dS[3], tx[3] = { 0.0f, 0.0f, 0.0f }, iD[3] = { 0.0f, 0.0f, 0.0f }, iS[3] = { 0.0f, 0.0f, 0.0f };
#pragma unroll
            for (int c = 0; c < 3; c++) { dD[c] = oD[c] * t.d[c]; dS[c] = oS[c] * t.ks; }          // :304-305
            if (!color_is_small(t.t[0], t.t[1], t.t[2])) {                                         // :307-309
#pragma unroll
                for (int c = 0; c < 3; c++) tx[c] = sT[c] * t.t[c];
            }
            if (!color_is_small(t.d[0], t.d[1], t.d[2])) {                                         // sampleDiffuse, :315-319
#pragma unroll
                for (int c = 0; c < 3; c++) iD[c] = t.d[c] * sD[c];
            }
            if (!color_is_small(kr, kg, kb)) {                                                     // :321
#pragma unroll
                for (int c = 0; c < 3; c++) iS[c] = sG[c] * t.ks;
            }
            strgb(a.s.dd, i, dD[0], dD[1], dD[2]);
            strgb(a.s.ds, i, dS[0], dS[1], dS[2]);
            strgb(a.refract.out, i, tx[0], tx[1], tx[2]);
            strgb(a.diffuse.out, i, iD[0], iD[1], iD[2]);
            strgb(a.glossy.out, i, iS[0], iS[1], iS[2]);
            // result = diffuse + specular + transmission (:311); result += indirectDiffuse + indirectGlossy (:323)
            if (a.out.r) strgb(a.out, i, ((dD[0] + dS[0]) + tx[0]) + (iD[0] + iS[0]), ((dD[1] + dS[1]) + tx[1]) + (iD[1] + iS[1]),
                               ((dD[2] + dS[2]) + tx[2]) + (iD[2] + iS[2]));
        }
    }
}

__global__ __launch_bounds__(rlsh::kBlock) void disney_node_resolve_kernel(DisneyNodeResolveIO a)
{
    __shared__ float prod[6][kShadowTile];
    __shared__ uint8_t kinds[kShadowTile];
    __shared__ float rad[RLS_MAX_LIGHTS][3];
    stage_radiance(rad, a.s);
    for (int64_t p0 = (int64_t)blockIdx.x * rlsh::kBlock; p0 < a.n; p0 += (int64_t)gridDim.x * rlsh::kBlock) {
        const int64_t i = p0 + threadIdx.x;
        float dS[3] = { 0.0f, 0.0f, 0.0f }, dD[3] = { 0.0f, 0.0f, 0.0f }, sD[3], sS[3];
        if (a.s.nl > 0) shadow_sums<3>(prod, kinds, rad, a.s, p0, dS, dD);
        ray_sums_about_reference<3>(prod, a.diffuse, p0, a.n, a.inv, sD);
        ray_sums_about_reference<3>(prod, a.specular, p0, a.n, a.inv, sS);
        if (i < a.n) {
            const float (&iD)[3] = sD, (&iS)[3] = sS;
            strgb(a.s.dd, i, dD[0], dD[1], dD[2]);
            strgb(a.s.ds, i, dS[0], dS[1], dS[2]);
            strgb(a.diffuse.out, i, iD[0], iD[1], iD[2]);
            strgb(a.specular.out, i, iS[0], iS[1], iS[2]);
            // result = diffuse + specular (src/rlDisney.cpp:712); result += indirectDiffuse + indirectGlossy (:722)
            if (a.out.r) strgb(a.out, i, (dD[0] + dS[0]) + (iD[0] + iS[0]), (dD[1] + dS[1]) + (iD[1] + iS[1]),
                               (dD[2] + dS[2]) + (iD[2] + iS[2]));
        }
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

// one launch of the rlSss emit or resolve: a workgroup per tile of io.tile_points points, grid-striding past the cap
template <class IO>
rls_status launch_tiles(rls_context *ctx, void (*kernel)(IO), const IO &io, const char *name)
{
    const dim3 grid = rlsh::grid_for(ctx, io.n, io.tile_points);
    hipLaunchKernelGGL(kernel, grid, dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(name, RLS_FAST);
}

// the kernel selection of each verb (rls_internal.hpp, RLS_FLAVOURS): the emits by lane group g, the rlSss verbs by nothing
rls_status launch_ggx_glossy_emit(rls_context *ctx, int g, const EmitIO<rls_ggx_closure> &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(ggx_glossy_emit_kernel), g, io, name);
}
rls_status launch_ggx_refract_emit(rls_context *ctx, int g, const EmitIO<rls_ggx_closure> &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(ggx_refract_emit_kernel), g, io, name);
}
rls_status launch_disney_diffuse_emit(rls_context *ctx, int g, const EmitIO<rls_disney_closure> &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(disney_diffuse_emit_kernel), g, io, name);
}
rls_status launch_disney_specular_emit(rls_context *ctx, int g, const EmitIO<rls_disney_closure> &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(disney_specular_emit_kernel), g, io, name);
}
rls_status launch_ggx_node_glossy_emit(rls_context *ctx, int g, const GgxNodeEmitIO &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(ggx_node_glossy_emit_kernel), g, io, name);
}
rls_status launch_ggx_node_refract_emit(rls_context *ctx, int g, const GgxNodeEmitIO &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(ggx_node_refract_emit_kernel), g, io, name);
}
rls_status launch_ggx_node_diffuse_emit(rls_context *ctx, int g, const GgxNodeEmitIO &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(ggx_node_diffuse_emit_kernel), g, io, name);
}
rls_status launch_disney_node_diffuse_emit(rls_context *ctx, int g, const EmitIO<rls_disney_closure> &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(disney_node_diffuse_emit_kernel), g, io, name);
}
rls_status launch_disney_node_specular_emit(rls_context *ctx, int g, const EmitIO<rls_disney_closure> &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(disney_node_specular_emit_kernel), g, io, name);
}
rls_status launch_ggx_direct_emit(rls_context *ctx, int g, const ShadowEmitIO<rls_ggx_closure, rls_ggx_shader> &io,
                                  const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(ggx_direct_emit_kernel), g, io, name);
}
rls_status launch_disney_direct_emit(rls_context *ctx, int g, const ShadowEmitIO<rls_disney_closure, NoShader> &io,
                                     const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(disney_direct_emit_kernel), g, io, name);
}
rls_status launch_sss_probe_emit(rls_context *ctx, int, const SssEmitIO &io, const char *name)
{
    return launch_tiles(ctx, sss_probe_emit_kernel<>, io, name);
}
rls_status launch_sss_scatter_resolve(rls_context *ctx, int, const SssResolveIO &io, const char *name)
{
    return launch_tiles(ctx, sss_scatter_resolve_kernel<>, io, name);
}
rls_status launch_skin_shadow_emit(rls_context *ctx, int g, const SkinShadowEmitIO &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(skin_shadow_emit_kernel), g, io, name);
}
rls_status launch_skin_sheen_glossy_emit(rls_context *ctx, int g, const SkinGlossyEmitIO &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(skin_sheen_glossy_emit_kernel), g, io, name);
}
rls_status launch_skin_specular_glossy_emit(rls_context *ctx, int g, const SkinGlossyEmitIO &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(skin_specular_glossy_emit_kernel), g, io, name);
}
rls_status launch_skin_probe_emit(rls_context *ctx, int, const SkinProbeEmitIO &io, const char *name)
{
    return launch_tiles(ctx, skin_probe_emit_kernel<>, io, name);
}
rls_status launch_skin_node_resolve(rls_context *ctx, int, const SkinNodeResolveIO &io, const char *name)
{
    hipLaunchKernelGGL(skin_node_resolve_kernel<>, rlsh::grid_for(ctx, io.n), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(name, RLS_FAST);
}

} // namespace

RLS_FLAVOURS(ggx_glossy_emit, EmitIO<rls_ggx_closure>)
RLS_FLAVOURS(ggx_refract_emit, EmitIO<rls_ggx_closure>)
RLS_FLAVOURS(disney_diffuse_emit, EmitIO<rls_disney_closure>)
RLS_FLAVOURS(disney_specular_emit, EmitIO<rls_disney_closure>)
RLS_FLAVOURS(ggx_node_glossy_emit, GgxNodeEmitIO)
RLS_FLAVOURS(ggx_node_refract_emit, GgxNodeEmitIO)
RLS_FLAVOURS(ggx_node_diffuse_emit, GgxNodeEmitIO)
RLS_FLAVOURS(disney_node_diffuse_emit, EmitIO<rls_disney_closure>)
RLS_FLAVOURS(disney_node_specular_emit, EmitIO<rls_disney_closure>)
using GgxShadowEmitIO = ShadowEmitIO<rls_ggx_closure, rls_ggx_shader>;
using DisneyShadowEmitIO = ShadowEmitIO<rls_disney_closure, NoShader>;
RLS_FLAVOURS(ggx_direct_emit, GgxShadowEmitIO)
RLS_FLAVOURS(disney_direct_emit, DisneyShadowEmitIO)
RLS_FLAVOURS(sss_probe_emit, SssEmitIO)
RLS_FLAVOURS(sss_scatter_resolve, SssResolveIO)
RLS_FLAVOURS(skin_shadow_emit, SkinShadowEmitIO)
RLS_FLAVOURS(skin_sheen_glossy_emit, SkinGlossyEmitIO)
RLS_FLAVOURS(skin_specular_glossy_emit, SkinGlossyEmitIO)
RLS_FLAVOURS(skin_probe_emit, SkinProbeEmitIO)
RLS_FLAVOURS(skin_node_resolve, SkinNodeResolveIO)

#if !RLS_FAST

namespace {

// The staging of an emit carved out of the caller's scratch, each part 256-byte aligned: `planes` float planes and the tags
// (tag_bytes each) of n * slots_per_point slots, then the scan's tile sums.  The sample-ray emits: dir[3], w[3], 16-bit tags,
// spp slots a point; the light loops: ShadowCompactIO's planes, 32-bit tags, n_lights * 3 * spp slots a point.
constexpr int kRayPlanes = 6;
struct Staging {
    float *f[kShadowPlanes];
    void *tag;
    int64_t *totals;
    int64_t tiles;
    size_t bytes;
};
static_assert(kRayPlanes <= kShadowPlanes, "Staging::f holds the planes of either emit");
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline Staging staging(void *base, int64_t n, int slots_per_point, int planes, size_t tag_bytes)
{
    Staging s = {};
    const size_t slots = (size_t)n * (size_t)slots_per_point;
    char *p = (char *)base;
    size_t off = 0;
    for (int k = 0; k < planes; k++) { s.f[k] = (float *)(p + off); off += align256(slots * sizeof(float)); }
    s.tag = p + off; off += align256(slots * tag_bytes);
    s.tiles = (n + kScanTile - 1) / kScanTile;
    s.totals = (int64_t *)(p + off); off += align256((size_t)(s.tiles > 0 ? s.tiles : 1) * sizeof(int64_t));
    s.bytes = off;
    return s;
}

// The checks every queue verb opens with, in this order; fn: the name its messages carry
rls_status check_batch(const char *fn, const rls_context *ctx, int64_t n, int spp_n)
{
    RLS_REQUIRE_IN(fn, ctx != nullptr, "ctx is NULL");
    RLS_REQUIRE_IN(fn, n >= 0, "n < 0");
    RLS_REQUIRE_IN(fn, n <= (int64_t)UINT32_MAX, "n > 2^32 - 1 (the queue's point index is 32-bit)");
    RLS_REQUIRE_IN(fn, spp_n >= 1 && spp_n * spp_n <= kMaxSpp, "spp_n must be in [1, 16]");
    return RLS_OK;
}

// the queue of an empty batch: offsets[0] = 0
rls_status empty_queue(rls_context *ctx, int64_t *offsets, const char *name)
{
    hipLaunchKernelGGL(trace_scan_totals_kernel, dim3(1), dim3(rlsh::kBlock), 0, ctx->stream, offsets, (int64_t)0, offsets);
    return rlsh::check_launch(name);
}

// offsets: the per-point counts of an emit scanned in place (exclusive), offsets[n] = the ray count
rls_status scan_counts(rls_context *ctx, int64_t *offsets, int64_t n, int64_t *totals, int64_t tiles)
{
    rls_status s;
    hipLaunchKernelGGL(trace_scan_block_kernel, dim3((unsigned)tiles), dim3(rlsh::kBlock), 0, ctx->stream, offsets, n, totals);
    if ((s = rlsh::check_launch("trace_scan_block_kernel")) != RLS_OK) return s;
    hipLaunchKernelGGL(trace_scan_totals_kernel, dim3(1), dim3(rlsh::kBlock), 0, ctx->stream, totals, tiles, offsets + n);
    if ((s = rlsh::check_launch("trace_scan_totals_kernel")) != RLS_OK) return s;
    hipLaunchKernelGGL(trace_scan_add_kernel, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, offsets, n,
                       (const int64_t *)totals);
    return rlsh::check_launch("trace_scan_add_kernel");
}

// What every emit does between its checks and its compaction: the closure's emit kernel (dispatch, with G for the batch)
// leaves the per-point counts in offsets, which are then scanned in place.
template <class IO>
rls_status emit_and_scan(rls_context *ctx, IO &io, int64_t n, int spp_n, uint32_t seed, uint64_t first_index, int64_t *offsets,
                         const Staging &st, const char *name, rls_status (*dispatch)(rls_context *, int, const IO &, const char *))
{
    io.count = offsets;
    set_loop(io, n, spp_n, seed, first_index);
    const rls_status s = dispatch(ctx, pick_group(ctx, n, spp_n * spp_n), io, name);
    return s != RLS_OK ? s : scan_counts(ctx, offsets, n, st.totals, st.tiles);
}
// points per compaction tile: as many as tile_slots slots hold, a point's index in its tile being 8 bits
inline int compact_tile_points(int tile_slots, int per_point) { return std::min(tile_slots / per_point, kCompactMaxPoints); }

// the planes a ray emit needs of its queue (nw: the weight's planes), for n points at spp_n^2 samples; fn: the name the
// messages carry
rls_status check_ray_queue(const char *fn, const rls_ray_queue *q, int nw, int64_t n, int spp_n)
{
    RLS_REQUIRE_IN(fn, rlsh::has3(q->dir), "queue.dir plane is NULL");
    RLS_REQUIRE_IN(fn, nw == 1 ? q->weight.r != nullptr : rlsh::has3(q->weight), "queue.weight plane is NULL");
    RLS_REQUIRE_IN(fn, q->capacity >= n * spp_n * spp_n, "queue.capacity < n * spp_n^2");
    RLS_REQUIRE_IN(fn, q->scratch != nullptr && q->scratch_bytes >= staging(nullptr, n, spp_n * spp_n, kRayPlanes, sizeof(uint16_t)).bytes,
                   "queue.scratch is NULL or smaller than rls_trace_scratch_bytes");
    return RLS_OK;
}

// A checked ray emit of n > 0 points at `spp` samples a point (a node's untraced refraction: 1): the staging in the queue's
// scratch, the closure's emit kernel (io: its closure part filled), the scan, the compaction.
template <class IO>
rls_status run_ray_emit(rls_context *ctx, int64_t n, IO &io, int spp, uint32_t seed, uint64_t first_index, const rls_ray_queue *q,
                        float *side, int nw, const char *name, rls_status (*dispatch)(rls_context *, int, const IO &, const char *))
{
    const Staging st = staging(q->scratch, n, spp, kRayPlanes, sizeof(uint16_t));
    for (int k = 0; k < 3; k++) { io.dir[k] = st.f[k]; io.w[k] = st.f[3 + k]; }
    io.tag = (uint16_t *)st.tag; io.side = side;
    io.count = q->offsets;
    io.n = n; io.spp = spp; io.seed = seed; io.first = first_index;
    if (rls_status s = dispatch(ctx, pick_group(ctx, n, spp), io, name)) return s;
    if (rls_status s = scan_counts(ctx, q->offsets, n, st.totals, st.tiles)) return s;

    TraceCompactIO cio = {};
    for (int k = 0; k < 3; k++) { cio.sdir[k] = st.f[k]; cio.sw[k] = st.f[3 + k]; }
    cio.tag = io.tag; cio.offsets = q->offsets; cio.q = *q; cio.n = n; cio.spp = spp;
    cio.tile_points = compact_tile_points(kCompactSlots, spp);
    const dim3 cgrid = rlsh::grid_for(ctx, n, cio.tile_points);
    if (nw == 1) hipLaunchKernelGGL(trace_compact_kernel<1>, cgrid, dim3(rlsh::kBlock), 0, ctx->stream, cio);
    else hipLaunchKernelGGL(trace_compact_kernel<3>, cgrid, dim3(rlsh::kBlock), 0, ctx->stream, cio);
    return rlsh::check_launch("trace_compact_kernel");
}

// Every emit: the argument checks (lobe_ok: the rlDisney lobe, checked after spp_n), the empty queue of n == 0, the staging
// in the caller's scratch, then the closure's emit kernel (dispatch, with G for the batch) and the steps the closures share:
// the per-point counts scanned in place into offsets, the kept records compacted into the queue (nw weight planes).  side:
// the per-point side output; name: the entry point.
template <class Closure>
rls_status emit(rls_context *ctx, int64_t n, const Closure *c, int spp_n, uint32_t seed, uint64_t first_index, bool lobe_ok,
                const rls_ray_queue *q, float *side, int nw, const char *name,
                rls_status (*dispatch)(rls_context *, int, const EmitIO<Closure> &, const char *))
{
    if (rls_status s = check_batch(__func__, ctx, n, spp_n)) return s;
    RLS_REQUIRE(lobe_ok, "lobe must be RLS_RAY_DIFFUSE or RLS_RAY_GLOSSY");
    RLS_REQUIRE(q != nullptr && q->offsets != nullptr, "queue or queue.offsets is NULL");
    if (n == 0) return empty_queue(ctx, q->offsets, name);
    if (rls_status s = rlsh::check_closure(__func__, c)) return s;
    if (rls_status s = check_ray_queue(__func__, q, nw, n, spp_n)) return s;
    EmitIO<Closure> io = {};
    io.c = *c;
    return run_ray_emit(ctx, n, io, spp_n * spp_n, seed, first_index, q, side, nw, name, dispatch);
}

rls_status resolve(rls_context *ctx, int64_t n, const rls_ray_queue *q, int spp_n, rls_crgb radiance, rls_rgb out, bool refract)
{
    RLS_LOOP_PROLOGUE(spp_n);                            // (the glossy resolve passes spp_n = 1)
    RLS_REQUIRE(q != nullptr && q->offsets != nullptr, "queue or queue.offsets is NULL");
    RLS_REQUIRE(refract ? q->weight.r != nullptr : rlsh::has3(q->weight), "queue.weight plane is NULL");
    RLS_REQUIRE(radiance.r && radiance.g && radiance.b, "radiance plane is NULL");
    RLS_REQUIRE(rlsh::has3(out), "NULL output plane");
    TraceResolveIO io = {};
    io.offsets = q->offsets;
    io.w[0] = q->weight.r; io.w[1] = q->weight.g; io.w[2] = q->weight.b;
    io.L = radiance; io.out = out; io.n = n;
    io.scale = refract ? 1.0f / (float)(spp_n * spp_n) : 1.0f;     // AiSamplerGetSampleInvCount, src/rlGgx.h:244
    const dim3 grid = rlsh::grid_for(ctx, n);
    if (refract) hipLaunchKernelGGL(trace_resolve_kernel<1>, grid, dim3(rlsh::kBlock), 0, ctx->stream, io);
    else hipLaunchKernelGGL(trace_resolve_kernel<3>, grid, dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(refract ? "rls_trace_ggx_refract_resolve" : "rls_trace_ggx_glossy_resolve");
}

// the planes both light-loop verbs need of a queue; nwd: the planes of weight_diffuse (rlDisney 3; rlGgx 1, its .r; a lobe of
// rlSkin 0: none, and two segments a light instead of three)
rls_status check_shadow_queue(const char *fn, const rls_shadow_queue *q, int nwd, int64_t n, int nl, int spp)
{
    RLS_REQUIRE_IN(fn, rlsh::has3(q->dir) && q->maxdist != nullptr, "queue.dir or queue.maxdist plane is NULL");
    if (nwd == 0) RLS_REQUIRE_IN(fn, rlsh::has3(q->weight_specular), "queue.weight_specular plane is NULL");
    else RLS_REQUIRE_IN(fn, rlsh::has3(q->weight_specular) && (nwd == 1 ? q->weight_diffuse.r != nullptr : rlsh::has3(q->weight_diffuse)),
                        "queue.weight_specular or queue.weight_diffuse plane is NULL");
    RLS_REQUIRE_IN(fn, q->kind != nullptr, "queue.kind is NULL");
    if (nwd == 0) RLS_REQUIRE_IN(fn, q->capacity >= n * nl * kSkinShadowSegments * spp, "queue.capacity < n * n_lights * 2 * spp_n^2");
    else RLS_REQUIRE_IN(fn, q->capacity >= n * nl * kShadowSegments * spp, "queue.capacity < n * n_lights * 3 * spp_n^2");
    return RLS_OK;
}
// the staged diffuse planes of a light-loop emit (rlSkin's has none)
template <class C, class S>
void set_diffuse_staging(ShadowEmitIO<C, S> &io, const Staging &st) { for (int k = 0; k < 3; k++) io.wd[k] = st.f[7 + k]; }
void set_diffuse_staging(SkinShadowEmitIO &, const Staging &) {}
// a point's staging slots and the staged planes of a light-loop emit
inline int shadow_slots(int nwd, int nl, int spp) { return nl * (nwd == 0 ? kSkinShadowSegments : kShadowSegments) * spp; }
inline int shadow_planes(int nwd) { return nwd == 0 ? kSkinShadowPlanes : kShadowPlanes; }

// Both light-loop emits: the argument checks (closure: the node's checks of its closure, shader and P, which fill io), the
// empty queue of n == 0, the staging in the caller's scratch, the closure's emit kernel (dispatch, with G for the batch), then
// the scan of the counts and the compaction.
template <class IO, class ClosureCheck>
rls_status shadow_emit(rls_context *ctx, int64_t n, ClosureCheck closure, const rls_sphere_light *lights, int n_lights,
                       int spp_n, uint32_t seed, uint64_t first_index, const rls_shadow_queue *q, int nwd, const char *name,
                       rls_status (*dispatch)(rls_context *, int, const IO &, const char *))
{
    if (rls_status s = check_batch(name, ctx, n, spp_n)) return s;
    RLS_REQUIRE_IN(name, q != nullptr && q->offsets != nullptr, "queue or queue.offsets is NULL");
    const int spp = spp_n * spp_n;
    if (n == 0) return empty_queue(ctx, q->offsets, name);
    IO io = {};
    if (rls_status s = closure(io)) return s;
    if (rls_status s = copy_lights(lights, n_lights, 1, io.lights, &io.nl)) return s;
    if (rls_status s = check_shadow_queue(name, q, nwd, n, io.nl, spp)) return s;
    const int slots = shadow_slots(nwd, io.nl, spp);
    const Staging st = staging(q->scratch, n, slots, shadow_planes(nwd), sizeof(uint32_t));
    RLS_REQUIRE_IN(name, q->scratch != nullptr && q->scratch_bytes >= st.bytes,
                   "queue.scratch is NULL or smaller than rls_trace_shadow_scratch_bytes");

    for (int k = 0; k < 3; k++) { io.dir[k] = st.f[k]; io.ws[k] = st.f[4 + k]; }
    set_diffuse_staging(io, st);
    io.maxdist = st.f[3]; io.tag = (uint32_t *)st.tag;
    if (rls_status s = emit_and_scan(ctx, io, n, spp_n, seed, first_index, q->offsets, st, name, dispatch)) return s;

    ShadowCompactIO cio = {};
    for (int k = 0; k < shadow_planes(nwd); k++) cio.src[k] = st.f[k];
    cio.tag = io.tag; cio.offsets = q->offsets; cio.q = *q; cio.n = n; cio.spp = spp; cio.slots = slots;
    cio.tile_points = compact_tile_points(kShadowMaxSlots, slots);
    const dim3 cgrid = rlsh::grid_for(ctx, n, cio.tile_points);
    if (nwd == 0) hipLaunchKernelGGL(shadow_compact_kernel<0>, cgrid, dim3(rlsh::kBlock), 0, ctx->stream, cio);
    else if (nwd == 1) hipLaunchKernelGGL(shadow_compact_kernel<1>, cgrid, dim3(rlsh::kBlock), 0, ctx->stream, cio);
    else hipLaunchKernelGGL(shadow_compact_kernel<3>, cgrid, dim3(rlsh::kBlock), 0, ctx->stream, cio);
    return rlsh::check_launch("shadow_compact_kernel");
}

// The light loop's part of a resolve's argument struct (the light-loop resolves and the node resolves): the lights, the queue's
// planes, the visibility, 1 / spp.  n_lights >= 1.
rls_status shadow_resolve_io(const char *name, ShadowResolveIO &io, int64_t n, int nwd, const rls_sphere_light *lights,
                             int n_lights, int spp_n, const rls_shadow_queue *q, rls_crgb visibility)
{
    rls_sphere_light lt[RLS_MAX_LIGHTS];
    if (rls_status s = copy_lights(lights, n_lights, 1, lt, &io.nl)) return s;
    if (rls_status s = check_shadow_queue(name, q, nwd, n, io.nl, spp_n * spp_n)) return s;
    RLS_REQUIRE_IN(name, visibility.r && visibility.g && visibility.b, "visibility plane is NULL");
    for (int l = 0; l < io.nl; l++)
        for (int k = 0; k < 3; k++) io.rad[l][k] = lt[l].radiance[k];
    io.offsets = q->offsets; io.kind = q->kind; io.vis = visibility;
    io.ws[0] = q->weight_specular.r; io.ws[1] = q->weight_specular.g; io.ws[2] = q->weight_specular.b;
    io.wd[0] = q->weight_diffuse.r; io.wd[1] = q->weight_diffuse.g; io.wd[2] = q->weight_diffuse.b;
    io.inv = 1.0f / (float)(spp_n * spp_n);                      // as the loop kernels: 1 / spp
    io.n = n;
    return RLS_OK;
}

// Both light-loop resolves; c, sh: rlGgx's tail (NULL for rlDisney)
rls_status shadow_resolve(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh, bool ggx,
                          const rls_sphere_light *lights, int n_lights, int spp_n, const rls_shadow_queue *q, rls_crgb visibility,
                          rls_rgb direct_diffuse, rls_rgb direct_specular, const char *name)
{
    if (rls_status s = check_batch(name, ctx, n, spp_n)) return s;
    if (n == 0) return RLS_OK;
    RLS_REQUIRE_IN(name, q != nullptr && q->offsets != nullptr, "queue or queue.offsets is NULL");
    ShadowResolveIO io = {};
    if (ggx) {
        RLS_REQUIRE_IN(name, c != nullptr && sh != nullptr, "closure or shader is NULL");
        RLS_REQUIRE_IN(name, rlsh::ok_rgb(sh->KdColor), "colour planes must be all set or all NULL");
        RLS_REQUIRE_IN(name, rlsh::ok_materials(c->materials), "materials.id is set but materials.count is 0");
        io.materials = c->materials; io.sh = *sh;
    }
    if (rls_status s = shadow_resolve_io(name, io, n, ggx ? 1 : 3, lights, n_lights, spp_n, q, visibility)) return s;
    RLS_REQUIRE_IN(name, rlsh::has3(direct_diffuse) && rlsh::has3(direct_specular), "NULL output plane");
    io.dd = direct_diffuse; io.ds = direct_specular;
    const dim3 grid = rlsh::grid_for(ctx, n);
    if (ggx) hipLaunchKernelGGL(shadow_resolve_kernel<1>, grid, dim3(rlsh::kBlock), 0, ctx->stream, io);
    else hipLaunchKernelGGL(shadow_resolve_kernel<3>, grid, dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(name);
}

// What the node verbs check first: the batch, the queue struct, the light count, and the shadow queue present exactly where
// there are lights
rls_status check_node(const char *fn, const rls_context *ctx, int64_t n, int spp_n, int n_lights, bool have_queues,
                      const rls_shadow_queue *const *shadow)
{
    if (rls_status s = check_batch(fn, ctx, n, spp_n)) return s;
    RLS_REQUIRE_IN(fn, have_queues, "queues is NULL");
    RLS_REQUIRE_IN(fn, n_lights >= 0 && n_lights <= RLS_MAX_LIGHTS, "n_lights out of range (RLS_MAX_LIGHTS)");
    RLS_REQUIRE_IN(fn, n_lights > 0 || *shadow == nullptr, "queues.shadow is set but n_lights is 0");
    RLS_REQUIRE_IN(fn, n_lights == 0 || *shadow != nullptr, "queues.shadow is NULL but n_lights > 0");
    return RLS_OK;
}

// one ray queue of a node resolve: its planes, the radiance traced for it, the AOV it feeds
rls_status node_ray_io(const char *fn, TraceResolveIO &io, const rls_ray_queue *q, int nw, int64_t n, int spp_n, rls_crgb radiance,
                       rls_rgb aov)
{
    RLS_REQUIRE_IN(fn, q->offsets != nullptr, "queue.offsets is NULL");
    RLS_REQUIRE_IN(fn, nw == 1 ? q->weight.r != nullptr : rlsh::has3(q->weight), "queue.weight plane is NULL");
    RLS_REQUIRE_IN(fn, q->capacity >= n * spp_n * spp_n, "queue.capacity < n * spp_n^2");
    RLS_REQUIRE_IN(fn, radiance.r && radiance.g && radiance.b, "radiance plane is NULL");
    io.offsets = q->offsets;
    io.w[0] = q->weight.r; io.w[1] = q->weight.g; io.w[2] = q->weight.b;
    io.L = radiance; io.out = aov; io.scale = 1.0f; io.n = n;
    return RLS_OK;
}

// RLS_NODE_RESOLVE=separate: the node resolves through the existing resolve kernels and a compose pass (see
// ggx_node_compose_kernel)
bool separate_node_resolve()
{
    const char *e = getenv("RLS_NODE_RESOLVE");
    return e != nullptr && strcmp(e, "separate") == 0;
}
// one existing ray resolve of that path: the queue's plain sum (x scale for a one-plane queue) into its AOV plane
rls_status launch_ray_resolve(rls_context *ctx, TraceResolveIO io, int nw, float scale, const char *name)
{
    io.scale = scale;
    const dim3 grid = rlsh::grid_for(ctx, io.n);
    if (nw == 1) hipLaunchKernelGGL(trace_resolve_kernel<1>, grid, dim3(rlsh::kBlock), 0, ctx->stream, io);
    else hipLaunchKernelGGL(trace_resolve_kernel<3>, grid, dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(name);
}

} // namespace

extern "C" {

rls_status rls_trace_scratch_bytes(int64_t n, int spp_n, size_t *bytes)
{
    RLS_REQUIRE(bytes != nullptr, "bytes is NULL");
    RLS_REQUIRE(n >= 0, "n < 0");
    RLS_REQUIRE(spp_n >= 1 && spp_n * spp_n <= kMaxSpp, "spp_n must be in [1, 16]");
    *bytes = staging(nullptr, n, spp_n * spp_n, kRayPlanes, sizeof(uint16_t)).bytes;
    return RLS_OK;
}

rls_status rls_trace_ggx_glossy_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, int spp_n, uint32_t seed,
                                     uint64_t first_index, const rls_ray_queue *q, float *avg_reflect_weight)
{
    return emit(ctx, n, c, spp_n, seed, first_index, true, q, avg_reflect_weight, 3, __func__, dispatch_ggx_glossy_emit);
}

rls_status rls_trace_ggx_refract_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, int spp_n, uint32_t seed,
                                      uint64_t first_index, const rls_ray_queue *q, float *tir_fraction)
{
    return emit(ctx, n, c, spp_n, seed, first_index, true, q, tir_fraction, 1, __func__, dispatch_ggx_refract_emit);
}

rls_status rls_trace_disney_emit(rls_context *ctx, int64_t n, const rls_disney_closure *c, int lobe, int spp_n, uint32_t seed,
                                 uint64_t first_index, const rls_ray_queue *q, float *valid_count)
{
    const bool lobe_ok = lobe == RLS_RAY_DIFFUSE || lobe == RLS_RAY_GLOSSY;
    return emit(ctx, n, c, spp_n, seed, first_index, lobe_ok, q, valid_count, 3, __func__,
                lobe == RLS_RAY_DIFFUSE ? dispatch_disney_diffuse_emit : dispatch_disney_specular_emit);
}

rls_status rls_trace_ggx_glossy_resolve(rls_context *ctx, int64_t n, const rls_ray_queue *q, rls_crgb radiance, rls_rgb sum)
{
    return resolve(ctx, n, q, 1, radiance, sum, false);
}

rls_status rls_trace_ggx_refract_resolve(rls_context *ctx, int64_t n, const rls_ray_queue *q, int spp_n, rls_crgb radiance,
                                         rls_rgb result)
{
    return resolve(ctx, n, q, spp_n, radiance, result, true);
}

rls_status rls_trace_sss_probe_emit(rls_context *ctx, int64_t n, const rls_sss_closure *c, rls_cvec3 P, int spp_n,
                                    uint32_t seed, uint64_t first_index, const rls_probe_queue *q)
{
    if (rls_status s = check_batch(__func__, ctx, n, spp_n)) return s;
    RLS_REQUIRE(q != nullptr && q->offsets != nullptr, "queue or queue.offsets is NULL");
    const int spp = spp_n * spp_n;
    if (n == 0) return empty_queue(ctx, q->offsets, __func__);
    if (rls_status s = rlsh::check_closure(__func__, c, true)) return s;
    RLS_REQUIRE(rlsh::has3(P), "P plane is NULL");
    RLS_REQUIRE(rlsh::has3(q->origin) && rlsh::has3(q->dir) && q->maxdist != nullptr,
                "queue.origin, queue.dir or queue.maxdist plane is NULL");
    RLS_REQUIRE(q->capacity >= n * spp, "queue.capacity < n * spp_n^2");
    SssEmitIO io = {};
    io.c = *c; io.P = P; io.q = *q;
    set_loop(io, n, spp_n, seed, first_index);
    io.tile_points = sss_emit_tile_points(spp);
    return dispatch_sss_probe_emit(ctx, 0, io, __func__);
}

rls_status rls_trace_sss_scatter_resolve(rls_context *ctx, int64_t n, const rls_sss_closure *c, rls_cvec3 P, int spp_n,
                                         const rls_probe_queue *q, const rls_probe_hits *h, int use_cavity_fade,
                                         int literal_matrix, rls_rgb result, float *mean_depth)
{
    if (rls_status s = check_batch(__func__, ctx, n, spp_n)) return s;
    RLS_REQUIRE(q != nullptr, "queue is NULL");
    RLS_REQUIRE(h != nullptr, "hits is NULL");
    RLS_REQUIRE(h->max_hits >= 1 && h->max_hits <= RLS_MAX_PROBE_HITS, "hits.max_hits must be in [1, 12]");
    if (n == 0) return RLS_OK;
    const int spp = spp_n * spp_n;
    if (rls_status s = rlsh::check_closure(__func__, c, true)) return s;
    RLS_REQUIRE(rlsh::has3(P), "P plane is NULL");
    RLS_REQUIRE(q->capacity >= n * spp, "queue.capacity < n * spp_n^2");
    RLS_REQUIRE(h->stride >= n * spp, "hits.stride < n * spp_n^2");
    RLS_REQUIRE(h->count != nullptr && rlsh::has3(h->P) && rlsh::has3(h->N) && h->irradiance.r && h->irradiance.g &&
                h->irradiance.b, "hits.count, hits.P, hits.N or hits.irradiance plane is NULL");
    RLS_REQUIRE(rlsh::has3(result), "NULL output plane");
    SssResolveIO io = {};
    io.c = *c; io.P = P; io.h = *h; io.result = result; io.depth = mean_depth;
    io.n = n; io.spp = spp; io.tile_points = sss_resolve_tile_points(spp);
    io.cavity = use_cavity_fade != 0; io.literal = literal_matrix != 0;
    return dispatch_sss_scatter_resolve(ctx, 0, io, __func__);
}

rls_status rls_trace_shadow_scratch_bytes(int64_t n, int n_lights, int spp_n, size_t *bytes)
{
    RLS_REQUIRE(bytes != nullptr, "bytes is NULL");
    RLS_REQUIRE(n >= 0, "n < 0");
    RLS_REQUIRE(n_lights >= 1 && n_lights <= RLS_MAX_LIGHTS, "n_lights out of range (RLS_MAX_LIGHTS)");
    RLS_REQUIRE(spp_n >= 1 && spp_n * spp_n <= kMaxSpp, "spp_n must be in [1, 16]");
    *bytes = staging(nullptr, n, n_lights * kShadowSegments * spp_n * spp_n, kShadowPlanes, sizeof(uint32_t)).bytes;
    return RLS_OK;
}

rls_status rls_trace_ggx_direct_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                     rls_cvec3 P, const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                     uint64_t first_index, const rls_shadow_queue *q)
{
    const char *fn = __func__;
    auto closure = [&](GgxShadowEmitIO &io) -> rls_status {
        RLS_REQUIRE_IN(fn, c != nullptr && sh != nullptr, "closure or shader is NULL");
        if (rls_status s = rlsh::check_closure(fn, c, &P, sh)) return s;
        io.c = *c; io.sh = *sh; io.P = P;
        return RLS_OK;
    };
    return shadow_emit<GgxShadowEmitIO>(ctx, n, closure, lights, n_lights, spp_n, seed, first_index, q, 1, fn,
                                        dispatch_ggx_direct_emit);
}

rls_status rls_trace_disney_direct_emit(rls_context *ctx, int64_t n, const rls_disney_closure *c, rls_cvec3 P,
                                        const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                        uint64_t first_index, const rls_shadow_queue *q)
{
    const char *fn = __func__;
    auto closure = [&](DisneyShadowEmitIO &io) -> rls_status {
        if (rls_status s = rlsh::check_closure(fn, c, &P)) return s;
        io.c = *c; io.P = P;
        return RLS_OK;
    };
    return shadow_emit<DisneyShadowEmitIO>(ctx, n, closure, lights, n_lights, spp_n, seed, first_index, q, 3, fn,
                                           dispatch_disney_direct_emit);
}

rls_status rls_trace_ggx_direct_resolve(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                        const rls_sphere_light *lights, int n_lights, int spp_n, const rls_shadow_queue *q,
                                        rls_crgb visibility, rls_rgb direct_diffuse, rls_rgb direct_specular)
{
    return shadow_resolve(ctx, n, c, sh, true, lights, n_lights, spp_n, q, visibility, direct_diffuse, direct_specular, __func__);
}

rls_status rls_trace_disney_direct_resolve(rls_context *ctx, int64_t n, const rls_sphere_light *lights, int n_lights,
                                           int spp_n, const rls_shadow_queue *q, rls_crgb visibility,
                                           rls_rgb direct_diffuse, rls_rgb direct_specular)
{
    return shadow_resolve(ctx, n, nullptr, nullptr, false, lights, n_lights, spp_n, q, visibility, direct_diffuse,
                          direct_specular, __func__);
}

rls_status rls_trace_ggx_shade_emit(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                    rls_cvec3 P, const rls_sphere_light *lights, int n_lights, int traced, int spp_n,
                                    uint32_t seed, uint64_t first_index, const rls_ggx_node_queues *q)
{
    const char *fn = __func__;
    if (rls_status s = check_node(fn, ctx, n, spp_n, n_lights, q != nullptr, q ? &q->shadow : nullptr)) return s;
    RLS_REQUIRE(q->glossy != nullptr && q->refract != nullptr && q->diffuse != nullptr,
                "queues.glossy, queues.refract or queues.diffuse is NULL");
    const rls_ray_queue *const rq[3] = { q->glossy, q->refract, q->diffuse };
    const int nw[3] = { 3, 1, 1 };
    for (int k = 0; k < 3; k++) RLS_REQUIRE(rq[k]->offsets != nullptr, "queue.offsets is NULL");
    if (n > 0) {
        RLS_REQUIRE(c != nullptr && sh != nullptr, "closure or shader is NULL");
        if (rls_status s = rlsh::check_closure(fn, c, &P, sh, true)) return s;
        for (int k = 0; k < 3; k++)
            if (rls_status s = check_ray_queue(fn, rq[k], nw[k], n, spp_n)) return s;
    }
    if (n_lights > 0) {                                          // the light loop: rls_trace_ggx_direct_emit's queue
        auto closure = [&](GgxShadowEmitIO &io) -> rls_status {
            io.c = *c; io.sh = *sh; io.P = P;
            return RLS_OK;
        };
        if (rls_status s = shadow_emit<GgxShadowEmitIO>(ctx, n, closure, lights, n_lights, spp_n, seed, first_index, q->shadow,
                                                        1, fn, dispatch_ggx_direct_emit)) return s;
    }
    if (n == 0) {
        for (int k = 0; k < 3; k++)
            if (rls_status s = empty_queue(ctx, rq[k]->offsets, fn)) return s;
        return RLS_OK;
    }
    GgxNodeEmitIO io = {};
    io.c = *c; io.sh = *sh; io.traced = traced ? 1 : 0;
    const int spp = spp_n * spp_n;
    if (rls_status s = run_ray_emit(ctx, n, io, spp, seed, first_index, q->glossy, nullptr, 3, fn, dispatch_ggx_node_glossy_emit))
        return s;
    // the untraced branch is one ray a point: one sample (GgxNodeRefract)
    if (rls_status s = run_ray_emit(ctx, n, io, traced ? spp : 1, seed, first_index, q->refract, nullptr, 1, fn,
                                    dispatch_ggx_node_refract_emit)) return s;
    return run_ray_emit(ctx, n, io, spp, seed, first_index, q->diffuse, nullptr, 1, fn, dispatch_ggx_node_diffuse_emit);
}

rls_status rls_trace_ggx_shade_resolve(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                       const rls_sphere_light *lights, int n_lights, int traced, int spp_n,
                                       const rls_ggx_node_queues *q, const rls_ggx_node_traced *t,
                                       const rls_ggx_shade_out *out)
{
    const char *fn = __func__;
    if (rls_status s = check_node(fn, ctx, n, spp_n, n_lights, q != nullptr, q ? &q->shadow : nullptr)) return s;
    RLS_REQUIRE(q->glossy != nullptr && q->refract != nullptr && q->diffuse != nullptr,
                "queues.glossy, queues.refract or queues.diffuse is NULL");
    RLS_REQUIRE(t != nullptr && out != nullptr, "traced or out is NULL");
    if (n == 0) return RLS_OK;
    RLS_REQUIRE(c != nullptr && sh != nullptr, "closure or shader is NULL");
    RLS_REQUIRE(rlsh::ok_rgb(c->KsColor) && rlsh::ok_rgb(sh->KdColor) && rlsh::ok_rgb(sh->KtColor),
                "colour planes must be all set or all NULL");
    RLS_REQUIRE(rlsh::ok_materials(c->materials), "materials.id is set but materials.count is 0");
    RLS_REQUIRE(rlsh::has3(out->direct_diffuse) && rlsh::has3(out->direct_specular) && rlsh::has3(out->refraction) &&
                rlsh::has3(out->indirect_diffuse) && rlsh::has3(out->indirect_specular), "NULL AOV plane");
    RLS_REQUIRE(rlsh::has3(out->out) || (!out->out.r && !out->out.g && !out->out.b), "out planes must be all set or all NULL");
    GgxNodeResolveIO io = {};
    if (n_lights > 0)
        if (rls_status s = shadow_resolve_io(fn, io.s, n, 1, lights, n_lights, spp_n, q->shadow, t->visibility)) return s;
    io.s.materials = c->materials; io.s.sh = *sh; io.s.n = n;
    io.s.dd = out->direct_diffuse; io.s.ds = out->direct_specular;
    if (rls_status s = node_ray_io(fn, io.glossy, q->glossy, 3, n, spp_n, t->glossy, out->indirect_specular)) return s;
    if (rls_status s = node_ray_io(fn, io.refract, q->refract, 1, n, spp_n, t->refract, out->refraction)) return s;
    if (rls_status s = node_ray_io(fn, io.diffuse, q->diffuse, 1, n, spp_n, t->diffuse, out->indirect_diffuse)) return s;
    io.KsColor = c->KsColor; io.out = out->out; io.traced = traced ? 1 : 0; io.n = n;
    io.inv = 1.0f / (float)(spp_n * spp_n);                      // as the loop kernels: 1 / spp
    if (separate_node_resolve()) {
        if (io.s.nl > 0) {
            hipLaunchKernelGGL(shadow_resolve_kernel<1>, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, io.s);
            if (rls_status s = rlsh::check_launch(fn)) return s;
        }
        if (rls_status s = launch_ray_resolve(ctx, io.glossy, 3, 1.0f, fn)) return s;
        if (rls_status s = launch_ray_resolve(ctx, io.refract, 1, traced ? io.inv : 1.0f, fn)) return s;
        if (rls_status s = launch_ray_resolve(ctx, io.diffuse, 1, io.inv, fn)) return s;
        hipLaunchKernelGGL(ggx_node_compose_kernel, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, io);
        return rlsh::check_launch(fn);
    }
    hipLaunchKernelGGL(ggx_node_resolve_kernel, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(fn);
}

rls_status rls_trace_disney_shade_emit(rls_context *ctx, int64_t n, const rls_disney_closure *c, rls_cvec3 P,
                                       const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                       uint64_t first_index, const rls_disney_node_queues *q)
{
    const char *fn = __func__;
    if (rls_status s = check_node(fn, ctx, n, spp_n, n_lights, q != nullptr, q ? &q->shadow : nullptr)) return s;
    RLS_REQUIRE(q->diffuse != nullptr && q->specular != nullptr, "queues.diffuse or queues.specular is NULL");
    RLS_REQUIRE(q->diffuse->offsets != nullptr && q->specular->offsets != nullptr, "queue.offsets is NULL");
    if (n > 0) {
        if (rls_status s = rlsh::check_closure(fn, c, &P)) return s;
        if (rls_status s = check_ray_queue(fn, q->diffuse, 3, n, spp_n)) return s;
        if (rls_status s = check_ray_queue(fn, q->specular, 3, n, spp_n)) return s;
    }
    if (n_lights > 0) {                                          // the light loop: rls_trace_disney_direct_emit's queue
        auto closure = [&](DisneyShadowEmitIO &io) -> rls_status {
            io.c = *c; io.P = P;
            return RLS_OK;
        };
        if (rls_status s = shadow_emit<DisneyShadowEmitIO>(ctx, n, closure, lights, n_lights, spp_n, seed, first_index, q->shadow,
                                                           3, fn, dispatch_disney_direct_emit)) return s;
    }
    if (n == 0) {
        if (rls_status s = empty_queue(ctx, q->diffuse->offsets, fn)) return s;
        return empty_queue(ctx, q->specular->offsets, fn);
    }
    EmitIO<rls_disney_closure> io = {};
    io.c = *c;
    const int spp = spp_n * spp_n;
    if (rls_status s = run_ray_emit(ctx, n, io, spp, seed, first_index, q->diffuse, nullptr, 3, fn, dispatch_disney_node_diffuse_emit))
        return s;
    return run_ray_emit(ctx, n, io, spp, seed, first_index, q->specular, nullptr, 3, fn, dispatch_disney_node_specular_emit);
}

rls_status rls_trace_disney_shade_resolve(rls_context *ctx, int64_t n, const rls_sphere_light *lights, int n_lights,
                                          int spp_n, const rls_disney_node_queues *q, const rls_disney_node_traced *t,
                                          const rls_disney_shade_out *out)
{
    const char *fn = __func__;
    if (rls_status s = check_node(fn, ctx, n, spp_n, n_lights, q != nullptr, q ? &q->shadow : nullptr)) return s;
    RLS_REQUIRE(q->diffuse != nullptr && q->specular != nullptr, "queues.diffuse or queues.specular is NULL");
    RLS_REQUIRE(t != nullptr && out != nullptr, "traced or out is NULL");
    if (n == 0) return RLS_OK;
    RLS_REQUIRE(rlsh::has3(out->direct_diffuse) && rlsh::has3(out->direct_specular) && rlsh::has3(out->indirect_diffuse) &&
                rlsh::has3(out->indirect_specular), "NULL AOV plane");
    RLS_REQUIRE(rlsh::has3(out->out) || (!out->out.r && !out->out.g && !out->out.b), "out planes must be all set or all NULL");
    DisneyNodeResolveIO io = {};
    if (n_lights > 0)
        if (rls_status s = shadow_resolve_io(fn, io.s, n, 3, lights, n_lights, spp_n, q->shadow, t->visibility)) return s;
    io.s.n = n; io.s.dd = out->direct_diffuse; io.s.ds = out->direct_specular;
    if (rls_status s = node_ray_io(fn, io.diffuse, q->diffuse, 3, n, spp_n, t->diffuse, out->indirect_diffuse)) return s;
    if (rls_status s = node_ray_io(fn, io.specular, q->specular, 3, n, spp_n, t->specular, out->indirect_specular)) return s;
    io.out = out->out; io.n = n;
    io.inv = 1.0f / (float)(spp_n * spp_n);
    if (separate_node_resolve()) {
        if (io.s.nl > 0) {
            hipLaunchKernelGGL(shadow_resolve_kernel<3>, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, io.s);
            if (rls_status s = rlsh::check_launch(fn)) return s;
        }
        if (rls_status s = launch_ray_resolve(ctx, io.diffuse, 3, 1.0f, fn)) return s;
        if (rls_status s = launch_ray_resolve(ctx, io.specular, 3, 1.0f, fn)) return s;
        hipLaunchKernelGGL(disney_node_compose_kernel, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, io);
        return rlsh::check_launch(fn);
    }
    hipLaunchKernelGGL(disney_node_resolve_kernel, rlsh::grid_for(ctx, n), dim3(rlsh::kBlock), 0, ctx->stream, io);
    return rlsh::check_launch(fn);
}

// What both rlSkin verbs check first, in check_node's style: the batch, the queue struct and its members, the light count, and
// the two shadow queues present exactly where there are lights
static rls_status check_skin_node(const char *fn, const rls_context *ctx, int64_t n, int spp_n, const rls_sphere_light *lights,
                                  int n_lights, const rls_skin_node_queues *q)
{
    if (rls_status s = check_batch(fn, ctx, n, spp_n)) return s;
    RLS_REQUIRE_IN(fn, q != nullptr, "queues is NULL");
    RLS_REQUIRE_IN(fn, n_lights >= 0 && n_lights <= RLS_MAX_LIGHTS, "n_lights out of range (RLS_MAX_LIGHTS)");
    RLS_REQUIRE_IN(fn, n_lights == 0 || lights != nullptr, "lights is NULL");
    RLS_REQUIRE_IN(fn, n_lights > 0 || (q->sheen_shadow == nullptr && q->specular_shadow == nullptr),
                   "queues.sheen_shadow or queues.specular_shadow is set but n_lights is 0");
    RLS_REQUIRE_IN(fn, n_lights == 0 || (q->sheen_shadow != nullptr && q->specular_shadow != nullptr),
                   "queues.sheen_shadow or queues.specular_shadow is NULL but n_lights > 0");
    RLS_REQUIRE_IN(fn, q->sheen_glossy != nullptr && q->specular_glossy != nullptr && q->probes != nullptr,
                   "queues.sheen_glossy, queues.specular_glossy or queues.probes is NULL");
    RLS_REQUIRE_IN(fn, q->sheenFresnel != nullptr && q->specularFresnel != nullptr && q->sssWeight != nullptr,
                   "queues.sheenFresnel, queues.specularFresnel or queues.sssWeight is NULL");
    RLS_REQUIRE_IN(fn, q->sheen_glossy->offsets != nullptr && q->specular_glossy->offsets != nullptr && q->probes->offsets != nullptr &&
                   (n_lights == 0 || (q->sheen_shadow->offsets != nullptr && q->specular_shadow->offsets != nullptr)),
                   "queue.offsets is NULL");
    return RLS_OK;
}

rls_status rls_trace_skin_emit(rls_context *ctx, int64_t n, const rls_skin_closure *c, rls_cvec3 P,
                               const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                               uint64_t first_index, const rls_skin_node_queues *q)
{
    const char *fn = __func__;
    if (rls_status s = check_skin_node(fn, ctx, n, spp_n, lights, n_lights, q)) return s;
    const rls_shadow_queue *const sq[2] = { q->sheen_shadow, q->specular_shadow };
    const rls_ray_queue *const gq[2] = { q->sheen_glossy, q->specular_glossy };
    float *const fresnel[2] = { q->sheenFresnel, q->specularFresnel };
    const int spp = spp_n * spp_n;
    if (n == 0) {
        for (int k = 0; k < 2; k++) {
            if (n_lights > 0)
                if (rls_status s = empty_queue(ctx, sq[k]->offsets, fn)) return s;
            if (rls_status s = empty_queue(ctx, gq[k]->offsets, fn)) return s;
        }
        return empty_queue(ctx, q->probes->offsets, fn);
    }
    if (rls_status s = rlsh::check_closure(fn, c, &P)) return s;
    for (int k = 0; k < 2; k++)
        if (rls_status s = check_ray_queue(fn, gq[k], 3, n, spp_n)) return s;
    RLS_REQUIRE(rlsh::has3(q->probes->origin) && rlsh::has3(q->probes->dir) && q->probes->maxdist != nullptr,
                "queue.origin, queue.dir or queue.maxdist plane is NULL");
    RLS_REQUIRE(q->probes->capacity >= n * spp, "queue.capacity < n * spp_n^2");
    for (int k = 0; k < 2 && n_lights > 0; k++) {                // (ahead of the first launch: a refused call writes nothing)
        if (rls_status s = check_shadow_queue(fn, sq[k], 0, n, n_lights, spp)) return s;
        RLS_REQUIRE(sq[k]->scratch != nullptr &&
                    sq[k]->scratch_bytes >= staging(nullptr, n, shadow_slots(0, n_lights, spp), shadow_planes(0), sizeof(uint32_t)).bytes,
                    "queue.scratch is NULL or smaller than rls_trace_shadow_scratch_bytes");
    }
    // per lobe: the light loop, which leaves its Fresnel (sum, count) in (the lobe's Fresnel plane, sssWeight); integrateGlossy,
    // which folds on from there and writes the lobe's hand-down into its Fresnel plane
    for (int k = 0; k < 2; k++) {
        if (n_lights > 0) {
            auto closure = [&](SkinShadowEmitIO &io) -> rls_status {
                io.c = *c; io.P = P; io.lobe = k; io.fsum = fresnel[k]; io.fcnt = q->sssWeight;
                return RLS_OK;
            };
            if (rls_status s = shadow_emit<SkinShadowEmitIO>(ctx, n, closure, lights, n_lights, spp_n, seed, first_index, sq[k], 0,
                                                             fn, dispatch_skin_shadow_emit)) return s;
        }
        SkinGlossyEmitIO io = {};
        io.c = *c;
        if (n_lights > 0) { io.fsum = fresnel[k]; io.fcnt = q->sssWeight; }
        if (rls_status s = run_ray_emit(ctx, n, io, spp, seed, first_index, gq[k], fresnel[k], 3, fn,
                                        k == 0 ? dispatch_skin_sheen_glossy_emit : dispatch_skin_specular_glossy_emit)) return s;
    }
    // integrateScatter's probe rays; sssWeight from the two hand-downs
    SkinProbeEmitIO io = {};
    io.c = *c; io.P = P; io.q = *q->probes;
    io.sheenFresnel = q->sheenFresnel; io.specularFresnel = q->specularFresnel; io.sssWeight = q->sssWeight;
    set_loop(io, n, spp_n, seed, first_index);
    io.tile_points = sss_emit_tile_points(spp);
    return dispatch_skin_probe_emit(ctx, 0, io, fn);
}

rls_status rls_trace_skin_resolve(rls_context *ctx, int64_t n, const rls_skin_closure *c, rls_cvec3 P,
                                  const rls_sphere_light *lights, int n_lights, int use_cavity_fade, int literal_matrix,
                                  int spp_n, const rls_skin_node_queues *q, const rls_skin_node_traced *t,
                                  const rls_skin_integrate_out *out)
{
    const char *fn = __func__;
    if (rls_status s = check_skin_node(fn, ctx, n, spp_n, lights, n_lights, q)) return s;
    RLS_REQUIRE(t != nullptr && out != nullptr, "traced or out is NULL");
    RLS_REQUIRE(t->hits != nullptr, "traced.hits is NULL");
    RLS_REQUIRE(t->hits->max_hits >= 1 && t->hits->max_hits <= RLS_MAX_PROBE_HITS, "hits.max_hits must be in [1, 12]");
    if (n == 0) return RLS_OK;
    const int spp = spp_n * spp_n;
    if (rls_status s = rlsh::check_closure(fn, c, &P)) return s;
    RLS_REQUIRE(rlsh::has3(out->sheen) && rlsh::has3(out->specular) && rlsh::has3(out->sss), "NULL AOV plane");
    RLS_REQUIRE(rlsh::has3(out->out) || (!out->out.r && !out->out.g && !out->out.b), "out planes must be all set or all NULL");
    SkinNodeResolveIO io = {};
    if (n_lights > 0) {
        if (rls_status s = shadow_resolve_io(fn, io.sheen_s, n, 0, lights, n_lights, spp_n, q->sheen_shadow, t->sheen_visibility))
            return s;
        if (rls_status s = shadow_resolve_io(fn, io.spec_s, n, 0, lights, n_lights, spp_n, q->specular_shadow, t->specular_visibility))
            return s;
    }
    io.sheen_s.n = n; io.spec_s.n = n;
    if (rls_status s = node_ray_io(fn, io.sheen_g, q->sheen_glossy, 3, n, spp_n, t->sheen_glossy, out->sheen)) return s;
    if (rls_status s = node_ray_io(fn, io.spec_g, q->specular_glossy, 3, n, spp_n, t->specular_glossy, out->specular)) return s;
    const rls_probe_hits *h = t->hits;
    RLS_REQUIRE(q->probes->capacity >= n * spp, "queue.capacity < n * spp_n^2");
    RLS_REQUIRE(h->stride >= n * spp, "hits.stride < n * spp_n^2");
    RLS_REQUIRE(h->count != nullptr && rlsh::has3(h->P) && rlsh::has3(h->N) && h->irradiance.r && h->irradiance.g &&
                h->irradiance.b, "hits.count, hits.P, hits.N or hits.irradiance plane is NULL");
    io.c = *c; io.P = P; io.h = *h; io.o = *out;
    io.sheenFresnel = q->sheenFresnel; io.specularFresnel = q->specularFresnel; io.sssWeight = q->sssWeight;
    io.inv = 1.0f / (float)spp;                                  // as the loop kernels: 1 / spp
    io.spp = spp; io.tile_points = sss_resolve_tile_points(spp);
    io.cavity = use_cavity_fade != 0; io.literal = literal_matrix != 0; io.n = n;
    return dispatch_skin_node_resolve(ctx, 0, io, fn);
}

} // extern "C"

#endif // !RLS_FAST
