// rls_trace_shadow_emit.hpp -- the light loops' shadow-ray emits and rlSkin's shadow and glossy emits (part of trace.hip,
// included there inside its anonymous namespace, after rls_trace_emit.hpp).  The light loops' emit has the sample-ray emits'
// three steps with a queue of its own (rls_shadow_queue): ggx_direct_emit_kernel / disney_direct_emit_kernel /
// skin_shadow_emit_kernel, the scan, shadow_compact_kernel (rls_trace_queue.hpp).

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
// function taking the struct by reference went from 56 to 144 B (measured again with the bounce calls: 56 -> 144 B, and
// rlGgx's 0 -> 32 B).  So the state-gated instantiations of the bounce calls (ggx_bounce_direct_emit_kernel,
// disney_bounce_direct_emit_kernel) share their parent's lines as an INCLUDED body, rls_trace_body_*_direct_emit.hpp, with
// `if constexpr (STATE)` around the few lines that differ: the parents compile to the code they had.

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

// One point's place in the staging and its running ray count; SEGS: the segments of a light.  STATE (the bounce calls): `lobes`,
// the RLS_SHADOW_SPECULAR / _DIFFUSE bits of the lobes the point's ray state leaves; a term of another lobe is not the ray's.
template <int G, class IO, int SEGS = kShadowSegments, bool STATE = false>
struct ShadowStage {
    const IO &a;
    int64_t i;
    bool live;
    int sub, run;
    int lobes;
    // sample s of segment `seg` of light l, in every lane of the wavefront (group_rank ballots): dir and the two lobes' terms
    // (zeros where the ray carries none); NWD: the planes of the diffuse term
    template <int NWD>
    __device__ __forceinline__ void put(const LightCone &cone, int l, int seg, int s, bool ok, V3 dir, const float (&ws)[3],
                                        const float (&wd)[3])
    {
        bool bs = !(ws[0] == 0.0f && ws[1] == 0.0f && ws[2] == 0.0f);
        bool bd = !(wd[0] == 0.0f);
        if (NWD == 3) bd = !(wd[0] == 0.0f && wd[1] == 0.0f && wd[2] == 0.0f);
        if constexpr (STATE) { bs = bs && (lobes & RLS_SHADOW_SPECULAR); bd = bd && (lobes & RLS_SHADOW_DIFFUSE); }
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
                if constexpr (kStageSpecular<IO>) {
#pragma unroll
                    for (int c = 0; c < 3; c++) al.ws[c][slot] = ws[c];
                }
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

// STATE, the bounce call's instantiation (rls_trace_ggx_bounce_emit): the loop runs whole -- sampleDiffuse stays the colour's
// test, so every weight is the parent's -- and the point's ray state decides which lobes' terms its rays carry (ShadowStage):
// the diffuse term and segment 1 exist iff Rr_diff <= GI_diffuse_depth, the specular term and segment 2 iff Rr_gloss <=
// GI_glossy_depth (src/rlGgx.cpp:280, 292), neither at a shadow ray's point.
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void ggx_direct_emit_kernel(ShadowEmitIO<rls_ggx_closure, rls_ggx_shader> a)
{
    constexpr bool STATE = false;
#include "rls_trace_body_ggx_direct_emit.hpp"
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void ggx_bounce_direct_emit_kernel(ShadowEmitIO<rls_ggx_closure, rls_ggx_shader> a)
{
    constexpr bool STATE = true;
#include "rls_trace_body_ggx_direct_emit.hpp"
}

// STATE (rls_trace_disney_bounce_emit): rlDisney's light loop is whole at every depth (src/rlDisney.cpp:695-705); a shadow
// ray's point has no rays.
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_DISNEY_LIGHT_ATTR void disney_direct_emit_kernel(ShadowEmitIO<rls_disney_closure, NoShader> a)
{
    constexpr bool STATE = false;
#include "rls_trace_body_disney_direct_emit.hpp"
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_DISNEY_LIGHT_ATTR void disney_bounce_direct_emit_kernel(ShadowEmitIO<rls_disney_closure, NoShader> a)
{
    constexpr bool STATE = true;
#include "rls_trace_body_disney_direct_emit.hpp"
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
    constexpr bool STATE = false;
#include "rls_trace_body_skin_shadow_emit.hpp"
}
// STATE (rls_trace_skin_bounce_emit): both lobes sit behind sS = Rr_gloss <= GI_glossy_depth (src/rlSkin.cpp:185) and neither
// runs at a shadow ray's point: such a point draws nothing -- no ray, and (sum, count) = (0, 0) handed on.
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void skin_bounce_shadow_emit_kernel(SkinBounceShadowEmitIO a)
{
    constexpr bool STATE = true;
#include "rls_trace_body_skin_shadow_emit.hpp"
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

// STATE (rls_trace_skin_bounce_emit): the lobe behind sS as its light loop (lobe_open: else the scalar 0 is handed down), and
// integrateGlossy behind Rr == 0 on top of the lobe's own gates (src/rlSkin.cpp:200, 224): where that is shut the queue has no
// ray for the point and the hand-down is the mean over the light loop's BSDF samples alone -- what a small colour gets.
template <int G, int LOBE>
struct SkinBounceGlossy : SkinGlossy<G, LOBE> {
    __device__ SkinBounceGlossy(const SkinBounceGlossyEmitIO &a, int64_t ii) : SkinGlossy<G, LOBE>(a, ii)
    {
        const SkinGates b = skin_gates(a.st, ii);
        this->lobe_open = this->lobe_open && b.specular;
        this->open = this->open && b.specular && b.first;
    }
};
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void skin_bounce_sheen_glossy_emit_kernel(SkinBounceGlossyEmitIO a)
{
    emit_points<G, SkinBounceGlossy<G, 0>>(a);
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void skin_bounce_specular_glossy_emit_kernel(SkinBounceGlossyEmitIO a)
{
    emit_points<G, SkinBounceGlossy<G, 1>>(a);
}
