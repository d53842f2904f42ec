// rls_trace_emit.hpp -- the sample-ray emits of the caller-traced integrators (part of trace.hip, included there inside its
// anonymous namespace): integrateGlossy and integrateRefract's traced branch (src/rlGgx.h:172-184, 228-244), rlDisney's
// integrateDiffuse / integrateGlossy (src/rlDisney.cpp:240-243, 279-283), and the same lobes as the whole nodes draw them.
//
// Step 1 of an emit (steps 2 and 3: rls_trace_queue.hpp).  ggx_{glossy,refract}_emit_kernel,
// disney_{diffuse,specular}_emit_kernel: the sample loop of rls_ggx_integrate / rls_ggx_integrate_refract / one lobe of
// rls_disney_integrate (one G-lane group per point, the same packed sampling), each sample computed ONCE: its record goes to a
// fixed staging slot s * n + i (sample-major: the lanes of a wavefront store to consecutive words) with a tag (its rank among
// the point's kept samples, or "dropped"), the point's kept count to offsets[i].  A count pass and a write pass would run the
// sample arithmetic twice.  The node emits (*_node_*_emit_kernel): one kernel per queue of rls_ggx_shade / rls_disney_shade --
// the same lobes at the node's stream pairs, behind the node's gates.

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
//   kPerSample, wants(s)     a lobe that takes only some of an open point's samples (kPerSample): the others draw and queue nothing
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
                    bool ok = s < a.spp && open;
                    if constexpr (Lobe::kPerSample) ok = ok && lobe.wants(s);
                    lobe.push(slow, k, cnt, ok, bits_u01(tab[0][sc] ^ sx), bits_u01(tab[1][sc] ^ sy));
                }
                slow_run<K>(slow, cnt);
            }
#pragma unroll 1
            for (int k = 0; k < K; k++) {
                const int s = s0 + k * G;
                const bool in = s < a.spp;
                bool ok = in && open;
                if constexpr (Lobe::kPerSample) ok = ok && lobe.wants(s);
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
    static constexpr bool kPerSample = false;
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
    static constexpr bool kPerSample = false;
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
    static constexpr bool kPerSample = false;
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
// Secondary-ray hits (rls_trace_*_bounce_emit): the node's lobes with `open`, and for refraction `traced`, read off the point's
// ray state (bounce_gates, rls_trace_device.hpp) on top of the node's own gates.  Every point of a launch runs at the call's spp.

// integrateGlossy: camera rays only (src/rlGgx.cpp:307)
template <int G>
struct GgxBounceGlossy : GgxNodeGlossy<G> {
    __device__ GgxBounceGlossy(const GgxBounceEmitIO &a, int64_t ii) : GgxNodeGlossy<G>(a, ii)
    {
        this->open = this->open && bounce_gates(a.st, ii).cam;
    }
};
// integrateRefract: the branch per point; the untraced branch's one ray is sample 0 of the point
template <int G>
struct GgxBounceRefract : GgxNodeRefract<G> {
    static constexpr bool kPerSample = true;
    __device__ GgxBounceRefract(const GgxBounceEmitIO &a, int64_t ii) : GgxNodeRefract<G>(a, ii)
    {
        const BounceGates b = bounce_gates(a.st, ii);
        this->open = this->open && b.lit;
        this->traced = b.traced;
    }
    __device__ bool wants(int s) const { return this->traced || s == 0; }
};
// the indirect diffuse loop: camera rays with sampleDiffuse, its depth half included (src/rlGgx.cpp:280, 313)
template <int G>
struct GgxBounceDiffuse : GgxNodeDiffuse<G> {
    __device__ GgxBounceDiffuse(const GgxBounceEmitIO &a, int64_t ii) : GgxNodeDiffuse<G>(a, ii)
    {
        const BounceGates b = bounce_gates(a.st, ii);
        this->open = this->open && b.cam && b.diffuse;
    }
};
// rlDisney's lobes behind shouldTraceDiffuse / shouldTraceGlossy (src/rlDisney.cpp:75-83, 713-719)
template <int G, bool SPEC>
struct DisneyBounceLobe : DisneyLobe<G, SPEC, kNodeStream + (SPEC ? 2 : 0)> {
    static constexpr bool kGated = true;
    bool open;
    __device__ DisneyBounceLobe(const DisneyBounceEmitIO &a, int64_t ii) : DisneyLobe<G, SPEC, kNodeStream + (SPEC ? 2 : 0)>(a, ii)
    {
        const BounceGates b = bounce_gates(a.st, ii);
        open = SPEC ? b.trace_glossy : b.trace_diffuse;
    }
};

template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void ggx_bounce_glossy_emit_kernel(GgxBounceEmitIO a)
{
    emit_points<G, GgxBounceGlossy<G>>(a);
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void ggx_bounce_refract_emit_kernel(GgxBounceEmitIO a)
{
    emit_points<G, GgxBounceRefract<G>>(a);
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void ggx_bounce_diffuse_emit_kernel(GgxBounceEmitIO a)
{
    emit_points<G, GgxBounceDiffuse<G>>(a);
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void disney_bounce_diffuse_emit_kernel(DisneyBounceEmitIO a)
{
    emit_points<G, DisneyBounceLobe<G, false>>(a);
}
template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void disney_bounce_specular_emit_kernel(DisneyBounceEmitIO a)
{
    emit_points<G, DisneyBounceLobe<G, true>>(a);
}
