// rls_trace_body_disney_direct_emit.hpp -- the body of disney_direct_emit_kernel and disney_bounce_direct_emit_kernel
// (rls_trace_shadow_emit.hpp, which includes it once inside each, after `constexpr bool STATE`): G, a and STATE are the kernel's.
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
        ShadowStage<G, decltype(a), kShadowSegments, STATE> st = { a, i, live, sub, 0, 0 };
        if constexpr (STATE) st.lobes = bounce_gates(a.st, ii).lit ? RLS_SHADOW_SPECULAR | RLS_SHADOW_DIFFUSE : 0;
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
