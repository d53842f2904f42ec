// rls_trace_body_ggx_direct_emit.hpp -- the body of ggx_direct_emit_kernel and ggx_bounce_direct_emit_kernel
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
        RLS_GGX_LOAD(g, a.c, ii)
        const VndfView w = vndf_view(g.view, g.fr, g.ax, g.ay);
        const OrenNayar on = oren_nayar_make(N, ldp(a.sh.diffuseRoughness, pk));
        const float kd = ldp(a.sh.Kd, pk);
        float dr, dg, db;
        ldrgb(a.sh.KdColor, pk, dr, dg, db);
        const bool sampleDiffuse = !color_is_small(dr * kd, dg * kd, db * kd);      // src/rlGgx.cpp:279-281
        const V3 P = ld3(a.P, ii);
        const uint64_t index = a.first + (uint64_t)ii;
        ShadowStage<G, decltype(a), kShadowSegments, STATE> st = { a, i, live, sub, 0, 0 };
        if constexpr (STATE) {
            const BounceGates b = bounce_gates(a.st, ii);
            st.lobes = (b.specular ? RLS_SHADOW_SPECULAR : 0) | (b.diffuse ? RLS_SHADOW_DIFFUSE : 0);
        }
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
