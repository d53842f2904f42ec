// rls_trace_body_skin_shadow_emit.hpp -- the body of skin_shadow_emit_kernel and skin_bounce_shadow_emit_kernel
// (rls_trace_shadow_emit.hpp, which includes it once inside each, after `constexpr bool STATE`): G, a and STATE are the kernel's.
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
        ShadowStage<G, SkinShadowEmitIO, kSkinShadowSegments> st = { a, i, live, sub, 0, 0 };
        bool open = true;
        if constexpr (STATE) open = state_gates<STATE>(a, ii).specular;
        float f = 0.0f, cnt = 0.0f;
        for (int l = 0; l < a.nl; l++) {
            const LightRegs lt = light_regs(a.lights[l], P);
            const LightCone &cone = lt.cone;
            const int mode = lt.mode;
            uint32_t scr[4];
#pragma unroll
            for (int k = 0; k < 4; k++) scr[k] = hash_u32(a.seed, index, kScrambleStream + 2 * (stream + 4 * l) + k);
            bool draw = sl.weight > kEps && cone.valid;
            if constexpr (STATE) draw = draw && open;
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
