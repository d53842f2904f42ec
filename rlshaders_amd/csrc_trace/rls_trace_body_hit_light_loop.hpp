// rls_trace_body_hit_light_loop.hpp -- evalLightSample's Oren-Nayar light loop at one "point" of sss_hits_emit_kernel and
// skin_diffuse_emit_kernel (rls_trace_hits.hpp, which includes it once inside each kernel's point walk): the closure `on` about
// N, the view (kView: whether it is another direction than N), the frame fr, the position P and the sample index `index` are the
// point's; a, st (the point's ShadowStage), slow, tab, spp, sub, tid, zero, G and K the kernel's.  Whole wavefront (ballots,
// shuffles): the trip counts depend on the call alone.
        for (int l = 0; l < a.nl; l++) {
            const LightRegs lt = light_regs(a.lights[l], P);
            const LightCone &cone = lt.cone;
            const int mode = lt.mode;
            const uint32_t stream = kScrambleStream + 6 * l;
            const uint32_t sx = hash_u32(a.seed, index, stream), sy = hash_u32(a.seed, index, stream + 1);
            const uint32_t dx = hash_u32(a.seed, index, stream + 4), dy = hash_u32(a.seed, index, stream + 5);

            // segment 0: one light sample
            if (mode == RLS_MIS_BSDF_ONLY) st.skip(l, 0);
            for (int s0 = sub; mode != RLS_MIS_BSDF_ONLY && s0 - sub < spp; s0 += K * G) {
                RLS_LIGHT_SAMPLE_PUSH(slow, qn, tab, spp, s0, cone, N, sx, sy,
                                      slow.st[0][k][tid] = L.x; slow.st[1][k][tid] = L.y; slow.st[2][k][tid] = L.z;)
                hit_light_eval_run<K, kView>(slow, qn, on, view, cone.pdf, mode);
#pragma unroll 1
                for (int k = 0; k < K; k++) {
                    float t[4], ud[3] = { 0.0f, 0.0f, 0.0f };
                    if (eval_pop<K>(slow, k, t)) ud[0] = t[3];
                    const V3 L = mk(slow.st[0][k][tid], slow.st[1][k][tid], slow.st[2][k][tid]);
                    st.template put<1>(cone, l, 0, s0 + k * G, s0 + k * G < spp, L, zero, ud);
                }
            }
            // segment 1: one BSDF sample of the Oren-Nayar lobe (streams +4/5), where it hits the light
            if (mode == RLS_MIS_LIGHT_ONLY) st.skip(l, 1);
            for (int s0 = sub; mode != RLS_MIS_LIGHT_ONLY && s0 - sub < spp; s0 += G) {
                const int s = s0;
                float ud[3] = { 0.0f, 0.0f, 0.0f };
                V3 Ld = mk(0.0f, 0.0f, 0.0f);
                if (s < spp && cone.valid) {
                    const float rx = bits_u01(tab[0][s] ^ dx), ry = bits_u01(tab[1][s] ^ dy);
                    Ld = cosine_hemisphere(fr, rx, ry);
                    const float pd = oren_nayar_pdf(on, Ld);
                    if (pd > 0.0f && cone_hit(cone, Ld)) {
                        const float fd = oren_nayar_brdf(on, view, Ld);
                        const float wd = mode == RLS_MIS_BSDF_ONLY ? 1.0f : power_heuristic(pd, cone.pdf);
                        ud[0] = R_DIV(fd * wd, pd);
                    }
                }
                st.template put<1>(cone, l, 1, s, s < spp, Ld, zero, ud);
            }
        }
