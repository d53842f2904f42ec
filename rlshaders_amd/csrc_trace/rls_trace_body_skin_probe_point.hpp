// rls_trace_body_skin_probe_point.hpp -- one point of skin_probe_emit_kernel and skin_bounce_probe_emit_kernel
// (rls_trace_probe.hpp, which includes it once inside each kernel's point function, after `constexpr bool STATE`): a, i, p and fr
// are the function's; it returns whether the point's probe rays are traced.
        const rls_skin_closure &c = a.c;
        const PIndex<int64_t> pk = pindex(c.materials, i);
        const float mult = ldp(c.sss_dist_multiplier, pk);                            // :235-236
        float sssWeight = ldp(c.sss_weight, pk);
        sssWeight *= 1.0f - a.specularFresnel[i] * (1.0f - a.sheenFresnel[i]);        // :238
        bool walk = true;
        if constexpr (STATE) {
            const SkinGates b = state_gates<STATE>(a, i);
            if (!b.lit) sssWeight = 0.0f;                                             // :169-172: nothing is shaded
            walk = b.lit && !b.sss_diffuse;                                           // src/rlSss.h:172: the light loop instead
        }
        a.sssWeight[i] = sssWeight;
        p = nd_make<true>(ldp(c.sss_scatter_dist[0], pk) * mult, ldp(c.sss_scatter_dist[1], pk) * mult,
                          ldp(c.sss_scatter_dist[2], pk) * mult);
        fr = sss_frame(ld3(c.N, i), ld3(c.T, i), true);
        return walk && !(sssWeight < kEps);
