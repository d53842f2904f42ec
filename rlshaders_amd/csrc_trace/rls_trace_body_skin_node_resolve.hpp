// rls_trace_body_skin_node_resolve.hpp -- the body of skin_node_resolve_kernel and skin_bounce_resolve_kernel
// (rls_trace_node_resolve.hpp, which includes it once inside each, after `constexpr bool STATE`): a and STATE are the kernel's.
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
        SkinGates b = {};
        float dD[3] = { 0.0f, 0.0f, 0.0f };
        if constexpr (STATE) {
            const ShadowResolveIO &dif = skin_diffuse_loop<STATE>(a);
            if (dif.nl > 0) shadow_sums<1, false>(prod, kinds, rad, dif, p0, none, dD);                 // src/rlSss.h:177-183
            if (i < a.n) b = state_gates<STATE>(a, i);
        }
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
                bool walk = !(al.sssWeight[pi] < kEps);
                if constexpr (STATE) walk = walk && !state_gates<STATE>(a, pi).sss_diffuse;      // (a shadow ray's sssWeight is 0)
                if (!walk) {
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
            if constexpr (STATE) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    if (!b.specular) { sh[k] = 0.0f; sp[k] = 0.0f; }                      // :185: AI_RGB_BLACK, not 0 * weight
                    if (b.sss_diffuse) ss[k] = sssWeight < kEps ? 0.0f : (bc3[k] * dD[k]) * sssWeight;    // src/rlSss.h:185
                }
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
