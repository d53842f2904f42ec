// rls_trace_body_ggx_node_resolve.hpp -- the body of ggx_node_resolve_kernel and ggx_bounce_resolve_kernel
// (rls_trace_node_resolve.hpp, which includes it once inside each, after `constexpr bool STATE`): a and STATE are the kernel's.
    __shared__ float prod[6][kShadowTile];
    __shared__ uint8_t kinds[kShadowTile];
    __shared__ float rad[RLS_MAX_LIGHTS][3];
    stage_radiance(rad, a.s);
    for (int64_t p0 = (int64_t)blockIdx.x * rlsh::kBlock; p0 < a.n; p0 += (int64_t)gridDim.x * rlsh::kBlock) {
        const int64_t i = p0 + threadIdx.x;
        float oS[3] = { 0.0f, 0.0f, 0.0f }, oD[3] = { 0.0f, 0.0f, 0.0f }, sG[3], sT[3], sD[3];
        if (a.s.nl > 0) shadow_sums<1>(prod, kinds, rad, a.s, p0, oS, oD);
        ray_sums_about_reference<3>(prod, a.glossy, p0, a.n, a.inv, sG);
        BounceGates b = { true, true, true, true, true, false, false, false };    // (the node call: a camera ray at depth 0)
        float invT = a.traced ? a.inv : 1.0f;                                                     // (untraced: no "x inv")
        if constexpr (STATE) {
            if (i < a.n) b = bounce_gates(a.st, i);
            invT = b.traced ? a.inv : 1.0f;
        }
        ray_sums_about_reference<1>(prod, a.refract, p0, a.n, invT, sT);
        ray_sums_about_reference<1>(prod, a.diffuse, p0, a.n, a.inv, sD);
        if (i < a.n) {
            const GgxTail t = ggx_tail(a.s.materials, a.s.sh, i, true);
            float kr, kg, kb;
            ldrgb(a.KsColor, pindex(a.s.materials, i), kr, kg, kb);
            float dD[3], dS[3], tx[3] = { 0.0f, 0.0f, 0.0f }, iD[3] = { 0.0f, 0.0f, 0.0f }, iS[3] = { 0.0f, 0.0f, 0.0f };
            if constexpr (STATE) {
#pragma unroll
                for (int c = 0; c < 3; c++) { oD[c] = b.diffuse ? oD[c] : 0.0f; oS[c] = b.specular ? oS[c] : 0.0f; }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) { dD[c] = oD[c] * t.d[c]; dS[c] = oS[c] * t.ks; }          // :304-305
            if (b.lit && !color_is_small(t.t[0], t.t[1], t.t[2])) {                                // :307-309
#pragma unroll
                for (int c = 0; c < 3; c++) tx[c] = sT[c] * t.t[c];
            }
            if (b.cam && b.diffuse && !color_is_small(t.d[0], t.d[1], t.d[2])) {                   // sampleDiffuse, :315-319
#pragma unroll
                for (int c = 0; c < 3; c++) iD[c] = t.d[c] * sD[c];
            }
            if (b.cam && !color_is_small(kr, kg, kb)) {                                            // :321
#pragma unroll
                for (int c = 0; c < 3; c++) iS[c] = sG[c] * t.ks;
            }
            if constexpr (STATE) {
                if (!b.lit) {
#pragma unroll
                    for (int c = 0; c < 3; c++) { dD[c] = 0.0f; dS[c] = 0.0f; }
                }
            }
            strgb(a.s.dd, i, dD[0], dD[1], dD[2]);
            strgb(a.s.ds, i, dS[0], dS[1], dS[2]);
            strgb(a.refract.out, i, tx[0], tx[1], tx[2]);
            strgb(a.diffuse.out, i, iD[0], iD[1], iD[2]);
            strgb(a.glossy.out, i, iS[0], iS[1], iS[2]);
            // result = diffuse + specular + transmission (:311); result += indirectDiffuse + indirectGlossy (:323)
            if (STATE && !b.cam) {                               // (no "+ (0 + 0)": the reference adds nothing off a camera ray)
                if (a.out.r) strgb(a.out, i, (dD[0] + dS[0]) + tx[0], (dD[1] + dS[1]) + tx[1], (dD[2] + dS[2]) + tx[2]);
            } else if (a.out.r) {
                strgb(a.out, i, ((dD[0] + dS[0]) + tx[0]) + (iD[0] + iS[0]), ((dD[1] + dS[1]) + tx[1]) + (iD[1] + iS[1]),
                      ((dD[2] + dS[2]) + tx[2]) + (iD[2] + iS[2]));
            }
        }
    }
