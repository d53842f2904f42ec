// rls_trace_body_disney_node_resolve.hpp -- the body of disney_node_resolve_kernel and disney_bounce_resolve_kernel
// (rls_trace_node_resolve.hpp, which includes it once inside each, after `constexpr bool STATE`): a and STATE are the kernel's.
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
            bool cam = true;
            if constexpr (STATE) {
                const BounceGates b = bounce_gates(a.st, i);
                cam = b.cam;
                if (b.scaled) {
                    const PIndex<int64_t> pk = pindex(a.materials, i);
                    const float kd = ldp(a.diffuse_scale, pk), ks = ldp(a.specular_scale, pk);
#pragma unroll
                    for (int c = 0; c < 3; c++) { dD[c] = dD[c] * kd; dS[c] = dS[c] * ks; }
                }
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    if (!b.lit) { dD[c] = 0.0f; dS[c] = 0.0f; }
                    if (!b.cam) { sD[c] = 0.0f; sS[c] = 0.0f; }
                }
            }
            const float (&iD)[3] = sD, (&iS)[3] = sS;
            strgb(a.s.dd, i, dD[0], dD[1], dD[2]);
            strgb(a.s.ds, i, dS[0], dS[1], dS[2]);
            strgb(a.diffuse.out, i, iD[0], iD[1], iD[2]);
            strgb(a.specular.out, i, iS[0], iS[1], iS[2]);
            // result = diffuse + specular (src/rlDisney.cpp:712); result += indirectDiffuse + indirectGlossy (:722)
            if (STATE && !cam) {
                if (a.out.r) strgb(a.out, i, dD[0] + dS[0], dD[1] + dS[1], dD[2] + dS[2]);
            } else if (a.out.r) {
                strgb(a.out, i, (dD[0] + dS[0]) + (iD[0] + iS[0]), (dD[1] + dS[1]) + (iD[1] + iS[1]),
                      (dD[2] + dS[2]) + (iD[2] + iS[2]));
            }
        }
    }
