// ggx_rr.hip -- librls_ggx_rr.so: the EXACT, every-plane-streamed rlGgx reflect+refract kernel (BASELINE config 2) with ONE
// pass of the uniform-slope fallback per workgroup tile instead of one per wavefront (rls_rr_device.hpp).  A companion code
// object beside librlshaders_amd.so, whose device code is frozen (tests/test_profile_binding.py): csrc/ggx.hip finds this
// library next to itself and hands it the launches of ggx_kernel<OP_REFLECT_REFRACT, 0, STREAMED_ALL>; without this file, or
// with RLS_GGX_RR_WG=0, that kernel runs as before.  One exported symbol, the launcher at the end.
//
// The body is ggx_body<OP_REFLECT_REFRACT, 0, STREAMED_ALL> of csrc/ggx.hip: the same calls in the same order on the same
// loads, the same occupancy, block, tile walk, argument reloads and non-temporal plane accesses; only the packing of the
// fallback's requests differs.  Outputs are the same bits.
#include "../csrc/rls_internal.hpp"
#include "rls_rr_device.hpp"

#if RLS_FAST
#error "the companion kernel is the EXACT flavour only"
#endif

using namespace rlsd;

namespace {

using rlsh::GgxIO;

__global__ __launch_bounds__(rlsh::kBlock) __attribute__((amdgpu_waves_per_eu(8, 8))) void ggx_rr_wg_kernel(GgxIO a0)
{
    __shared__ RrShared sh;
    stage_libm_tables();   // the range table of atanf -> LDS (visible-normal sampling calls atan2f twice); ends in a barrier
    const TileRange tiles = tile_range(a0.n);              // workgroup-uniform bounds
    uint32_t round = 0;
    for (int64_t base = tiles.first; base < tiles.end; base += tiles.step, ++round) {
        const Idx i = make_idx(base);
        // a scalar test: the whole workgroup takes one side.  A full tile (every lane has a point) shares the fallback
        // across the workgroup, with barriers; the batch's last, partial tile runs the per-wavefront form, without any.
        // (gfx950 compares 64-bit integers for order in the vector unit only: the test is made on the halves of n - base > 0)
        const uint64_t left = (uint64_t)(a0.n - base);
        const uint32_t left_lo = (uint32_t)left, left_hi = (uint32_t)(left >> 32);
        const bool full = (left_hi | (left_lo >> 8)) != 0u;              // base + kBlock <= n
        static_assert(rlsh::kBlock == 256, "the shift above is log2(kBlock)");
        if (!full && threadIdx.x >= left_lo) continue;
        const GgxIO a = reload_args(a0);
        const rls_ggx_closure &c = a.c;
        V3 wo = ld3(c.wo, i), N = ld3(c.N, i), T = ld3(c.T, i);
        float kr = ldg(c.KsColor.r, i), kg = ldg(c.KsColor.g, i), kb = ldg(c.KsColor.b, i);
        float rough = ldg(c.specularRoughness.v, i);
        float ior = ldg(c.ior.v, i);
        float aniso = ldg(c.anisotropic.v, i);
        bool exiting = c.exiting ? (c.exiting[i.full()] != 0) : false;
        Ggx g = ggx_make(wo, N, T, exiting, kr, kg, kb, ior, rough, aniso);

        float rx = ldg(a.rx, i), ry = ldg(a.ry, i);
        VndfView w = vndf_view(g.view, g.fr, g.ax, g.ay);
        float rx2 = ldg(a.rx2, i), ry2 = ldg(a.ry2, i);
        V3 M, M2;
        if (full)
            vndf_microfacet_pair_wg(sh, round, (uint32_t)(base / rlsh::kBlock), w, g.fr, rx, ry, rx2, ry2, M, M2);
        else
            vndf_microfacet_pair(w, g.fr, rx, ry, w, g.fr, rx2, ry2, M, M2);
        V3 L = reflect_direction(g.view, M);
        float F = ggx_fresnel(g, L, M);
        {
            const GgxIO b = reload_args(a0);
            st3(b.wi, i, L);
            if (b.fresnel) stg(b.fresnel, i, F);
        }
        {
            float fr, fg, fb, pdf;
            ggx_eval_pdf<true, true>(g, L, fr, fg, fb, pdf);
            const GgxIO b = reload_args(a0);
            strgb(b.f, i, fr, fg, fb);
            stg(b.pdf, i, pdf);
        }
        {
            V3 dir;
            ggx_refract(g, M2, dir);
            const float wgt = ggx_sample_weight(g, g.view, dir, M2);
            const GgxIO b = reload_args(a0);
            st3(b.wt, i, dir);
            stg(b.weight, i, wgt);
        }
    }
}

} // namespace

// the one export: what launch_kernel<OP_REFLECT_REFRACT> of csrc/ggx.hip launches for a streamed closure in EXACT mode.
// Same grid as the kernel it stands in for; a failed launch is reported through the product library's error state.
extern "C" rls_status rls_ggx_rr_wg_launch(rls_context *ctx, const rlsh::GgxIO *io, const char *name)
{
    hipLaunchKernelGGL(ggx_rr_wg_kernel, rlsh::grid_for(ctx, io->n, rlsh::kBlock, RLS_CAP_MULT), dim3(rlsh::kBlock), 0,
                       ctx->stream, *io);
    return rlsh::check_launch(name, 0);
}
