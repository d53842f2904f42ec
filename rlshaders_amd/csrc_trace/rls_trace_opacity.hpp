// rls_trace_opacity.hpp -- shadow rays' hits (part of trace.hip, included there inside its anonymous namespace, last): the
// opacity each node's shader_evaluate returns (rls_trace_ggx_opacity / _disney_opacity / _skin_opacity) and the fold of the
// opacities along a shadow ray into the visibility the resolves read (rls_trace_shadow_visibility).  Products, differences and
// comparisons only, each rounded by itself (-ffp-contract=off): mode-free, in the EXACT unit like state_advance_kernel, one
// point or ray per lane, grid-striding.

#if !RLS_FAST
struct GgxOpacityIO {
    rls_ggx_opacity p;
    const uint8_t *ray_type;     // NULL: no point is a shadow ray's
    rls_rgb out;
    int64_t n;
};
struct DisneyOpacityIO {
    rls_disney_opacity p;
    const uint8_t *ray_type;
    rls_rgb out;
    int64_t n;
};
struct SkinOpacityIO {
    rls_skin_opacity p;
    const uint8_t *ray_type;
    rls_crgb incoming;           // all NULL: 1
    rls_rgb out;
    int64_t n;
};
struct ShadowFoldIO {
    rls_shadow_hits h;
    rls_crgb base;               // all NULL: 1
    rls_rgb vis;
    int64_t rays;
};

// AiColorClamp(c, 0, 1) per channel: the stand-in's MAX(0, MIN(v, 1)) with a < b ? a : b and a > b ? a : b.  clampf
// (rls_device.hpp) is maxf(lo, minf(v, hi)) over exactly those two selects: a NaN gives 1, -0 stays -0.
__device__ __forceinline__ float clamp01(float v) { return clampf(v, 0.0f, 1.0f); }
__device__ __forceinline__ bool shadow_point(const uint8_t *ray_type, int64_t i)
{
    return ray_type != nullptr && (ray_type[i] & RLS_RT_SHADOW) != 0;
}

// rlGgx: a shadow ray's point WHITE - KtColor * Kt (src/rlGgx.cpp:264-268), any other AiColorClamp(opacity * opacity_color)
// (:250, :326).  A point reads the parameters of its own branch only.
__global__ __launch_bounds__(rlsh::kBlock) void ggx_opacity_kernel(GgxOpacityIO a)
{
    for (int64_t i = (int64_t)blockIdx.x * rlsh::kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * rlsh::kBlock) {
        const auto k = pindex(a.p.materials, i);
        float r, g, b;
        if (shadow_point(a.ray_type, i)) {
            ldrgb(a.p.KtColor, k, r, g, b);
            const float kt = ldp(a.p.Kt, k);
            r = 1.0f - (r * kt); g = 1.0f - (g * kt); b = 1.0f - (b * kt);
        } else {
            ldrgb(a.p.opacity_color, k, r, g, b);
            const float o = ldp(a.p.opacity, k);
            r = clamp01(o * r); g = clamp01(o * g); b = clamp01(o * b);
        }
        strgb(a.out, i, r, g, b);
    }
}

// rlDisney: a shadow ray's point the opacity as it is (src/rlDisney.cpp:685-687), any other AiColorClamp(opacity) (:728)
__global__ __launch_bounds__(rlsh::kBlock) void disney_opacity_kernel(DisneyOpacityIO a)
{
    for (int64_t i = (int64_t)blockIdx.x * rlsh::kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * rlsh::kBlock) {
        float r, g, b;
        ldrgb(a.p.opacity, pindex(a.p.materials, i), r, g, b);
        if (!shadow_point(a.ray_type, i)) { r = clamp01(r); g = clamp01(g); b = clamp01(b); }
        strgb(a.out, i, r, g, b);
    }
}

// rlSkin: AiColorClamp(opacity * opacity_color) (src/rlSkin.cpp:167, :255), at a shadow ray's point multiplied into the
// sg->out_opacity the node found (:169-172).  incoming may be the output: a lane reads its element before it writes it.
__global__ __launch_bounds__(rlsh::kBlock) void skin_opacity_kernel(SkinOpacityIO a)
{
    for (int64_t i = (int64_t)blockIdx.x * rlsh::kBlock + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * rlsh::kBlock) {
        const auto k = pindex(a.p.materials, i);
        float r, g, b;
        ldrgb(a.p.opacity_color, k, r, g, b);
        const float o = ldp(a.p.opacity, k);
        r = clamp01(o * r); g = clamp01(o * g); b = clamp01(o * b);
        if (a.incoming.r != nullptr && shadow_point(a.ray_type, i)) {
            r = a.incoming.r[i] * r; g = a.incoming.g[i] * g; b = a.incoming.b[i] * b;
        }
        strgb(a.out, i, r, g, b);
    }
}

// The fold: one ray per lane; slot k of the wavefront's 64 rays is 64 consecutive elements of each plane (e = k * stride + j),
// so every slot's loads are coalesced (the indexed form gathers from the table after one coalesced load of the indices).  The
// k loop is per lane: a wavefront leaves it when none of its lanes has count > k, and a lane past its own count is masked off,
// so no element beyond a ray's count is read.  No clamp, no early exit: T = T * (1 - o), three plain products a hit.
__global__ __launch_bounds__(rlsh::kBlock) void shadow_visibility_kernel(ShadowFoldIO a)
{
    const int64_t stride = a.h.stride;
    const uint32_t last = a.h.table_count - 1u;
    for (int64_t j = (int64_t)blockIdx.x * rlsh::kBlock + threadIdx.x; j < a.rays; j += (int64_t)gridDim.x * rlsh::kBlock) {
        float r = 1.0f, g = 1.0f, b = 1.0f;
        if (a.base.r != nullptr) { r = a.base.r[j]; g = a.base.g[j]; b = a.base.b[j]; }
        const int hits = a.h.count[j];
        const int count = hits < a.h.max_hits ? hits : a.h.max_hits;
        for (int k = 0; k < count; k++) {
            int64_t e = (int64_t)k * stride + j;
            if (a.h.index != nullptr) {
                const uint32_t t = a.h.index[e];
                e = t < last ? t : last;
            }
            r = r * (1.0f - a.h.opacity.r[e]);
            g = g * (1.0f - a.h.opacity.g[e]);
            b = b * (1.0f - a.h.opacity.b[e]);
        }
        strgb(a.vis, j, r, g, b);
    }
}
#endif
