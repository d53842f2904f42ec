// lights.hip -- the light loops of rlGgx and rlDisney (src/rlGgx.cpp:274-299,
// src/rlDisney.cpp:695-705): two-sample MIS over up to eight spherical lights per shading point.  The loops are
// rls_loops.hpp (ggx_direct_loops, disney_direct_loops); this unit holds the kernels and the C-ABI entry points
// rls_ggx_direct_lighting / rls_disney_direct_lighting.  VALU-bound.
#include "rls_loops.hpp"

namespace {

template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_INT_ATTR void ggx_direct_kernel(LightIO a)
{
    __shared__ uint32_t tab[2][kMaxSpp];
    __shared__ SlowLds<RLS_SPEC_BLOCK> slow;
    stage_libm_tables();   // atanf range table (+ expf / logf / powf tables) -> LDS
    stage_table(tab, a.spp);
    RLS_POINT_WALK(G, a.n)
    const float inv = 1.0f / (float)a.spp;
    for (int64_t it = 0, i = first; it < rounds; it++, i += stride) {
        const bool live = i < a.n;
        const int64_t ii = live ? i : a.n - 1;
        RLS_GGX_LOAD(g, a.c, ii)
        VndfView w = vndf_view(g.view, g.fr, g.ax, g.ay);
        OrenNayar on = oren_nayar_make(N, ldp(a.sh.diffuseRoughness, pk));
        const float ks = ldp(a.sh.Ks, pk), kd = ldp(a.sh.Kd, pk);
        float dr, dg, db;
        ldrgb(a.sh.KdColor, pk, dr, dg, db);
        dr *= kd; dg *= kd; db *= kd;                                       // diffuseColor, src/rlGgx.cpp:279
        float oD[3], oS[3];
        ggx_direct_loops<G>(slow, g, w, on, wo, N, ld3(a.P, ii), !color_is_small(dr, dg, db), a, tab, a.spp, sub,
                            inv, a.seed, a.first + (uint64_t)ii, oD, oS);
        if (live && sub == 0) {
            strgb(a.ds, i, oS[0] * ks, oS[1] * ks, oS[2] * ks);            // specular *= specularWeight, :305
            strgb(a.dd, i, oD[0] * dr, oD[1] * dg, oD[2] * db);            // diffuse *= diffuseColor, :304
        }
    }
}

template <int G, int FAST_MATH = RLS_FAST>
__global__ RLS_DISNEY_LIGHT_ATTR void disney_direct_kernel(DisneyLightIO a)
{
    __shared__ uint32_t tab[2][kMaxSpp];
    __shared__ SlowLds<RLS_SPEC_BLOCK> slow;
    stage_libm_tables();
    stage_table(tab, a.spp);
    RLS_POINT_WALK(G, a.n)
    const float inv = 1.0f / (float)a.spp;
    for (int64_t it = 0, i = first; it < rounds; it++, i += stride) {
        const bool live = i < a.n;
        const int64_t ii = live ? i : a.n - 1;
        RLS_DISNEY_LOAD(d, a.c, ii)
        VndfView w = vndf_view(d.view, d.fr, d.ax, d.ay);
        float oD[3], oS[3];
        disney_direct_loops<G>(slow, d, w, d.fr.N, ld3(a.P, ii), a, tab, a.spp, sub, inv, a.seed,
                               a.first + (uint64_t)ii, oD, oS);
        if (live && sub == 0) {
            strgb(a.dd, i, oD[0], oD[1], oD[2]);
            strgb(a.ds, i, oS[0], oS[1], oS[2]);
        }
    }
}

rls_status launch_ggx_direct(rls_context *ctx, int g, const LightIO &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(ggx_direct_kernel), g, io, name);
}
rls_status launch_disney_direct(rls_context *ctx, int g, const DisneyLightIO &io, const char *name)
{
    return launch_g(ctx, RLS_G_FAMILY(disney_direct_kernel), g, io, name);
}

} // namespace

RLS_FLAVOURS(ggx_direct, rlsh::LightIO)
RLS_FLAVOURS(disney_direct, rlsh::DisneyLightIO)

#if !RLS_FAST

extern "C" {

rls_status rls_ggx_direct_lighting(rls_context *ctx, int64_t n, const rls_ggx_closure *c, const rls_ggx_shader *sh,
                                   rls_cvec3 P, const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                   uint64_t first_index, rls_rgb direct_diffuse, rls_rgb direct_specular)
{
    RLS_LOOP_PROLOGUE(spp_n);
    RLS_REQUIRE(c != nullptr && sh != nullptr, "closure or shader is NULL");
    if (rls_status s = rlsh::check_closure(__func__, c, &P, sh)) return s;
    RLS_REQUIRE(rlsh::has3(direct_diffuse) && rlsh::has3(direct_specular), "NULL output plane");
    LightIO io = {};
    if (rls_status st = copy_lights(lights, n_lights, 1, io.lights, &io.nl)) return st;
    io.c = *c; io.sh = *sh; io.P = P; io.dd = direct_diffuse; io.ds = direct_specular;
    set_loop(io, n, spp_n, seed, first_index);
    return dispatch_ggx_direct(ctx, pick_group(ctx, n, io.spp), io, "rls_ggx_direct_lighting");
}

rls_status rls_disney_direct_lighting(rls_context *ctx, int64_t n, const rls_disney_closure *c, rls_cvec3 P,
                                      const rls_sphere_light *lights, int n_lights, int spp_n, uint32_t seed,
                                      uint64_t first_index, rls_rgb direct_diffuse, rls_rgb direct_specular)
{
    RLS_LOOP_PROLOGUE(spp_n);
    if (rls_status s = rlsh::check_closure(__func__, c, &P)) return s;
    RLS_REQUIRE(rlsh::has3(direct_diffuse) && rlsh::has3(direct_specular), "NULL output plane");
    DisneyLightIO io = {};
    if (rls_status st = copy_lights(lights, n_lights, 1, io.lights, &io.nl)) return st;
    io.c = *c; io.P = P; io.dd = direct_diffuse; io.ds = direct_specular;
    set_loop(io, n, spp_n, seed, first_index);
    return dispatch_disney_direct(ctx, pick_group(ctx, n, io.spp), io, "rls_disney_direct_lighting");
}

} // extern "C"

#endif // !RLS_FAST
