// argument_checks.cpp -- the argument checks of every closure and loop entry point of librlshaders_amd.so and of the four
// calls of librls_trace.so, driven with dummy planes and no GPU (tests/test_argument_checks.py builds and runs it).
//
// Every case starts from a set of arguments that passes every check, breaks one of them (or none) and records what the
// call returns.  A call whose arguments pass reaches the launch, and with no device there its hipSetDevice fails: status
// RLS_ERR_HIP.  So a check that goes missing shows up as a wrong status, not as a crash -- but only while no device is
// visible: on a GPU the dummy planes would reach a kernel.  The driver refuses to run if HIP reports a device.
//
// Output: one tab-separated line per case and math mode:
//   entry  case  fast  status  expected-status  expected-prefix  expected-text  message
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <functional>
#include <string>
#include <vector>

#include "../../rlshaders_amd/csrc/rls_internal.hpp"
#include "../../include/rlshaders_amd_trace.h"

namespace {

float g_plane[64];                      // the stand-in for every device plane: never dereferenced without a device
uint32_t g_ids[4];
uint8_t g_bytes[4];
int64_t g_offsets[4];
float *const D = g_plane;

rls_cvec3 cv() { return { D, D, D }; }
rls_vec3 v3() { return { D, D, D }; }
rls_rgb rgb() { return { D, D, D }; }
rls_param par() { return { D, 0.0f }; }
rls_param_rgb prgb() { return { D, D, D, 0.0f, 0.0f, 0.0f }; }

int chunk_consumer(void *, int64_t, int64_t, const rls_disney_stream_out *) { return 0; }

// every argument any entry point takes, valid as constructed
struct World {
    rls_context context;
    rls_context *ctx;
    int64_t n;
    int spp_n;
    int e;                                   // the enum argument: kernel, lobe, kind, fn
    rls_ggx_closure gc;
    rls_disney_closure dc;
    rls_sss_closure sc;
    rls_skin_closure kc;
    const rls_ggx_closure *gp;
    const rls_disney_closure *dp;
    const rls_sss_closure *sp;
    const rls_skin_closure *kp;
    rls_ggx_shader sh;
    const rls_ggx_shader *shp;
    rls_cvec3 P, a, b, c;                    // input vec3 planes
    rls_vec3 v, v2;                          // output vec3 planes
    rls_rgb f, f2;                           // output rgb planes
    const float *x, *y, *x2, *y2;            // input scalar planes
    float *o1, *o2, *o3;                     // output scalar planes
    uint8_t *u8;
    rls_param dist;
    rls_sphere_light lights[2];
    const rls_sphere_light *lp;
    int n_lights;
    float env[3];
    const float *envp;
    rls_sss_scene scene;
    const rls_sss_scene *scenep;
    const float *xi[6];
    const float *const *xip;
    rls_skin_out ko;
    const rls_skin_out *kop;
    rls_skin_integrate_out kio;
    const rls_skin_integrate_out *kiop;
    rls_ggx_shade_out gso;
    const rls_ggx_shade_out *gsop;
    rls_disney_shade_out dso;
    const rls_disney_shade_out *dsop;
    rls_disney_stream_out st;
    const rls_disney_stream_out *stp;
    int64_t chunk_points;
    rls_disney_chunk_fn consume;
    rls_ray_queue q;
    const rls_ray_queue *qp;
    rls_crgb L;

    explicit World(int fast)
    {
        context = {};
        context.device = 0;
        context.compute_units = 256;
        context.blocks_per_cu = 64;
        context.fast = fast;
        ctx = &context;
        n = 1000;
        spp_n = 4;
        e = 0;
        gc = {};
        gc.wo = cv(); gc.N = cv(); gc.T = cv(); gc.KsColor = prgb();
        gc.specularRoughness = par(); gc.ior = par(); gc.anisotropic = par();
        gc.materials = { g_ids, 4 };
        dc = {};
        dc.wo = cv(); dc.N = cv(); dc.T = cv(); dc.base_color = prgb(); dc.roughness = par();
        dc.materials = { g_ids, 4 };
        sc = {};
        sc.sss_color = prgb(); sc.sss_dist_multiplier = par(); sc.N = cv(); sc.T = cv();
        sc.materials = { g_ids, 4 };
        kc = {};
        kc.wo = cv(); kc.N = cv(); kc.T = cv();
        kc.sss_color = prgb(); kc.specular_color = prgb(); kc.sheen_color = prgb();
        kc.materials = { g_ids, 4 };
        gp = &gc; dp = &dc; sp = &sc; kp = &kc;
        sh = {};
        sh.KdColor = prgb(); sh.KtColor = prgb();
        shp = &sh;
        P = a = b = c = cv();
        v = v2 = v3();
        f = f2 = rgb();
        x = y = x2 = y2 = D;
        o1 = o2 = o3 = D;
        u8 = g_bytes;
        dist = par();
        for (rls_sphere_light &l : lights) l = { { 0.0f, 0.0f, 0.0f }, 1.0f, { 1.0f, 1.0f, 1.0f }, RLS_MIS_BOTH };
        lp = lights;
        n_lights = 2;
        env[0] = env[1] = env[2] = 1.0f;
        envp = env;
        scene = {};
        scene.geometry = RLS_SCENE_SPHERE;
        scenep = &scene;
        for (const float *&p : xi) p = D;
        xip = xi;
        ko = { v3(), rgb(), D, D, v3(), rgb(), D, D, D, D, rgb(), D, D, D };
        kop = &ko;
        kio = { rgb(), rgb(), rgb(), rgb(), D, D, D };
        kiop = &kio;
        gso = { rgb(), rgb(), rgb(), rgb(), rgb(), rgb() };
        gsop = &gso;
        dso = { rgb(), rgb(), rgb(), rgb(), rgb() };
        dsop = &dso;
        st = { v3(), rgb(), D };
        stp = &st;
        chunk_points = 100;
        consume = chunk_consumer;
        q = {};
        q.capacity = (int64_t)1 << 40;
        q.offsets = g_offsets;
        q.dir = v3(); q.weight = rgb();
        q.scratch = g_plane;
        q.scratch_bytes = SIZE_MAX;
        qp = &q;
        L = { D, D, D };
    }
};

typedef std::function<rls_status(World &)> Call;
typedef std::function<void(World &)> Break;

struct Case {
    std::string entry, what;
    Call call;
    Break brk;
    int status;
    std::string prefix, text;              // for RLS_ERR_INVALID_ARGUMENT / RLS_ERR_UNSUPPORTED: "<prefix>: <text>"
};
std::vector<Case> g_cases;

const int BAD = RLS_ERR_INVALID_ARGUMENT, HIP = RLS_ERR_HIP;

struct Verb {
    std::string name;
    Call call;
    std::string prefix;                    // the function RLS_REQUIRE names (the entry point itself but where noted)

    // one case: break `brk`, expect `status` (and for a refused argument "<prefix>: <text>")
    const Verb &on(const char *what, Break brk, int status, const char *text = "", const char *pfx = nullptr) const
    {
        g_cases.push_back({ name, what, call, brk, status, pfx ? pfx : prefix, text });
        return *this;
    }
    // ctx, n < 0, the arguments as constructed, and n == 0 with nothing else wrong
    const Verb &basics() const
    {
        on("valid", [](World &) {}, HIP);
        on("ctx NULL", [](World &w) { w.ctx = nullptr; }, BAD, "ctx is NULL");
        on("n < 0", [](World &w) { w.n = -1; }, BAD, "n < 0");
        return on("n == 0", [](World &w) { w.n = 0; }, RLS_OK);
    }
    // spp_n outside [1, 16]; checked before the n == 0 return, so an empty batch with a bad spp_n is refused too
    const Verb &spp() const
    {
        on("spp_n 0", [](World &w) { w.spp_n = 0; }, BAD, "spp_n must be in [1, 16]");
        on("spp_n 17", [](World &w) { w.spp_n = 17; }, BAD, "spp_n must be in [1, 16]");
        return on("n == 0, spp_n 0", [](World &w) { w.n = 0; w.spp_n = 0; }, BAD, "spp_n must be in [1, 16]");
    }
    // the lights of a light loop (copy_lights): at_least = 1 for the light loops, 0 for the whole-shader verbs
    const Verb &lights(int at_least) const
    {
        const char *range = "n_lights out of range (RLS_MAX_LIGHTS)";
        on("n_lights 9", [](World &w) { w.n_lights = 9; }, BAD, range, "copy_lights");
        on("n_lights -1", [](World &w) { w.n_lights = -1; }, BAD, range, "copy_lights");
        if (at_least == 1) on("n_lights 0", [](World &w) { w.n_lights = 0; }, BAD, range, "copy_lights");
        else on("n_lights 0, lights NULL", [](World &w) { w.n_lights = 0; w.lp = nullptr; }, HIP);
        on("lights NULL", [](World &w) { w.lp = nullptr; }, BAD, "lights is NULL", "copy_lights");
        on("unknown mis_mode", [](World &w) { w.lights[1].mis_mode = 3; }, BAD, "unknown mis_mode", "copy_lights");
        return on("light radius 0", [](World &w) { w.lights[1].radius = 0.0f; }, BAD, "light radius must be positive",
                  "copy_lights");
    }
};

Verb verb(const char *name, Call call, const char *prefix = nullptr) { return Verb{ name, call, prefix ? prefix : name }; }

const char *const MATERIALS = "materials.id is set but materials.count is 0";

// the rlGgx closure's checks; null / frame / colour: the verb's message for each (it may name more arguments)
void ggx_closure(const Verb &v, const char *null = "closure is NULL", const char *frame = "wo/N/T plane is NULL",
                 const char *colour = "KsColor planes must be all set or all NULL")
{
    v.on("closure NULL", [](World &w) { w.gp = nullptr; }, BAD, null)
     .on("wo NULL", [](World &w) { w.gc.wo.x = nullptr; }, BAD, frame)
     .on("N NULL", [](World &w) { w.gc.N.y = nullptr; }, BAD, frame)
     .on("T NULL", [](World &w) { w.gc.T.z = nullptr; }, BAD, frame)
     .on("KsColor mixed NULL", [](World &w) { w.gc.KsColor.g = nullptr; }, BAD, colour)
     .on("KsColor uniform", [](World &w) { w.gc.KsColor.r = w.gc.KsColor.g = w.gc.KsColor.b = nullptr; }, HIP)
     .on("materials.count 0", [](World &w) { w.gc.materials.count = 0; }, BAD, MATERIALS)
     .on("no materials", [](World &w) { w.gc.materials = {}; }, HIP);
}
void disney_closure(const Verb &v, const char *null = "closure is NULL", const char *frame = "wo/N/T plane is NULL")
{
    const char *colour = "base_color planes must be all set or all NULL";
    v.on("closure NULL", [](World &w) { w.dp = nullptr; }, BAD, null)
     .on("wo NULL", [](World &w) { w.dc.wo.y = nullptr; }, BAD, frame)
     .on("N NULL", [](World &w) { w.dc.N.z = nullptr; }, BAD, frame)
     .on("T NULL", [](World &w) { w.dc.T.x = nullptr; }, BAD, frame)
     .on("base_color mixed NULL", [](World &w) { w.dc.base_color.b = nullptr; }, BAD, colour)
     .on("materials.count 0", [](World &w) { w.dc.materials.count = 0; }, BAD, MATERIALS);
}
// frame: the verb's N/T message, or NULL where it takes no frame
void sss_closure(const Verb &v, const char *frame, const char *null = "closure is NULL")
{
    v.on("closure NULL", [](World &w) { w.sp = nullptr; }, BAD, null)
     .on("sss_color mixed NULL", [](World &w) { w.sc.sss_color.r = nullptr; }, BAD, "sss_color planes must be all set or all NULL")
     .on("materials.count 0", [](World &w) { w.sc.materials.count = 0; }, BAD, MATERIALS)
     .on("sss_color NULL, materials.count 0", [](World &w) { w.sc.sss_color.r = nullptr; w.sc.materials.count = 0; }, BAD,
         "sss_color planes must be all set or all NULL");
    if (frame)
        v.on("N NULL", [](World &w) { w.sc.N.x = nullptr; }, BAD, frame).on("T NULL", [](World &w) { w.sc.T.y = nullptr; }, BAD, frame);
    else
        v.on("no frame", [](World &w) { w.sc.N = {}; w.sc.T = {}; }, HIP);
}
void skin_closure(const Verb &v, const char *null, const char *frame)
{
    const char *colour = "colour planes must be all set or all NULL";
    v.on("closure NULL", [](World &w) { w.kp = nullptr; }, BAD, null)
     .on("wo NULL", [](World &w) { w.kc.wo.x = nullptr; }, BAD, frame)
     .on("T NULL", [](World &w) { w.kc.T.z = nullptr; }, BAD, frame)
     .on("sss_color mixed NULL", [](World &w) { w.kc.sss_color.g = nullptr; }, BAD, colour)
     .on("specular_color mixed NULL", [](World &w) { w.kc.specular_color.b = nullptr; }, BAD, colour)
     .on("sheen_color mixed NULL", [](World &w) { w.kc.sheen_color.r = nullptr; }, BAD, colour)
     .on("materials.count 0", [](World &w) { w.kc.materials.count = 0; }, BAD, MATERIALS);
}
// an empty batch is done before the closure is looked at
void empty_before_closure(const Verb &v)
{
    v.on("n == 0, closure NULL", [](World &w) { w.n = 0; w.gp = nullptr; w.dp = nullptr; w.sp = nullptr; w.kp = nullptr; }, RLS_OK);
}

void ggx_verbs()
{
    Verb v = verb("rls_ggx_sample", [](World &w) { return rls_ggx_sample(w.ctx, w.n, w.gp, w.x, w.y, w.v, w.o1); });
    v.basics().on("rx NULL", [](World &w) { w.x = nullptr; }, BAD, "rx/ry is NULL")
     .on("ry NULL", [](World &w) { w.y = nullptr; }, BAD, "rx/ry is NULL")
     .on("wi NULL", [](World &w) { w.v.y = nullptr; }, BAD, "wi plane is NULL")
     .on("fresnel NULL", [](World &w) { w.o1 = nullptr; }, HIP);
    ggx_closure(v); empty_before_closure(v);

    v = verb("rls_ggx_eval", [](World &w) { return rls_ggx_eval(w.ctx, w.n, w.gp, w.a, w.f); });
    v.basics().on("wi NULL", [](World &w) { w.a.z = nullptr; }, BAD, "wi/f plane is NULL")
     .on("f NULL", [](World &w) { w.f.g = nullptr; }, BAD, "wi/f plane is NULL");
    ggx_closure(v); empty_before_closure(v);

    v = verb("rls_ggx_pdf", [](World &w) { return rls_ggx_pdf(w.ctx, w.n, w.gp, w.a, w.o1); });
    v.basics().on("wi NULL", [](World &w) { w.a.x = nullptr; }, BAD, "wi/pdf is NULL")
     .on("pdf NULL", [](World &w) { w.o1 = nullptr; }, BAD, "wi/pdf is NULL");
    ggx_closure(v); empty_before_closure(v);

    v = verb("rls_ggx_sample_eval_pdf",
             [](World &w) { return rls_ggx_sample_eval_pdf(w.ctx, w.n, w.gp, w.x, w.y, w.v, w.f, w.o1, w.o2); });
    v.basics().on("rx NULL", [](World &w) { w.x = nullptr; }, BAD, "rx/ry is NULL")
     .on("wi NULL", [](World &w) { w.v.x = nullptr; }, BAD, "wi/f/pdf is NULL")
     .on("f NULL", [](World &w) { w.f.b = nullptr; }, BAD, "wi/f/pdf is NULL")
     .on("pdf NULL", [](World &w) { w.o1 = nullptr; }, BAD, "wi/f/pdf is NULL")
     .on("fresnel NULL", [](World &w) { w.o2 = nullptr; }, HIP);
    ggx_closure(v); empty_before_closure(v);

    v = verb("rls_ggx_refract_sample",
             [](World &w) { return rls_ggx_refract_sample(w.ctx, w.n, w.gp, w.x, w.y, w.v, w.o1, w.u8); });
    v.basics().on("ry NULL", [](World &w) { w.y = nullptr; }, BAD, "rx/ry is NULL")
     .on("wt NULL", [](World &w) { w.v.z = nullptr; }, BAD, "wt/weight is NULL")
     .on("weight NULL", [](World &w) { w.o1 = nullptr; }, BAD, "wt/weight is NULL")
     .on("refracted NULL", [](World &w) { w.u8 = nullptr; }, HIP);
    ggx_closure(v); empty_before_closure(v);

    v = verb("rls_ggx_reflect_refract", [](World &w) {
        return rls_ggx_reflect_refract(w.ctx, w.n, w.gp, w.x, w.y, w.x2, w.y2, w.v, w.f, w.o1, w.o2, w.v2, w.o3);
    });
    v.basics().on("rx NULL", [](World &w) { w.x = nullptr; }, BAD, "random-number plane is NULL")
     .on("ry2 NULL", [](World &w) { w.y2 = nullptr; }, BAD, "random-number plane is NULL")
     .on("wi NULL", [](World &w) { w.v.y = nullptr; }, BAD, "wi/f/pdf is NULL")
     .on("f NULL", [](World &w) { w.f.r = nullptr; }, BAD, "wi/f/pdf is NULL")
     .on("pdf NULL", [](World &w) { w.o1 = nullptr; }, BAD, "wi/f/pdf is NULL")
     .on("fresnel NULL", [](World &w) { w.o2 = nullptr; }, HIP)
     .on("wt NULL", [](World &w) { w.v2.x = nullptr; }, BAD, "wt/weight is NULL")
     .on("weight NULL", [](World &w) { w.o3 = nullptr; }, BAD, "wt/weight is NULL")
     .on("all parameters streamed, no materials", [](World &w) { w.gc.materials = {}; }, HIP);
    ggx_closure(v); empty_before_closure(v);

    v = verb("rls_ggx_microfacet",
             [](World &w) { return rls_ggx_microfacet(w.ctx, w.n, w.gp, w.e, w.x, w.y, w.v); });
    v.basics().on("kernel NDF", [](World &w) { w.e = RLS_KERNEL_NDF; }, HIP)
     .on("unknown kernel", [](World &w) { w.e = 2; }, BAD, "unknown sampling kernel")
     .on("unknown kernel, rx NULL", [](World &w) { w.e = -1; w.x = nullptr; }, BAD, "unknown sampling kernel")
     .on("rx NULL", [](World &w) { w.x = nullptr; }, BAD, "rx/ry is NULL")
     .on("m NULL", [](World &w) { w.v.z = nullptr; }, BAD, "m plane is NULL")
     .on("closure NULL, unknown kernel", [](World &w) { w.gp = nullptr; w.e = 2; }, BAD, "closure is NULL");
    ggx_closure(v); empty_before_closure(v);

    v = verb("rls_ggx_ndf_pdf", [](World &w) { return rls_ggx_ndf_pdf(w.ctx, w.n, w.gp, w.a, w.o1); });
    v.basics().on("wi NULL", [](World &w) { w.a.y = nullptr; }, BAD, "wi/pdf is NULL")
     .on("pdf NULL", [](World &w) { w.o1 = nullptr; }, BAD, "wi/pdf is NULL");
    ggx_closure(v); empty_before_closure(v);

    v = verb("rls_ggx_integrate",
             [](World &w) { return rls_ggx_integrate(w.ctx, w.n, w.gp, w.spp_n, 7u, 0u, w.f, w.o1); });
    v.basics().spp().on("sum NULL", [](World &w) { w.f.b = nullptr; }, BAD, "NULL output plane")
     .on("avg_reflect_weight NULL", [](World &w) { w.o1 = nullptr; }, BAD, "NULL output plane");
    ggx_closure(v); empty_before_closure(v);

    v = verb("rls_ggx_integrate_refract", [](World &w) {
        return rls_ggx_integrate_refract(w.ctx, w.n, w.gp, 1, w.envp, w.spp_n, 7u, 0u, w.f, w.o1);
    });
    v.basics().spp().on("env NULL", [](World &w) { w.envp = nullptr; }, BAD, "closure or env is NULL")
     .on("result NULL", [](World &w) { w.f.g = nullptr; }, BAD, "NULL output plane")
     .on("tir_fraction NULL", [](World &w) { w.o1 = nullptr; }, HIP);
    ggx_closure(v, "closure or env is NULL"); empty_before_closure(v);
    verb("rls_ggx_integrate_refract", [](World &w) {
        return rls_ggx_integrate_refract(w.ctx, w.n, w.gp, 0, w.envp, w.spp_n, 7u, 0u, w.f, w.o1);
    }).on("untraced", [](World &) {}, HIP).on("untraced, spp_n 17", [](World &w) { w.spp_n = 17; }, BAD, "spp_n must be in [1, 16]");

    v = verb("rls_ggx_direct_lighting", [](World &w) {
        return rls_ggx_direct_lighting(w.ctx, w.n, w.gp, w.shp, w.P, w.lp, w.n_lights, w.spp_n, 7u, 0u, w.f, w.f2);
    });
    v.basics().spp().lights(1)
     .on("shader NULL", [](World &w) { w.shp = nullptr; }, BAD, "closure or shader is NULL")
     .on("P NULL", [](World &w) { w.P.y = nullptr; }, BAD, "wo/N/T/P plane is NULL")
     .on("KdColor mixed NULL", [](World &w) { w.sh.KdColor.b = nullptr; }, BAD, "colour planes must be all set or all NULL")
     .on("direct_diffuse NULL", [](World &w) { w.f.r = nullptr; }, BAD, "NULL output plane")
     .on("direct_specular NULL", [](World &w) { w.f2.b = nullptr; }, BAD, "NULL output plane")
     .on("direct_specular NULL, lights NULL", [](World &w) { w.f2.b = nullptr; w.lp = nullptr; }, BAD, "NULL output plane");
    ggx_closure(v, "closure or shader is NULL", "wo/N/T/P plane is NULL", "colour planes must be all set or all NULL");
    empty_before_closure(v);

    v = verb("rls_ggx_shade", [](World &w) {
        return rls_ggx_shade(w.ctx, w.n, w.gp, w.shp, w.P, w.lp, w.n_lights, w.envp, 1, w.spp_n, 7u, 0u, w.gsop);
    });
    const char *null = "closure, shader, env or out is NULL";
    v.basics().spp().lights(0)
     .on("shader NULL", [](World &w) { w.shp = nullptr; }, BAD, null)
     .on("env NULL", [](World &w) { w.envp = nullptr; }, BAD, null)
     .on("out NULL", [](World &w) { w.gsop = nullptr; }, BAD, null)
     .on("P NULL", [](World &w) { w.P.z = nullptr; }, BAD, "wo/N/T/P plane is NULL")
     .on("KdColor mixed NULL", [](World &w) { w.sh.KdColor.g = nullptr; }, BAD, "colour planes must be all set or all NULL")
     .on("KtColor mixed NULL", [](World &w) { w.sh.KtColor.r = nullptr; }, BAD, "colour planes must be all set or all NULL")
     .on("refraction NULL", [](World &w) { w.gso.refraction.g = nullptr; }, BAD, "NULL AOV plane")
     .on("indirect_specular NULL", [](World &w) { w.gso.indirect_specular.b = nullptr; }, BAD, "NULL AOV plane")
     .on("out mixed NULL", [](World &w) { w.gso.out.g = nullptr; }, BAD, "out planes must be all set or all NULL")
     .on("out NULL", [](World &w) { w.gso.out = {}; }, HIP);
    ggx_closure(v, null, "wo/N/T/P plane is NULL", "colour planes must be all set or all NULL");
    empty_before_closure(v);
}

void disney_verbs()
{
    const char *lobe = "lobe must be RLS_RAY_DIFFUSE or RLS_RAY_GLOSSY";
    struct { const char *name; Call call; } pointwise[] = {
        { "rls_disney_sample", [](World &w) { return rls_disney_sample(w.ctx, w.n, w.dp, w.e, w.x, w.y, w.v); } },
        { "rls_disney_eval", [](World &w) { return rls_disney_eval(w.ctx, w.n, w.dp, w.e, w.a, w.f); } },
        { "rls_disney_pdf", [](World &w) { return rls_disney_pdf(w.ctx, w.n, w.dp, w.e, w.a, w.o1); } },
        { "rls_disney_sample_eval_pdf",
          [](World &w) { return rls_disney_sample_eval_pdf(w.ctx, w.n, w.dp, w.e, w.x, w.y, w.v, w.f, w.o1); } },
    };
    for (auto &p : pointwise) {
        Verb v = verb(p.name, [call = p.call](World &w) { w.e = w.e == 0 ? RLS_RAY_DIFFUSE : w.e; return call(w); });
        v.basics().on("glossy", [](World &w) { w.e = RLS_RAY_GLOSSY; }, HIP)
         .on("unknown lobe", [](World &w) { w.e = 1; }, BAD, lobe)
         .on("unknown lobe, wo NULL", [](World &w) { w.e = 1; w.dc.wo.x = nullptr; }, BAD, lobe)
         .on("closure NULL, unknown lobe", [](World &w) { w.e = 1; w.dp = nullptr; }, BAD, "closure is NULL")
         .on("n == 0, unknown lobe", [](World &w) { w.e = 1; w.n = 0; }, RLS_OK);
        disney_closure(v); empty_before_closure(v);
    }
    Verb v = verb("rls_disney_sample", [](World &w) { return rls_disney_sample(w.ctx, w.n, w.dp, RLS_RAY_GLOSSY, w.x, w.y, w.v); });
    v.on("rx NULL", [](World &w) { w.x = nullptr; }, BAD, "rx/ry is NULL")
     .on("wi NULL", [](World &w) { w.v.z = nullptr; }, BAD, "wi plane is NULL");
    v = verb("rls_disney_eval", [](World &w) { return rls_disney_eval(w.ctx, w.n, w.dp, RLS_RAY_GLOSSY, w.a, w.f); });
    v.on("wi NULL", [](World &w) { w.a.z = nullptr; }, BAD, "wi/f plane is NULL")
     .on("f NULL", [](World &w) { w.f.r = nullptr; }, BAD, "wi/f plane is NULL");
    v = verb("rls_disney_pdf", [](World &w) { return rls_disney_pdf(w.ctx, w.n, w.dp, RLS_RAY_DIFFUSE, w.a, w.o1); });
    v.on("wi NULL", [](World &w) { w.a.y = nullptr; }, BAD, "wi/pdf is NULL")
     .on("pdf NULL", [](World &w) { w.o1 = nullptr; }, BAD, "wi/pdf is NULL");
    v = verb("rls_disney_sample_eval_pdf",
             [](World &w) { return rls_disney_sample_eval_pdf(w.ctx, w.n, w.dp, RLS_RAY_GLOSSY, w.x, w.y, w.v, w.f, w.o1); });
    v.on("ry NULL", [](World &w) { w.y = nullptr; }, BAD, "rx/ry is NULL")
     .on("wi NULL", [](World &w) { w.v.x = nullptr; }, BAD, "wi/f/pdf is NULL")
     .on("f NULL", [](World &w) { w.f.g = nullptr; }, BAD, "wi/f/pdf is NULL")
     .on("pdf NULL", [](World &w) { w.o1 = nullptr; }, BAD, "wi/f/pdf is NULL");

    v = verb("rls_disney_alt_sample", [](World &w) { return rls_disney_alt_sample(w.ctx, w.n, w.dp, w.e, w.x, w.y, w.v); });
    v.basics().on("kind GTR2", [](World &w) { w.e = RLS_DISNEY_ALT_GTR2; }, HIP)
     .on("unknown kind", [](World &w) { w.e = 2; }, BAD, "unknown alternate sampler")
     .on("wo NULL, unknown kind", [](World &w) { w.e = 2; w.dc.wo.x = nullptr; }, BAD, "wo/N/T plane is NULL")
     .on("rx NULL", [](World &w) { w.x = nullptr; }, BAD, "NULL plane")
     .on("m NULL", [](World &w) { w.v.y = nullptr; }, BAD, "NULL plane");
    disney_closure(v); empty_before_closure(v);
    v = verb("rls_disney_alt_pdf", [](World &w) { return rls_disney_alt_pdf(w.ctx, w.n, w.dp, w.a, w.o1); });
    v.basics().on("wi NULL", [](World &w) { w.a.x = nullptr; }, BAD, "NULL plane")
     .on("pdf NULL", [](World &w) { w.o1 = nullptr; }, BAD, "NULL plane");
    disney_closure(v); empty_before_closure(v);
    v = verb("rls_disney_d_gtr2", [](World &w) { return rls_disney_d_gtr2(w.ctx, w.n, w.dp, w.a, w.o1); });
    v.basics().on("m NULL", [](World &w) { w.a.z = nullptr; }, BAD, "NULL plane")
     .on("d NULL", [](World &w) { w.o1 = nullptr; }, BAD, "NULL plane");
    disney_closure(v); empty_before_closure(v);

    v = verb("rls_disney_integrate", [](World &w) {
        return rls_disney_integrate(w.ctx, w.n, w.dp, w.spp_n, 7u, 0u, w.f, w.o1, w.f2, w.o2, w.stp);
    });
    v.basics().spp()
     .on("diffuse_sum NULL", [](World &w) { w.f.r = nullptr; }, BAD, "NULL output plane")
     .on("diffuse_count NULL", [](World &w) { w.o1 = nullptr; }, BAD, "NULL output plane")
     .on("specular_sum NULL", [](World &w) { w.f2.g = nullptr; }, BAD, "NULL output plane")
     .on("specular_count NULL", [](World &w) { w.o2 = nullptr; }, BAD, "NULL output plane")
     .on("stream NULL", [](World &w) { w.stp = nullptr; }, HIP)
     .on("stream.wi NULL", [](World &w) { w.st.wi.y = nullptr; }, BAD, "NULL streamed-output plane")
     .on("stream.pdf NULL", [](World &w) { w.st.pdf = nullptr; }, BAD, "NULL streamed-output plane");
    disney_closure(v); empty_before_closure(v);

    v = verb("rls_disney_integrate_chunked", [](World &w) {
        return rls_disney_integrate_chunked(w.ctx, w.n, w.dp, w.spp_n, 7u, 0u, w.f, w.o1, w.f2, w.o2, w.chunk_points, w.stp,
                                            w.consume, nullptr);
    });
    v.basics()
     .on("chunk_points 0", [](World &w) { w.chunk_points = 0; }, BAD, "chunk_points < 1")
     .on("chunk NULL", [](World &w) { w.stp = nullptr; }, BAD, "chunk buffers are NULL")
     .on("n == 0, chunk NULL", [](World &w) { w.n = 0; w.stp = nullptr; }, BAD, "chunk buffers are NULL")
     .on("consumer while capturing", [](World &w) { w.context.capturing = 1; }, RLS_ERR_UNSUPPORTED,
         "a consumer callback cannot be recorded into a launch graph")
     .on("closure NULL", [](World &w) { w.dp = nullptr; }, BAD, "closure is NULL")
     .on("n == 0, closure NULL", [](World &w) { w.n = 0; w.dp = nullptr; }, RLS_OK)
     .on("n == 0, spp_n 0", [](World &w) { w.n = 0; w.spp_n = 0; }, RLS_OK)
     // the chunks go through rls_disney_integrate, which checks the rest
     .on("spp_n 17", [](World &w) { w.spp_n = 17; }, BAD, "spp_n must be in [1, 16]", "rls_disney_integrate")
     .on("wo NULL", [](World &w) { w.dc.wo.x = nullptr; }, BAD, "wo/N/T plane is NULL", "rls_disney_integrate")
     .on("base_color mixed NULL", [](World &w) { w.dc.base_color.g = nullptr; }, BAD,
         "base_color planes must be all set or all NULL", "rls_disney_integrate")
     .on("materials.count 0", [](World &w) { w.dc.materials.count = 0; }, BAD, MATERIALS, "rls_disney_integrate")
     .on("stream.f NULL", [](World &w) { w.st.f.b = nullptr; }, BAD, "NULL streamed-output plane", "rls_disney_integrate");

    v = verb("rls_disney_direct_lighting", [](World &w) {
        return rls_disney_direct_lighting(w.ctx, w.n, w.dp, w.P, w.lp, w.n_lights, w.spp_n, 7u, 0u, w.f, w.f2);
    });
    v.basics().spp().lights(1)
     .on("P NULL", [](World &w) { w.P.x = nullptr; }, BAD, "wo/N/T/P plane is NULL")
     .on("direct_diffuse NULL", [](World &w) { w.f.g = nullptr; }, BAD, "NULL output plane")
     .on("direct_specular NULL", [](World &w) { w.f2.r = nullptr; }, BAD, "NULL output plane");
    disney_closure(v, "closure is NULL", "wo/N/T/P plane is NULL"); empty_before_closure(v);

    v = verb("rls_disney_shade", [](World &w) {
        return rls_disney_shade(w.ctx, w.n, w.dp, w.P, w.lp, w.n_lights, w.envp, w.spp_n, 7u, 0u, w.dsop);
    });
    const char *null = "closure, env or out is NULL";
    v.basics().spp().lights(0)
     .on("env NULL", [](World &w) { w.envp = nullptr; }, BAD, null)
     .on("out NULL", [](World &w) { w.dsop = nullptr; }, BAD, null)
     .on("P NULL", [](World &w) { w.P.y = nullptr; }, BAD, "wo/N/T/P plane is NULL")
     .on("direct_diffuse NULL", [](World &w) { w.dso.direct_diffuse.r = nullptr; }, BAD, "NULL AOV plane")
     .on("indirect_specular NULL", [](World &w) { w.dso.indirect_specular.g = nullptr; }, BAD, "NULL AOV plane")
     .on("out mixed NULL", [](World &w) { w.dso.out.b = nullptr; }, BAD, "out planes must be all set or all NULL")
     .on("out NULL", [](World &w) { w.dso.out = {}; }, HIP);
    disney_closure(v, null, "wo/N/T/P plane is NULL"); empty_before_closure(v);
}

void misc_verbs()
{
    Verb v = verb("rls_gaussian_sample", [](World &w) { return rls_gaussian_sample(w.ctx, w.n, w.dist, w.x, w.o1, w.o2, w.o3); });
    v.basics().on("rx NULL", [](World &w) { w.x = nullptr; }, BAD, "NULL plane")
     .on("profile NULL", [](World &w) { w.o3 = nullptr; }, BAD, "NULL plane")
     .on("n == 0, rx NULL", [](World &w) { w.n = 0; w.x = nullptr; }, RLS_OK);

    v = verb("rls_libm_eval", [](World &w) { return rls_libm_eval(w.ctx, w.e, w.n, w.x, w.y, w.o1); });
    v.basics().on("unary, y NULL", [](World &w) { w.e = RLS_FN_SQRT; w.y = nullptr; }, HIP)
     .on("binary, y NULL", [](World &w) { w.e = RLS_FN_POW; w.y = nullptr; }, BAD, "NULL plane")
     .on("x NULL", [](World &w) { w.x = nullptr; }, BAD, "NULL plane")
     .on("out NULL", [](World &w) { w.o1 = nullptr; }, BAD, "NULL plane")
     .on("unknown function", [](World &w) { w.e = RLS_FN_COS_BOUNDED + 1; }, BAD, "unknown function id")
     .on("function -1", [](World &w) { w.e = -1; }, BAD, "unknown function id")
     .on("n == 0, unknown function", [](World &w) { w.n = 0; w.e = 99; }, RLS_OK);

    v = verb("rls_sss_cavity_fade", [](World &w) { return rls_sss_cavity_fade(w.ctx, w.n, w.a, w.b, w.c, w.o1); });
    v.basics().on("No NULL", [](World &w) { w.c.y = nullptr; }, BAD, "NULL plane")
     .on("fade NULL", [](World &w) { w.o1 = nullptr; }, BAD, "NULL plane")
     .on("n == 0, fade NULL", [](World &w) { w.n = 0; w.o1 = nullptr; }, RLS_OK);
    v = verb("rls_sss_sample_diffuse_direction",
             [](World &w) { return rls_sss_sample_diffuse_direction(w.ctx, w.n, w.a, w.b, w.x, w.y, w.v); });
    v.basics().on("T NULL", [](World &w) { w.b.x = nullptr; }, BAD, "NULL plane")
     .on("wi NULL", [](World &w) { w.v.z = nullptr; }, BAD, "NULL plane");
    v = verb("rls_util_directions", [](World &w) { return rls_util_directions(w.ctx, w.n, w.x, w.y, w.v, w.v2); });
    v.basics().on("b NULL", [](World &w) { w.y = nullptr; }, BAD, "NULL plane")
     .on("disk NULL", [](World &w) { w.v2.y = nullptr; }, BAD, "NULL plane");
    v = verb("rls_util_reflect_luminance",
             [](World &w) { return rls_util_reflect_luminance(w.ctx, w.n, w.a, w.b, w.c, w.v, w.o1); });
    v.basics().on("color NULL", [](World &w) { w.c.z = nullptr; }, BAD, "NULL plane")
     .on("luminance NULL", [](World &w) { w.o1 = nullptr; }, BAD, "NULL plane");
}

void sss_verbs()
{
    Verb v = verb("rls_nd_sample", [](World &w) { return rls_nd_sample(w.ctx, w.n, w.sp, w.x, w.o1, w.o2, w.f); });
    v.basics().on("rx NULL", [](World &w) { w.x = nullptr; }, BAD, "NULL plane")
     .on("profile NULL", [](World &w) { w.f.g = nullptr; }, BAD, "NULL plane");
    sss_closure(v, nullptr); empty_before_closure(v);
    v = verb("rls_nd_pdf", [](World &w) { return rls_nd_pdf(w.ctx, w.n, w.sp, w.x, w.o1); });
    v.basics().on("r NULL", [](World &w) { w.x = nullptr; }, BAD, "NULL plane")
     .on("pdf NULL", [](World &w) { w.o1 = nullptr; }, BAD, "NULL plane");
    sss_closure(v, nullptr); empty_before_closure(v);
    v = verb("rls_nd_eval", [](World &w) { return rls_nd_eval(w.ctx, w.n, w.sp, w.x, w.f); });
    v.basics().on("r NULL", [](World &w) { w.x = nullptr; }, BAD, "NULL plane")
     .on("profile NULL", [](World &w) { w.f.b = nullptr; }, BAD, "NULL plane");
    sss_closure(v, nullptr); empty_before_closure(v);

    v = verb("rls_sss_probe_ray", [](World &w) {
        return rls_sss_probe_ray(w.ctx, w.n, w.sp, w.x, w.y, w.P, w.o1, w.v, w.v2, w.o2, w.o3, w.f);
    });
    v.basics().on("rx NULL", [](World &w) { w.x = nullptr; }, BAD, "rx/ry is NULL")
     .on("P mixed NULL", [](World &w) { w.P.y = nullptr; }, BAD, "P planes must be all set or all NULL")
     .on("P NULL", [](World &w) { w.P = {}; }, HIP)
     .on("origin NULL", [](World &w) { w.v.x = nullptr; }, BAD, "NULL output plane")
     .on("maxdist NULL", [](World &w) { w.o2 = nullptr; }, BAD, "NULL output plane")
     .on("profile NULL", [](World &w) { w.f.r = nullptr; }, BAD, "NULL output plane")
     .on("per-point parameters, no materials", [](World &w) { w.sc.materials = {}; }, HIP)
     .on("uniform parameters, no materials", [](World &w) { w.sc.materials = {}; w.sc.sss_dist_multiplier = {}; }, HIP)
     .on("materials.count 0, N NULL", [](World &w) { w.sc.materials.count = 0; w.sc.N.x = nullptr; }, BAD, MATERIALS);
    sss_closure(v, "N/T plane is NULL"); empty_before_closure(v);
    v = verb("rls_sss_mis_pdf", [](World &w) { return rls_sss_mis_pdf(w.ctx, w.n, w.sp, w.a, w.b, 0, w.o1); });
    v.basics().on("disp NULL", [](World &w) { w.a.x = nullptr; }, BAD, "NULL plane")
     .on("pdf NULL", [](World &w) { w.o1 = nullptr; }, BAD, "NULL plane");
    sss_closure(v, "N/T plane is NULL"); empty_before_closure(v);

    v = verb("rls_sss_integrate_scatter", [](World &w) {
        return rls_sss_integrate_scatter(w.ctx, w.n, w.sp, w.P, w.scenep, w.spp_n, 7u, 0u, w.f, w.o1);
    });
    v.basics().spp()
     .on("closure NULL", [](World &w) { w.sp = nullptr; }, BAD, "closure or scene is NULL")
     .on("scene NULL", [](World &w) { w.scenep = nullptr; }, BAD, "closure or scene is NULL")
     .on("N NULL", [](World &w) { w.sc.N.z = nullptr; }, BAD, "N/T/P plane is NULL")
     .on("P NULL", [](World &w) { w.P.x = nullptr; }, BAD, "N/T/P plane is NULL")
     .on("N NULL, sss_color mixed NULL", [](World &w) { w.sc.N.z = nullptr; w.sc.sss_color.g = nullptr; }, BAD,
         "N/T/P plane is NULL")
     .on("sss_color mixed NULL", [](World &w) { w.sc.sss_color.g = nullptr; }, BAD, "sss_color planes must be all set or all NULL")
     .on("materials.count 0", [](World &w) { w.sc.materials.count = 0; }, BAD, MATERIALS)
     .on("unknown geometry", [](World &w) { w.scene.geometry = 2; }, BAD, "unknown scene geometry")
     .on("result NULL", [](World &w) { w.f.b = nullptr; }, BAD, "NULL output plane")
     .on("mean_depth NULL", [](World &w) { w.o1 = nullptr; }, HIP);
    empty_before_closure(v);
}

void skin_verbs()
{
    Verb v = verb("rls_skin_sample_eval_pdf", [](World &w) { return rls_skin_sample_eval_pdf(w.ctx, w.n, w.kp, w.xip, w.kop); });
    v.basics().on("xi NULL", [](World &w) { w.xip = nullptr; }, BAD, "NULL argument")
     .on("out NULL", [](World &w) { w.kop = nullptr; }, BAD, "NULL argument")
     .on("xi[5] NULL", [](World &w) { w.xi[5] = nullptr; }, BAD, "xi plane is NULL")
     .on("sheen_wi NULL", [](World &w) { w.ko.sheen_wi.x = nullptr; }, BAD, "NULL output plane")
     .on("profile NULL", [](World &w) { w.ko.profile.b = nullptr; }, BAD, "NULL output plane")
     .on("sssWeight NULL", [](World &w) { w.ko.sssWeight = nullptr; }, BAD, "NULL output plane")
     .on("all parameters streamed, no materials", [](World &w) { w.kc.materials = {}; }, HIP);
    skin_closure(v, "NULL argument", "wo/N/T plane is NULL"); empty_before_closure(v);

    v = verb("rls_skin_integrate", [](World &w) {
        return rls_skin_integrate(w.ctx, w.n, w.kp, w.P, w.scenep, w.envp, w.lp, w.n_lights, w.spp_n, 7u, 0u, w.kiop);
    });
    const char *null = "closure, scene, env or out is NULL";
    v.basics().spp().lights(0)
     .on("scene NULL", [](World &w) { w.scenep = nullptr; }, BAD, null)
     .on("env NULL", [](World &w) { w.envp = nullptr; }, BAD, null)
     .on("out NULL", [](World &w) { w.kiop = nullptr; }, BAD, null)
     .on("P NULL", [](World &w) { w.P.z = nullptr; }, BAD, "wo/N/T/P plane is NULL")
     .on("unknown geometry", [](World &w) { w.scene.geometry = -1; }, BAD, "unknown scene geometry")
     .on("sheen NULL", [](World &w) { w.kio.sheen.r = nullptr; }, BAD, "NULL AOV plane")
     .on("sss NULL", [](World &w) { w.kio.sss.b = nullptr; }, BAD, "NULL AOV plane")
     .on("out mixed NULL", [](World &w) { w.kio.out.r = nullptr; }, BAD, "out planes must be all set or all NULL")
     .on("out NULL", [](World &w) { w.kio.out = {}; }, HIP);
    skin_closure(v, null, "wo/N/T/P plane is NULL"); empty_before_closure(v);
}

void trace_verbs()
{
    const char *queue = "queue or queue.offsets is NULL", *weight = "queue.weight plane is NULL";
    for (int refract = 0; refract < 2; refract++) {
        Verb v = refract
            ? verb("rls_trace_ggx_refract_emit",
                   [](World &w) { return rls_trace_ggx_refract_emit(w.ctx, w.n, w.gp, w.spp_n, 7u, 0u, w.qp, w.o1); }, "emit")
            : verb("rls_trace_ggx_glossy_emit",
                   [](World &w) { return rls_trace_ggx_glossy_emit(w.ctx, w.n, w.gp, w.spp_n, 7u, 0u, w.qp, w.o1); }, "emit");
        v.on("valid", [](World &) {}, HIP)
         .on("ctx NULL", [](World &w) { w.ctx = nullptr; }, BAD, "ctx is NULL")
         .on("n < 0", [](World &w) { w.n = -1; }, BAD, "n < 0")
         .on("n = 2^32", [](World &w) { w.n = (int64_t)1 << 32; }, BAD, "n > 2^32 - 1 (the queue's point index is 32-bit)")
         .on("n = 2^32, spp_n 0", [](World &w) { w.n = (int64_t)1 << 32; w.spp_n = 0; }, BAD,
             "n > 2^32 - 1 (the queue's point index is 32-bit)")
         .on("spp_n 0", [](World &w) { w.spp_n = 0; }, BAD, "spp_n must be in [1, 16]")
         .on("spp_n 17", [](World &w) { w.spp_n = 17; }, BAD, "spp_n must be in [1, 16]")
         .on("spp_n 17, queue NULL", [](World &w) { w.spp_n = 17; w.qp = nullptr; }, BAD, "spp_n must be in [1, 16]")
         .on("queue NULL", [](World &w) { w.qp = nullptr; }, BAD, queue)
         .on("queue.offsets NULL", [](World &w) { w.q.offsets = nullptr; }, BAD, queue)
         // an empty batch still writes offsets[0] = 0: a launch
         .on("n == 0", [](World &w) { w.n = 0; }, HIP)
         .on("n == 0, spp_n 0", [](World &w) { w.n = 0; w.spp_n = 0; }, BAD, "spp_n must be in [1, 16]")
         .on("n == 0, queue NULL", [](World &w) { w.n = 0; w.qp = nullptr; }, BAD, queue)
         .on("n == 0, closure NULL", [](World &w) { w.n = 0; w.gp = nullptr; }, HIP)
         .on("queue.dir NULL", [](World &w) { w.q.dir.y = nullptr; }, BAD, "queue.dir plane is NULL")
         .on("queue.weight.r NULL", [](World &w) { w.q.weight.r = nullptr; }, BAD, weight)
         .on("queue.capacity short", [](World &w) { w.q.capacity = w.n * w.spp_n * w.spp_n - 1; }, BAD,
             "queue.capacity < n * spp_n^2")
         .on("queue.scratch NULL", [](World &w) { w.q.scratch = nullptr; }, BAD,
             "queue.scratch is NULL or smaller than rls_trace_scratch_bytes")
         .on("queue.scratch short", [](World &w) { w.q.scratch_bytes = 4096; }, BAD,
             "queue.scratch is NULL or smaller than rls_trace_scratch_bytes")
         .on("side NULL", [](World &w) { w.o1 = nullptr; }, HIP);
        if (refract) v.on("queue.weight.g NULL", [](World &w) { w.q.weight.g = nullptr; }, HIP);
        else v.on("queue.weight.g NULL", [](World &w) { w.q.weight.g = nullptr; }, BAD, weight);
        ggx_closure(v);
    }
    for (int refract = 0; refract < 2; refract++) {
        Verb v = refract
            ? verb("rls_trace_ggx_refract_resolve",
                   [](World &w) { return rls_trace_ggx_refract_resolve(w.ctx, w.n, w.qp, w.spp_n, w.L, w.f); }, "resolve")
            : verb("rls_trace_ggx_glossy_resolve",
                   [](World &w) { return rls_trace_ggx_glossy_resolve(w.ctx, w.n, w.qp, w.L, w.f); }, "resolve");
        v.basics()
         .on("queue NULL", [](World &w) { w.qp = nullptr; }, BAD, queue)
         .on("queue.offsets NULL", [](World &w) { w.q.offsets = nullptr; }, BAD, queue)
         .on("n == 0, queue NULL", [](World &w) { w.n = 0; w.qp = nullptr; }, RLS_OK)
         .on("queue.weight.r NULL", [](World &w) { w.q.weight.r = nullptr; }, BAD, weight)
         .on("radiance NULL", [](World &w) { w.L.g = nullptr; }, BAD, "radiance plane is NULL")
         .on("out NULL", [](World &w) { w.f.b = nullptr; }, BAD, "NULL output plane");
        if (refract) v.spp().on("queue.weight.g NULL", [](World &w) { w.q.weight.g = nullptr; }, HIP);
        else v.on("queue.weight.g NULL", [](World &w) { w.q.weight.g = nullptr; }, BAD, weight);
    }
}

} // namespace

int main()
{
    int devices = 0;
    if (hipGetDeviceCount(&devices) == hipSuccess && devices > 0) {
        fprintf(stderr, "argument_checks: %d HIP device(s) visible; this driver hands dummy planes to the entry points and "
                        "runs only where no device is\n", devices);
        return 2;
    }
    (void)hipGetLastError();
    ggx_verbs();
    disney_verbs();
    misc_verbs();
    sss_verbs();
    skin_verbs();
    trace_verbs();
    for (int fast = 0; fast < 2; fast++) {
        for (const Case &c : g_cases) {
            World w(fast);
            c.brk(w);
            const rls_status st = c.call(w);
            const char *msg = st == RLS_OK ? "" : rls_last_error();
            printf("%s\t%s\t%d\t%d\t%d\t%s\t%s\t%s\n", c.entry.c_str(), c.what.c_str(), fast, st, c.status, c.prefix.c_str(),
                   c.text.c_str(), msg);
        }
    }
    return 0;
}
