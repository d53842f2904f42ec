/* bounded_study.c -- how much of config 2's arithmetic can leave the reference's operation sequence before an output
 * moves by more than north_star's 1e-5?  A CPU study on top of the oracle (test infrastructure; run by
 * tests/bounded_mode_study.py, results in profiles/r03_bounded_mode_study.txt).
 *
 * The question behind VERDICT r2 "next round" item 3: a third arithmetic mode that runs a cheap view analysis in every lane
 * and sends only the lanes a predictor flags through the exact functions.  Here the "cheap" variants use EXACTLY ROUNDED
 * + - * / sqrt in a mathematically equivalent but different operation sequence (no angle functions) -- the best case for
 * any fast path, hardware-approximate reciprocals and square roots only add error on top:
 *   bit 0 (A): the first round trip -- phiV = atan2f(V.V, U.V), sphericalDirection(cos, phiV) (src/rlGgx.cpp:68-72) --
 *              by algebra: (r x / h, r y / h, cos) with r = sqrtf(1 - cos^2) kept as the reference has it, h = |(x, y)|
 *   bit 1 (B): tanf(acosf(v.z)) (src/rlGgx.cpp:80, 31) by |(v.x, v.y)| / v.z
 *   bit 2 (C): cosf / sinf(atan2f(v.y, v.x)) (81, 86-87) by v.x / |(v.x, v.y)|, v.y / |(v.x, v.y)|
 * Everything downstream (slope equations, rotation, reflection, Fresnel, evalBrdf, evalPdf, refraction, weight) is the
 * oracle's own code.  For every point of the bench's seeded workload the program compares the variant's twelve config-2
 * outputs with the oracle's, the way the parity tests do (vectors by norm), and prints per point one record the Python
 * side turns into exceedance rates and into the smallest set of lanes a threshold predictor would have to flag.
 *
 * usage: bounded_study <variant bits> <log2 points> <seed> <out.bin>   -> writes n records of 6 floats:
 *   worst relative error over the 6 output groups, theta' (stretched view angle), min(alphaX, alphaY), |A^2 - 1| of the
 *   reflect sample, |A^2 - 1| of the refract sample, cos(theta_view) */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>

#include "../../oracle/rls_oracle.c"

static orc_v3 microfacet_variant(const orc_ggx *g, float rx, float ry, int bits, float *theta_out, float *a2m1_out)
{
    const orc_v3 U = g->U, Vb = g->V, N = g->N;
    const float ax = g->alphaX, ay = g->alphaY;
    orc_v3 V = g->viewDir;
    float cosThetaV = CLAMPf(v3dot(N, V), -1.0f, 1.0f);
    const float x = v3dot(U, V), y = v3dot(Vb, V);
    if (bits & 1) {
        const float r = sqrtf(1.0f - SQRf(cosThetaV));            /* as sphericalDirection has it */
        const float h = sqrtf(x * x + y * y);
        V = h > 0.0f ? v3(r * (x / h), r * (y / h), cosThetaV) : v3(r, 0.0f, cosThetaV);   /* atan2f(0, 0) = 0 */
    } else {
        V = orc_spherical_direction(cosThetaV, atan2f(y, x));
    }
    V.x *= ax;
    V.y *= ay;
    V = v3normalize(V);

    float theta = 0.0f, phi = 0.0f;
    const int tilted = V.z < (1.0f - AI_EPSILON);
    if (tilted) {
        theta = acosf(V.z);
        phi = atan2f(V.y, V.x);
    }
    *theta_out = theta;
    const float hv = sqrtf(V.x * V.x + V.y * V.y);
    /* the slope equations of orc_vndf_sample_slope with B injected */
    orc_v2 slope;
    *a2m1_out = 1.0f;
    if (theta < AI_EPSILON) {
        slope = uniform_slope(rx, ry);
    } else {
        const float B = (bits & 2) ? hv / V.z : tanf(theta);
        const float B2 = SQRf(B);
        const float G1 = 2.0f / (1.0f + sqrtf(1.0f + B2));
        const float A = 2.0f * rx / G1 - 1.0f;
        const float A2 = SQRf(A);
        *a2m1_out = ABSf(A2 - 1.0f);
        if (ABSf(A2 - 1.0f) < AI_EPSILON) {
            slope = uniform_slope(rx, ry);
        } else {
            const float tmp = 1.0f / (A2 - 1.0f);
            const float D = sqrtf(MAXf(0.0f, B2 * SQRf(tmp) - (A2 - B2) * tmp));
            const float slopeX1 = B * tmp - D;
            const float slopeX2 = B * tmp + D;
            slope.x = (A < 0.0f || slopeX2 > (1.0f / B)) ? slopeX1 : slopeX2;
            float sign = 1.0f, u = ry;
            if (u > 0.5f) {
                u = 2.0f * (u - 0.5f);
            } else {
                sign = -1.0f;
                u = 2.0f * (0.5f - u);
            }
            const float z = (u * (u * (u * 0.27385f - 0.73369f) + 0.46341f))
                          / (u * (u * (u * 0.093073f + 0.309420f) - 1.0f) + 0.597999f);
            slope.y = sign * z * sqrtf(1.0f + SQRf(slope.x));
        }
    }
    float cosPhi, sinPhi;
    if ((bits & 4) && tilted && hv > 0.0f) {
        cosPhi = V.x / hv;
        sinPhi = V.y / hv;
    } else {
        cosPhi = cosf(phi);
        sinPhi = sinf(phi);
    }
    orc_v3 omega;
    omega.x = -(cosPhi * slope.x - sinPhi * slope.y) * ax;
    omega.y = -(sinPhi * slope.x + cosPhi * slope.y) * ay;
    omega.z = 1.0f;
    omega = v3rotate_to_frame(omega, U, Vb, N);
    return v3normalize(omega);
}

typedef struct { orc_v3 wi; orc_rgb f; float pdf, F; orc_v3 wt; float w; } outputs;

static void run_point(const orc_ggx *g, const float xi[4], int bits, outputs *o, float feat[3])
{
    float th, a1, a2;
    /* reflect: evalSample -> evalBrdf -> evalPdf (src/rlGgx.h:97-127) */
    orc_v3 M = bits < 0 ? orc_vndf_sample(g, xi[0], xi[1]) : microfacet_variant(g, xi[0], xi[1], bits, &th, &a1);
    o->wi = orc_reflect_direction(g->viewDir, M);
    o->F = orc_ggx_fresnel(g, o->wi, M);
    o->f = orc_ggx_eval_brdf(g, o->wi);
    o->pdf = orc_ggx_eval_pdf(g, o->wi);
    /* refract: the per-sample body of integrateRefract, as orc_ggx_refract_sample */
    orc_v3 m = bits < 0 ? orc_vndf_sample(g, xi[2], xi[3]) : microfacet_variant(g, xi[2], xi[3], bits, &th, &a2);
    orc_v3 i = g->viewDir;
    float eta = g->iorIn / g->iorOut;
    float c = v3dot(i, m);
    float k2 = 1.0f - eta * eta * (1.0f - c * c);
    if (!(k2 < 0.0f)) {
        float sign = (float)SGNf(v3dot(i, g->axisN));
        float k = eta * c - sign * sqrtf(k2);
        o->wt = v3sub(v3scale(m, k), v3scale(i, eta));
    } else {
        o->wt = v3sub(v3scale(m, 2.0f * c), i);
    }
    o->w = orc_ggx_sample_weight(g, i, o->wt, m);
    if (bits >= 0) { feat[0] = th; feat[1] = a1; feat[2] = a2; }
}

static double relv(orc_v3 a, orc_v3 b)
{
    double dx = (double)a.x - b.x, dy = (double)a.y - b.y, dz = (double)a.z - b.z;
    double num = sqrt(dx * dx + dy * dy + dz * dz), den = sqrt((double)b.x * b.x + (double)b.y * b.y + (double)b.z * b.z);
    return num == 0.0 ? 0.0 : num / (den > 1e-30 ? den : 1e-30);
}
static double rels(float a, float b)
{
    double num = fabs((double)a - b), den = fabs((double)b);
    return num == 0.0 ? 0.0 : num / (den > 1e-30 ? den : 1e-30);
}

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: bounded_study <variant bits> <log2 points> <seed> <out.bin>\n"); return 2; }
    const int bits = atoi(argv[1]);
    const int64_t n = (int64_t)1 << atoi(argv[2]);
    const uint32_t seed = (uint32_t)atoi(argv[3]);
    FILE *out = fopen(argv[4], "wb");
    if (!out) return 2;
    const int64_t chunk = 1 << 16;
    float *buf = (float *)malloc(sizeof(float) * (size_t)chunk * 21);
    float *rec = (float *)malloc(sizeof(float) * (size_t)chunk * 6);
    for (int64_t first = 0; first < n; first += chunk) {
        float *p = buf;
        orc_v3p wo = { p, p + chunk, p + 2 * chunk }, N = { p + 3 * chunk, p + 4 * chunk, p + 5 * chunk },
                T = { p + 6 * chunk, p + 7 * chunk, p + 8 * chunk };
        orc_gen_frame(seed, (uint64_t)first, chunk, wo, N, T);
        float *ks = p + 9 * chunk, *rough = p + 12 * chunk, *ior = p + 13 * chunk, *aniso = p + 14 * chunk, *xi = p + 15 * chunk;
        for (int j = 0; j < 3; j++) orc_gen_uniform(seed, (uint64_t)first, chunk, 8 + (uint32_t)j, 0.0f, 1.0f, ks + j * chunk);
        orc_gen_uniform(seed, (uint64_t)first, chunk, 5, 0.05f, 1.0f, rough);
        orc_gen_uniform(seed, (uint64_t)first, chunk, 6, 1.05f, 2.55f, ior);
        orc_gen_aniso(seed, (uint64_t)first, chunk, aniso);
        for (int j = 0; j < 4; j++) orc_gen_uniform(seed, (uint64_t)first, chunk, 11 + (uint32_t)j, 0.0f, 1.0f, xi + j * chunk);
        for (int64_t i = 0; i < chunk; i++) {
            orc_ggx g;
            orc_ggx_init(&g, v3(wo.x[i], wo.y[i], wo.z[i]), v3(N.x[i], N.y[i], N.z[i]), v3(T.x[i], T.y[i], T.z[i]), 0,
                         rgb(ks[i], ks[chunk + i], ks[2 * chunk + i]), ior[i], rough[i], aniso[i]);
            const float x4[4] = { xi[i], xi[chunk + i], xi[2 * chunk + i], xi[3 * chunk + i] };
            outputs ref, var;
            float feat[3] = { 0, 0, 0 };
            run_point(&g, x4, -1, &ref, feat);
            run_point(&g, x4, bits, &var, feat);
            double e = relv(var.wi, ref.wi), t;
            if ((t = relv(v3(var.f.r, var.f.g, var.f.b), v3(ref.f.r, ref.f.g, ref.f.b))) > e) e = t;
            if ((t = rels(var.pdf, ref.pdf)) > e) e = t;
            if ((t = rels(var.F, ref.F)) > e) e = t;
            if ((t = relv(var.wt, ref.wt)) > e) e = t;
            if ((t = rels(var.w, ref.w)) > e) e = t;
            if (!(e == e)) e = 1e30;                                /* NaN mismatch */
            float *r = rec + 6 * i;
            r[0] = (float)e; r[1] = feat[0]; r[2] = g.alphaX < g.alphaY ? g.alphaX : g.alphaY; r[3] = feat[1]; r[4] = feat[2];
            r[5] = v3dot(g.N, g.viewDir);
        }
        fwrite(rec, sizeof(float) * 6, (size_t)chunk, out);
    }
    fclose(out);
    free(buf); free(rec);
    return 0;
}
