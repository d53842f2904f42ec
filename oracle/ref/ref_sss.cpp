/*
 * ref_sss.cpp -- drives the reference's subsurface profiles and the hot parts of SssSampler
 * (src/rlSss.h, src/rlSss.cpp), compiled from the reference checkout by path (oracle/Makefile,
 * target `ref`).
 *
 * Inputs are the oracle's orc_sss_soa: scatter distance (times the multiplier when given, as
 * src/rlSkin.cpp does), albedo (white when absent), Ns and dPdu / T.  SssSampler's shading globals:
 * sg.Ns = N, sg.dPdu = T when has_dPdu else 0 (the constructor then takes the polar-frame stand-in,
 * whose tangent is T), sg.P = -0 so that the probe origin is the offset bit for bit.
 * GaussianProfile's fast_exp is the stand-in expf (ref_services.cpp).
 */
#include <algorithm>
#include <array>
#include <cassert>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <set>
#include <string>
#include <vector>

#define private public
#include "rlSss.cpp"        /* resolved on the reference checkout's src/ (-I$(REF_SRC)/src) */
#undef private

#include "../rls_oracle.h"
#include "ref_services.h"

namespace
{
inline AtVector ld3(orc_cv3p p, int64_t i) { return AtVector{p.x[i], p.y[i], p.z[i]}; }
inline void st3(orc_v3p p, int64_t i, const AtVector &v) { p.x[i] = v.x; p.y[i] = v.y; p.z[i] = v.z; }
inline void stc(orc_v3p p, int64_t i, const AtRGB &c) { p.x[i] = c.r; p.y[i] = c.g; p.z[i] = c.b; }

using Sss = rls::SssSampler<rls::NDProfile>;

enum { ND, NDPDF, NDPROFILE, PROBE, DIFFUSE, GAUSS };

struct Job
{
    const orc_sss_soa *in; int has_dPdu; const float *rx, *ry, *rin;
    orc_cv3p normal, T;
    float *r; orc_v3p offset, dir; float *maxdist, *pdf; orc_v3p profile; float *prof1; int mode;
};

AtVector dist(const orc_sss_soa *in, int64_t i)
{
    AtVector d = ld3(in->sss_scatter_dist, i);
    if (in->sss_dist_multiplier) d = d * in->sss_dist_multiplier[i];
    return d;
}

AtRGB albedo(const orc_sss_soa *in, int64_t i)
{
    return in->sss_color.x ? AtRGB{in->sss_color.x[i], in->sss_color.y[i], in->sss_color.z[i]} : AI_RGB_WHITE;
}

void range(int64_t lo, int64_t hi, void *ctx)
{
    Job *j = static_cast<Job *>(ctx);
    for (int64_t i = lo; i < hi; i++) {
        switch (j->mode) {
        case ND: {
            rls::NDProfile p;
            p.setDistance(dist(j->in, i), albedo(j->in, i));
            float r = p.getRadius(j->rx[i]);
            j->r[i] = r; j->pdf[i] = p.getPdf(r); stc(j->profile, i, p.evalProfile(r));
        } break;
        case NDPDF: {
            rls::NDProfile p;
            p.setDistance(dist(j->in, i), albedo(j->in, i));
            j->pdf[i] = p.getPdf(j->rin[i]);
        } break;
        case NDPROFILE: {
            rls::NDProfile p;
            p.setDistance(dist(j->in, i), albedo(j->in, i));
            stc(j->profile, i, p.evalProfile(j->rin[i]));
        } break;
        case PROBE: {
            AtShaderGlobals sg = {};
            sg.Ns = ld3(j->in->N, i);
            refh::tangent = ld3(j->in->T, i);
            sg.dPdu = j->has_dPdu ? refh::tangent : AI_V3_ZERO;
            sg.P = AtVector{-0.0f, -0.0f, -0.0f};
            Sss s(&sg, albedo(j->in, i), dist(j->in, i));
            AtRay ray;
            float r = s.getProbeRay(j->rx[i], j->ry[i], sg.P, ray);
            j->r[i] = r; st3(j->offset, i, ray.origin); st3(j->dir, i, ray.dir); j->maxdist[i] = (float)ray.maxdist;
            j->pdf[i] = s.mProfile.getPdf(r);
            stc(j->profile, i, s.mProfile.evalProfile(r));
        } break;
        case DIFFUSE: {
            AtShaderGlobals sg = {};
            sg.Ns = AtVector{0.0f, 0.0f, 1.0f};
            sg.dPdu = AtVector{1.0f, 0.0f, 0.0f};
            Sss s(&sg, AI_RGB_WHITE, AtVector{1.0f, 1.0f, 1.0f});
            refh::tangent = ld3(j->T, i);
            st3(j->dir, i, s.sampleDiffuseDirection(j->rx[i], j->ry[i], ld3(j->normal, i)));
        } break;
        case GAUSS: {
            rls::GaussianProfile g;
            g.setDistance(AtVector{j->rin[i], 0.0f, 0.0f}, AI_RGB_WHITE);
            float r = g.getRadius(j->rx[i]);
            j->r[i] = r; j->pdf[i] = g.getPdf(r); j->prof1[i] = g.evalProfile(r);
        } break;
        }
    }
}
}

extern "C" {

void ref_batch_nd_sample_pdf_profile(int64_t n, const orc_sss_soa *in, const float *rx,
                                     float *r, float *pdf, orc_v3p profile, int nthreads)
{
    Job j = {}; j.in = in; j.rx = rx; j.r = r; j.pdf = pdf; j.profile = profile; j.mode = ND;
    refh::parallel_for(n, nthreads, range, &j);
}

void ref_batch_nd_pdf(int64_t n, const orc_sss_soa *in, const float *r, float *pdf, int nthreads)
{
    Job j = {}; j.in = in; j.rin = r; j.pdf = pdf; j.mode = NDPDF;
    refh::parallel_for(n, nthreads, range, &j);
}

void ref_batch_nd_profile(int64_t n, const orc_sss_soa *in, const float *r, orc_v3p profile, int nthreads)
{
    Job j = {}; j.in = in; j.rin = r; j.profile = profile; j.mode = NDPROFILE;
    refh::parallel_for(n, nthreads, range, &j);
}

/* offset = ray.origin - sg.P (sg.P = -0), as orc_batch_sss_probe */
void ref_batch_sss_probe(int64_t n, const orc_sss_soa *in, int has_dPdu, const float *rx, const float *ry,
                         float *r, orc_v3p offset, orc_v3p dir, float *maxdist,
                         float *pdf, orc_v3p profile, int nthreads)
{
    Job j = {}; j.in = in; j.has_dPdu = has_dPdu; j.rx = rx; j.ry = ry; j.r = r; j.offset = offset; j.dir = dir;
    j.maxdist = maxdist; j.pdf = pdf; j.profile = profile; j.mode = PROBE;
    refh::parallel_for(n, nthreads, range, &j);
}

void ref_batch_sss_sample_diffuse(int64_t n, orc_cv3p normal, orc_cv3p T, const float *rx, const float *ry,
                                  orc_v3p wi, int nthreads)
{
    Job j = {}; j.normal = normal; j.T = T; j.rx = rx; j.ry = ry; j.dir = wi; j.mode = DIFFUSE;
    refh::parallel_for(n, nthreads, range, &j);
}

void ref_batch_gauss(int64_t n, const float *dist_x, const float *rx, float *r, float *pdf, float *profile,
                     int nthreads)
{
    Job j = {}; j.rin = dist_x; j.rx = rx; j.r = r; j.pdf = pdf; j.prof1 = profile; j.mode = GAUSS;
    refh::parallel_for(n, nthreads, range, &j);
}

}
