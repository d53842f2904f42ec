/*
 * ref_ggx.cpp -- drives the reference's GGX closure (src/rlGgx.h, src/rlGgx.cpp) and its utilities
 * (src/rlUtil.h, src/rlUtil.cpp), compiled from the reference checkout by path (oracle/Makefile,
 * target `ref`).  Batch entry points mirror the oracle's orc_batch_* (same SoA structs).
 *
 * Shading globals of every point: sg.N = sg.Nf = N, sg.Rd = -wo, sg.P = 0; the tangent T is what the
 * AiBuildLocalFramePolar stand-in returns.  The closure decides entering / exiting itself from
 * dot(sg.N, sg.Rd) < AI_EPSILON; the SoA's `exiting` plane is not read.
 */
#include <algorithm>
#include <cassert>
#include <cstdlib>
#include <functional>
#include <memory>
#include <set>
#include <string>
#include <vector>
#include <sstream>
#include <iostream>
#include <iomanip>

#define private public
#include "rlGgx.cpp"      /* resolved on the reference checkout's src/ (-I$(REF_SRC)/src) */
#include "rlUtil.cpp"
#undef private

#include "../rls_oracle.h"
#include "ref_services.h"

namespace
{
inline AtVector ld3(orc_cv3p p, int64_t i) { return AtVector{p.x[i], p.y[i], p.z[i]}; }
inline void st3(orc_v3p p, int64_t i, const AtVector &v) { p.x[i] = v.x; p.y[i] = v.y; p.z[i] = v.z; }
inline void stc(orc_v3p p, int64_t i, const AtRGB &c) { p.x[i] = c.r; p.y[i] = c.g; p.z[i] = c.b; }

struct RefractData
{
    bool shouldTraceRefract(AtShaderGlobals *) const { return true; }
    AtSamplerIterator *getSamplerIter(AtShaderGlobals *sg) const { return AiSamplerIterator(AiSampler(1, 2), sg); }
};

enum { FUSED, EVAL, PDF, REFRACT, MICRO, NDFPDF };

struct Job
{
    const orc_ggx_soa *in; const float *rx, *ry; orc_cv3p cwi;
    orc_v3p wi, f; float *pdf, *fresnel, *weight; uint8_t *flag; int mode, alt;
};

AtShaderGlobals globals(const orc_ggx_soa *in, int64_t i)
{
    AtShaderGlobals sg = {};
    sg.N = sg.Nf = ld3(in->N, i);
    sg.Rd = -ld3(in->wo, i);
    refh::tangent = ld3(in->T, i);
    return sg;
}

AtRGB ks(const orc_ggx_soa *in, int64_t i) { return AtRGB{in->KsColor.x[i], in->KsColor.y[i], in->KsColor.z[i]}; }
float aniso(const orc_ggx_soa *in, int64_t i) { return in->anisotropic ? in->anisotropic[i] : 0.0f; }

/* constructed in place: the microfacet kernel keeps a reference to the closure's frame */
#define CLOSURE(type, g) \
    AtShaderGlobals sg = globals(j->in, i); \
    type g(&sg, ks(j->in, i), j->in->ior[i], j->in->specularRoughness[i], aniso(j->in, i))

void range(int64_t lo, int64_t hi, void *ctx)
{
    Job *j = static_cast<Job *>(ctx);
    for (int64_t i = lo; i < hi; i++) {
        if (j->mode == MICRO && j->alt) {
            CLOSURE(rls::GgxSamplerT<rls::NDFKernel>, g);
            st3(j->wi, i, g.mNormalSampler->evalSample(j->rx[i], j->ry[i]));
            continue;
        }
        if (j->mode == NDFPDF) {
            CLOSURE(rls::GgxSamplerT<rls::NDFKernel>, g);
            AtVector w = ld3(j->cwi, i);
            j->pdf[i] = rls::GgxSamplerT<rls::NDFKernel>::evalPdf(&g, &w);
            continue;
        }
        CLOSURE(rls::GgxSampler, g);
        switch (j->mode) {
        case FUSED: {
            /* the reference's call order: evalSample -> evalBrdf -> evalPdf */
            AtVector L = rls::GgxSampler::evalSample(&g, j->rx[i], j->ry[i]);
            AtRGB f = rls::GgxSampler::evalBrdf(&g, &L);
            float pdf = rls::GgxSampler::evalPdf(&g, &L);
            st3(j->wi, i, L); stc(j->f, i, f); j->pdf[i] = pdf;
            if (j->fresnel) j->fresnel[i] = g.getAvgReflectWeight();
        } break;
        case EVAL: {
            AtVector w = ld3(j->cwi, i);
            stc(j->f, i, rls::GgxSampler::evalBrdf(&g, &w));
        } break;
        case PDF: {
            AtVector w = ld3(j->cwi, i);
            j->pdf[i] = rls::GgxSampler::evalPdf(&g, &w);
        } break;
        case REFRACT: {
            /* integrateRefract's traced branch with one sample: the unit environment makes the result the
               sample weight; the recorded ray carries the direction */
            refh::sample_xi[0] = j->rx[i];
            refh::sample_xi[1] = j->ry[i];
            RefractData data;
            AtRGB res = g.integrateRefract(&sg, &data);
            st3(j->wi, i, refh::traced_ray.dir);
            j->weight[i] = res.r;
            if (j->flag) j->flag[i] = (uint8_t)refh::refracted;
        } break;
        case MICRO:
            st3(j->wi, i, g.mNormalSampler->evalSample(j->rx[i], j->ry[i]));
            break;
        }
    }
}

void run(int64_t n, Job &j, int nthreads) { refh::parallel_for(n, nthreads, range, &j); }
}

extern "C" {

void ref_batch_ggx_sample_eval_pdf(int64_t n, const orc_ggx_soa *in, const float *rx, const float *ry,
                                   orc_v3p wi, orc_v3p f, float *pdf, float *fresnel, int nthreads)
{
    Job j = {}; j.in = in; j.rx = rx; j.ry = ry; j.wi = wi; j.f = f; j.pdf = pdf; j.fresnel = fresnel; j.mode = FUSED;
    run(n, j, nthreads);
}

void ref_batch_ggx_eval(int64_t n, const orc_ggx_soa *in, orc_cv3p wi, orc_v3p f, int nthreads)
{
    Job j = {}; j.in = in; j.cwi = wi; j.f = f; j.mode = EVAL;
    run(n, j, nthreads);
}

void ref_batch_ggx_pdf(int64_t n, const orc_ggx_soa *in, orc_cv3p wi, float *pdf, int nthreads)
{
    Job j = {}; j.in = in; j.cwi = wi; j.pdf = pdf; j.mode = PDF;
    run(n, j, nthreads);
}

void ref_batch_ggx_refract(int64_t n, const orc_ggx_soa *in, const float *rx, const float *ry,
                           orc_v3p wt, float *weight, uint8_t *refracted, int nthreads)
{
    Job j = {}; j.in = in; j.rx = rx; j.ry = ry; j.wi = wt; j.weight = weight; j.flag = refracted; j.mode = REFRACT;
    run(n, j, nthreads);
}

void ref_batch_ggx_microfacet(int64_t n, const orc_ggx_soa *in, const float *rx, const float *ry,
                              orc_v3p m, int use_ndf_kernel, int nthreads)
{
    Job j = {}; j.in = in; j.rx = rx; j.ry = ry; j.wi = m; j.mode = MICRO; j.alt = use_ndf_kernel;
    run(n, j, nthreads);
}

void ref_batch_ggx_ndf_pdf(int64_t n, const orc_ggx_soa *in, orc_cv3p wi, float *pdf, int nthreads)
{
    Job j = {}; j.in = in; j.cwi = wi; j.pdf = pdf; j.mode = NDFPDF;
    run(n, j, nthreads);
}

/* a in [0,1) -> sphericalDirection(2a - 1, 2 pi b); concentricDiskSample(a, b) (z is left unset by the
   reference: written as 0 here, as the oracle does) */
void ref_batch_util(int64_t n, const float *a, const float *b, orc_v3p spherical, orc_v3p disk, int)
{
    for (int64_t i = 0; i < n; i++) {
        st3(spherical, i, rls::sphericalDirection(2.0f * a[i] - 1.0f, AI_PITIMES2 * b[i]));
        AtVector d = rls::concentricDiskSample(a[i], b[i]);
        st3(disk, i, AtVector{d.x, d.y, 0.0f});
    }
}

void ref_batch_reflect_luminance(int64_t n, orc_cv3p i, orc_cv3p nrm, orc_cv3p color, orc_v3p reflected,
                                 float *luminance)
{
    for (int64_t k = 0; k < n; k++) {
        st3(reflected, k, rls::reflectDirection(ld3(i, k), ld3(nrm, k)));
        luminance[k] = rls::colorToLuminance(AtRGB{color.x[k], color.y[k], color.z[k]});
    }
}

}
