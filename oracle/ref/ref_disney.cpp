/*
 * ref_disney.cpp -- drives the reference's DisneySampler (src/rlDisney.cpp), compiled from the
 * reference checkout by path (oracle/Makefile, target `ref`).  Its own unit: rlDisney.cpp and
 * rlGgx.cpp both define an anonymous-namespace ShaderData.
 *
 * DisneySampler(nullptr, &sg) reads its parameters through AiShaderEvalParam*, which the stand-in
 * answers from a per-thread table filled per point (ids: rlDisney.cpp's DisneyParams).
 * Shading globals: sg.N = sg.Nf = N, sg.Rd = -wo; tangent T from the AiBuildLocalFramePolar stand-in.
 * Lobe ids are the oracle's (ORC_RAY_DIFFUSE / ORC_RAY_GLOSSY), mapped to setSampleType.
 */
#include <algorithm>
#include <cassert>
#include <cstdlib>
#include <functional>
#include <memory>
#include <set>
#include <string>
#include <vector>

#define private public
#include "rlDisney.cpp"     /* resolved on the reference checkout's src/ (-I$(REF_SRC)/src) */
#undef private

#include "../rls_oracle.h"
#include "ref_services.h"

namespace
{
inline AtVector ld3(orc_cv3p p, int64_t i) { return AtVector{p.x[i], p.y[i], p.z[i]}; }
inline void st3(orc_v3p p, int64_t i, const AtVector &v) { p.x[i] = v.x; p.y[i] = v.y; p.z[i] = v.z; }
inline void stc(orc_v3p p, int64_t i, const AtRGB &c) { p.x[i] = c.r; p.y[i] = c.g; p.z[i] = c.b; }

/* orc_disney_soa.scalars order (oracle/rls_oracle.h) -> rlDisney parameter ids */
const int kScalarParam[10] = { p_subsurface, p_metallic, p_Ks, p_specular_tint, p_roughness, p_anisotropic,
                               p_sheen, p_sheen_tint, p_clearcoat, p_clearcoat_gloss };

enum { SAMPLE, EVAL, PDF, FUSED, ALT };

struct Job
{
    const orc_disney_soa *in; int lobe; const float *rx, *ry; orc_cv3p cwi;
    orc_v3p wi, f; float *pdf; int mode, kind;
};

void range(int64_t lo, int64_t hi, void *ctx)
{
    Job *j = static_cast<Job *>(ctx);
    const orc_disney_soa *in = j->in;
    for (int64_t i = lo; i < hi; i++) {
        refh::param_rgb[p_base_color] = AtRGB{in->base_color.x[i], in->base_color.y[i], in->base_color.z[i]};
        for (int k = 0; k < 10; k++) refh::param_flt[kScalarParam[k]] = in->scalars[k][i];
        AtShaderGlobals sg = {};
        sg.N = sg.Nf = ld3(in->N, i);
        sg.Rd = -ld3(in->wo, i);
        refh::tangent = ld3(in->T, i);
        DisneySampler d(nullptr, &sg);
        d.setSampleType(j->lobe == ORC_RAY_DIFFUSE ? AI_RAY_DIFFUSE : AI_RAY_GLOSSY);
        switch (j->mode) {
        case SAMPLE:
            st3(j->wi, i, DisneySampler::evalSample(&d, j->rx[i], j->ry[i]));
            break;
        case EVAL: {
            AtVector w = ld3(j->cwi, i);
            stc(j->f, i, DisneySampler::evalBrdf(&d, &w));
        } break;
        case PDF: {
            AtVector w = ld3(j->cwi, i);
            j->pdf[i] = DisneySampler::evalPdf(&d, &w);
        } break;
        case FUSED: {
            AtVector L = DisneySampler::evalSample(&d, j->rx[i], j->ry[i]);
            st3(j->wi, i, L);
            stc(j->f, i, DisneySampler::evalBrdf(&d, &L));
            j->pdf[i] = DisneySampler::evalPdf(&d, &L);
        } break;
        case ALT:
            /* the alternates rlDisney compiles but never selects (mSampleFromVisibleNormal = true) */
            switch (j->kind) {
            case 0: st3(j->wi, i, d.sampleGTR2AnisoDirection(j->rx[i], j->ry[i])); break;
            case 1: st3(j->wi, i, d.sampleGTR2Direction(j->rx[i], j->ry[i])); break;
            case 2: d.mSampleFromVisibleNormal = false; j->pdf[i] = d.evalSpecularPdf(ld3(j->cwi, i)); break;
            case 3: j->pdf[i] = d.D_GTR2(ld3(j->cwi, i)); break;
            }
            break;
        }
    }
}
}

extern "C" {

void ref_batch_disney_sample(int64_t n, const orc_disney_soa *in, int lobe, const float *rx, const float *ry,
                             orc_v3p wi, int nthreads)
{
    Job j = {}; j.in = in; j.lobe = lobe; j.rx = rx; j.ry = ry; j.wi = wi; j.mode = SAMPLE;
    refh::parallel_for(n, nthreads, range, &j);
}

void ref_batch_disney_eval(int64_t n, const orc_disney_soa *in, int lobe, orc_cv3p wi, orc_v3p f, int nthreads)
{
    Job j = {}; j.in = in; j.lobe = lobe; j.cwi = wi; j.f = f; j.mode = EVAL;
    refh::parallel_for(n, nthreads, range, &j);
}

void ref_batch_disney_pdf(int64_t n, const orc_disney_soa *in, int lobe, orc_cv3p wi, float *pdf, int nthreads)
{
    Job j = {}; j.in = in; j.lobe = lobe; j.cwi = wi; j.pdf = pdf; j.mode = PDF;
    refh::parallel_for(n, nthreads, range, &j);
}

void ref_batch_disney_sample_eval_pdf(int64_t n, const orc_disney_soa *in, int lobe, const float *rx, const float *ry,
                                      orc_v3p wi, orc_v3p f, float *pdf, int nthreads)
{
    Job j = {}; j.in = in; j.lobe = lobe; j.rx = rx; j.ry = ry; j.wi = wi; j.f = f; j.pdf = pdf; j.mode = FUSED;
    refh::parallel_for(n, nthreads, range, &j);
}

/* kind as orc_batch_disney_alt: 0 sampleGTR2AnisoDirection -> out3, 1 sampleGTR2Direction -> out3,
   2 non-VNDF evalSpecularPdf(v) -> out1, 3 D_GTR2(v) -> out1 */
void ref_batch_disney_alt(int64_t n, const orc_disney_soa *in, int kind, const float *rx, const float *ry,
                          orc_cv3p v, orc_v3p out3, float *out1, int nthreads)
{
    Job j = {}; j.in = in; j.lobe = ORC_RAY_GLOSSY; j.rx = rx; j.ry = ry; j.cwi = v; j.wi = out3; j.pdf = out1;
    j.mode = ALT; j.kind = kind;
    refh::parallel_for(n, nthreads, range, &j);
}

}
