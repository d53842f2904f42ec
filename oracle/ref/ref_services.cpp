/*
 * ref_services.cpp -- stand-ins for the closed Arnold services the reference closures call.  The
 * semantics are the oracle's documented ones (oracle/rls_oracle.h, PARITY STATUS) and stay unpinned
 * by this build:
 *   AiBuildLocalFramePolar(u, v, N)  u = refh::tangent (the input tangent), v = N x u
 *   AiM4Frame(m, o, u, v, w)         rows u, v, w, o (SssSampler's constructor calls it)
 *   AiMakeRay                        origin, dir (sg->Rd when NULL), maxdist
 *   AiRefractRay(ray, n, n1, n2, sg) Snell about n with i = -ray.dir, eta = n1/n2; the sign of the
 *                                    root is SGN(i . sg->Nf); false (ray unchanged) on total
 *                                    internal reflection.  Same operation order as the oracle's
 *                                    orc_ggx_refract_sample.
 *   AiReflectRay(ray, n, sg)         mirror: 2 (i.n) n - i with i = -ray.dir
 *   AiSampler*                       one sample, refh::sample_xi; inverse count 1
 *   AiTrace / AiTraceBackground      unit environment (colour 1), the ray is recorded
 *   AiShaderEvalParamFunc{Flt,RGB,Vec}  per-thread table lookup
 *   fast_exp                         expf (what orc_batch_gauss assumes)
 * Everything else aborts if called.
 */
#include <stdio.h>
#include <stdlib.h>

#include <thread>
#include <vector>

#include "ref_services.h"

namespace refh
{
thread_local AtVector tangent;
thread_local float param_flt[32];
thread_local AtRGB param_rgb[32];
thread_local AtVector param_vec[32];
thread_local float sample_xi[2];
thread_local int sample_left;
thread_local AtRay traced_ray;
thread_local int refracted;

void parallel_for(int64_t n, int nthreads, void (*fn)(int64_t, int64_t, void *), void *ctx)
{
    if (nthreads <= 1 || n < 2 * (int64_t)nthreads) {
        fn(0, n, ctx);
        return;
    }
    std::vector<std::thread> pool;
    int64_t chunk = (n + nthreads - 1) / nthreads;
    for (int t = 0; t < nthreads; t++) {
        int64_t lo = t * chunk, hi = lo + chunk < n ? lo + chunk : n;
        if (lo >= hi) break;
        pool.emplace_back(fn, lo, hi, ctx);
    }
    for (auto &th : pool) th.join();
}
}

[[noreturn]] static void unreachable(const char *what)
{
    fprintf(stderr, "librls_ref: the closed service %s has no stand-in\n", what);
    abort();
}
#define ABORTS(sig, name) sig { unreachable(name); }

void AiBuildLocalFramePolar(AtVector *u, AtVector *v, const AtVector *N)
{
    *u = refh::tangent;
    *v = AiV3Cross(*N, *u);
}

void AiM4Frame(AtMatrix m, const AtPoint *o, const AtVector *u, const AtVector *v, const AtVector *w)
{
    const AtVector *rows[4] = { u, v, w, o };
    for (int r = 0; r < 4; r++) {
        m[r][0] = rows[r]->x; m[r][1] = rows[r]->y; m[r][2] = rows[r]->z; m[r][3] = r == 3 ? 1.0f : 0.0f;
    }
}

void AiMakeRay(AtRay *ray, AtUInt32 type, const AtPoint *origin, const AtVector *dir, double maxdist,
               const AtShaderGlobals *sg)
{
    ray->type = (AtUInt16)type;
    ray->origin = *origin;
    ray->dir = dir ? *dir : sg->Rd;
    ray->maxdist = maxdist;
}

bool AiRefractRay(AtRay *ray, const AtVector *n, float n1, float n2, const AtShaderGlobals *sg)
{
    const AtVector m = *n;
    const AtVector i = -ray->dir;
    float eta = n1 / n2;
    float c = AiV3Dot(i, m);
    float cosThetaTSqr = 1.0f - eta * eta * (1.0f - c * c);
    refh::refracted = !(cosThetaTSqr < 0.0f);
    if (cosThetaTSqr < 0.0f) {
        return false;
    }
    float sign = (float)SGN(AiV3Dot(i, sg->Nf));
    float k = eta * c - sign * sqrtf(cosThetaTSqr);
    ray->dir = m * k - i * eta;
    return true;
}

void AiReflectRay(AtRay *ray, const AtVector *n, const AtShaderGlobals *)
{
    const AtVector i = -ray->dir;
    float c = AiV3Dot(i, *n);
    ray->dir = *n * (2.0f * c) - i;
}

struct AtSampler { int unused; };
struct AtSamplerIterator { int unused; };
static AtSampler g_sampler;
static AtSamplerIterator g_iter;
AtSampler *AiSampler(int, int) { return &g_sampler; }
void AiSamplerDestroy(AtSampler *) {}
AtSamplerIterator *AiSamplerIterator(const AtSampler *, const AtShaderGlobals *)
{
    refh::sample_left = 1;
    return &g_iter;
}
bool AiSamplerGetSample(AtSamplerIterator *, float *sample)
{
    if (refh::sample_left <= 0) return false;
    refh::sample_left--;
    sample[0] = refh::sample_xi[0];
    sample[1] = refh::sample_xi[1];
    return true;
}
int AiSamplerGetSampleCount(const AtSamplerIterator *) { return 1; }
float AiSamplerGetSampleInvCount(const AtSamplerIterator *) { return 1.0f; }

bool AiTrace(const AtRay *ray, AtScrSample *sample)
{
    refh::traced_ray = *ray;
    sample->color = AI_RGB_WHITE;
    return true;
}
void AiTraceBackground(const AtRay *ray, AtScrSample *sample)
{
    refh::traced_ray = *ray;
    sample->color = AI_RGB_WHITE;
}

float AiShaderEvalParamFuncFlt(AtShaderGlobals *, const AtNode *, int pid) { return refh::param_flt[pid]; }
AtRGB AiShaderEvalParamFuncRGB(AtShaderGlobals *, const AtNode *, int pid) { return refh::param_rgb[pid]; }
AtVector AiShaderEvalParamFuncVec(AtShaderGlobals *, const AtNode *, int pid) { return refh::param_vec[pid]; }

float fast_exp(float x) { return expf(x); }

/* reached only from integrateScatter's MIS combine, which needs the closed probe tracer: unpinned */
ABORTS(void AiM4VectorByMatrixMult(AtVector *, const AtMatrix, const AtVector *), "AiM4VectorByMatrixMult")
ABORTS(void AiBuildLocalFrameShirley(AtVector *, AtVector *, const AtVector *), "AiBuildLocalFrameShirley")
ABORTS(bool AiTraceProbe(const AtRay *, AtShaderGlobals *), "AiTraceProbe")
ABORTS(AtColor AiEvaluateLightSample(AtShaderGlobals *, const void *, AtBRDFEvalSampleFunc, AtBRDFEvalBrdfFunc,
                                     AtBRDFEvalPdfFunc), "AiEvaluateLightSample")
ABORTS(AtColor AiBRDFIntegrate(AtShaderGlobals *, const void *, AtBRDFEvalSampleFunc, AtBRDFEvalBrdfFunc,
                               AtBRDFEvalPdfFunc, AtUInt16), "AiBRDFIntegrate")
ABORTS(void *AiOrenNayarMISCreateData(const AtShaderGlobals *, float), "AiOrenNayarMISCreateData")
ABORTS(AtVector AiOrenNayarMISSample(const void *, float, float), "AiOrenNayarMISSample")
ABORTS(AtColor AiOrenNayarMISBRDF(const void *, const AtVector *), "AiOrenNayarMISBRDF")
ABORTS(float AiOrenNayarMISPDF(const void *, const AtVector *), "AiOrenNayarMISPDF")
ABORTS(void AiLightsPrepare(AtShaderGlobals *), "AiLightsPrepare")
ABORTS(bool AiLightsGetSample(AtShaderGlobals *), "AiLightsGetSample")
ABORTS(bool AiLightGetAffectDiffuse(const AtNode *), "AiLightGetAffectDiffuse")
ABORTS(bool AiLightGetAffectSpecular(const AtNode *), "AiLightGetAffectSpecular")
ABORTS(float AiLightGetDiffuse(const AtNode *), "AiLightGetDiffuse")
ABORTS(float AiLightGetSpecular(const AtNode *), "AiLightGetSpecular")
ABORTS(bool AiStateGetMsgInt(const char *, int *), "AiStateGetMsgInt")
ABORTS(bool AiStateSetMsgInt(const char *, int), "AiStateSetMsgInt")
ABORTS(bool AiStateGetMsgPtr(const char *, void **), "AiStateGetMsgPtr")
ABORTS(bool AiStateSetMsgPtr(const char *, void *), "AiStateSetMsgPtr")
ABORTS(bool AiStateGetMsgFlt(const char *, float *), "AiStateGetMsgFlt")
ABORTS(bool AiStateSetMsgFlt(const char *, float), "AiStateSetMsgFlt")
ABORTS(void *AiShaderGlobalsQuickAlloc(const AtShaderGlobals *, AtUInt32), "AiShaderGlobalsQuickAlloc")
ABORTS(bool AiShaderGlobalsApplyOpacity(AtShaderGlobals *, const AtRGB &), "AiShaderGlobalsApplyOpacity")
ABORTS(void AiAOVSetRGB(AtShaderGlobals *, const char *, const AtRGB &), "AiAOVSetRGB")
ABORTS(void AiShaderGlobalsSetTraceSet(AtShaderGlobals *, const char *, bool), "AiShaderGlobalsSetTraceSet")
ABORTS(void AiShaderGlobalsUnsetTraceSet(AtShaderGlobals *), "AiShaderGlobalsUnsetTraceSet")
ABORTS(AtNode *AiUniverseGetOptions(), "AiUniverseGetOptions")
ABORTS(AtNode *AiNodeLookUpByName(const char *), "AiNodeLookUpByName")
ABORTS(int AiNodeGetInt(const AtNode *, const char *), "AiNodeGetInt")
ABORTS(float AiNodeGetFlt(const AtNode *, const char *), "AiNodeGetFlt")
ABORTS(bool AiNodeGetBool(const AtNode *, const char *), "AiNodeGetBool")
ABORTS(const char *AiNodeGetStr(const AtNode *, const char *), "AiNodeGetStr")
ABORTS(void *AiNodeGetPtr(const AtNode *, const char *), "AiNodeGetPtr")
ABORTS(const char *AiNodeGetStrAtString(const AtNode *, const char *), "AiNodeGetStrAtString")
ABORTS(void *AiNodeGetLocalData(const AtNode *), "AiNodeGetLocalData")
ABORTS(void AiNodeSetLocalData(AtNode *, void *), "AiNodeSetLocalData")
ABORTS(const AtNodeEntry *AiNodeGetNodeEntry(const AtNode *), "AiNodeGetNodeEntry")
ABORTS(const char *AiNodeEntryGetName(const AtNodeEntry *), "AiNodeEntryGetName")
ABORTS(void AiMsgInfo(const char *, ...), "AiMsgInfo")
ABORTS(void AiMsgWarning(const char *, ...), "AiMsgWarning")
ABORTS(void AiMsgError(const char *, ...), "AiMsgError")
ABORTS(const char *AiShaderEvalParamFuncStr(AtShaderGlobals *, const AtNode *, int), "AiShaderEvalParamStr")
ABORTS(bool AiShaderEvalParamFuncBool(AtShaderGlobals *, const AtNode *, int), "AiShaderEvalParamBool")
ABORTS(int AiShaderEvalParamFuncInt(AtShaderGlobals *, const AtNode *, int), "AiShaderEvalParamInt")
ABORTS(void AiParameterFltFunc(AtList *, const char *, float), "AiParameterFlt")
ABORTS(void AiParameterRGBFunc(AtList *, const char *, float, float, float), "AiParameterRGB")
ABORTS(void AiParameterVecFunc(AtList *, const char *, float, float, float), "AiParameterVec")
ABORTS(void AiParameterStrFunc(AtList *, const char *, const char *), "AiParameterStr")
ABORTS(void AiParameterBoolFunc(AtList *, const char *, bool), "AiParameterBool")
ABORTS(void AiParameterIntFunc(AtList *, const char *, int), "AiParameterInt")
ABORTS(void AiMetaDataSetInt(AtMetaDataStore *, const char *, const char *, int), "AiMetaDataSetInt")
ABORTS(void AiMetaDataSetFlt(AtMetaDataStore *, const char *, const char *, float), "AiMetaDataSetFlt")
ABORTS(void AiMetaDataSetStr(AtMetaDataStore *, const char *, const char *, const char *), "AiMetaDataSetStr")
ABORTS(void AiMetaDataSetBool(AtMetaDataStore *, const char *, const char *, bool), "AiMetaDataSetBool")
