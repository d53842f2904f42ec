/*
 * ai.h -- stand-in for the Arnold 4.x SDK header, for the reference build only (oracle/Makefile,
 * target `ref`).  Written from the public semantics listed in SURVEY.md Appendix C; it is what the
 * reference translation units compile against when the harness units under oracle/ref/ include them.
 *
 * Inline helpers carry the semantics the oracle assumes (oracle/rls_oracle.h, PARITY STATUS):
 *   AiV3Normalize       multiply by the reciprocal length, 0 when the length is 0
 *   AiV3RotateToFrame   a = a.x*u + a.y*v + a.z*w
 *   SGN(a)              a < 0 ? -1 : 1 (int)
 *   LERP(t, a, b)       (1 - t)*a + b*t, t first
 *   LINEARSTEP(lo,hi,t) CLAMP((t - lo)/(hi - lo), 0, 1)
 *   AI_* constants      fp32 literals
 * Opaque services (AiBuildLocalFramePolar, AiM4*, AiRefractRay, AiSampler*, AiTrace*, ...) are only
 * declared here; oracle/ref/ref_services.cpp defines them.
 *
 * <math.h> (not <cmath> alone): the reference's unqualified exp/log/pow/sqrt then resolve to the float
 * overloads, as on the author's compiler.
 */
#ifndef RLS_REF_AI_H
#define RLS_REF_AI_H

#include <math.h>
#include <stdint.h>
#include <stddef.h>

/* ---- scalars and constants ------------------------------------------------------------------- */
typedef uint8_t  AtByte;
typedef uint16_t AtUInt16;
typedef uint32_t AtUInt32;
typedef int32_t  AtInt32;

#ifndef AI_EPSILON
#define AI_EPSILON    1e-4f
#endif
#define AI_PI         3.14159265f
#define AI_PITIMES2   6.28318530f
#define AI_PIOVER2    1.57079632f
#define AI_ONEOVERPI  0.31830988f
#define AI_ONEOVER2PI 0.15915494f
#define AI_BIG        1e12f

template <typename T> inline T SQR(T a) { return a * a; }
template <typename T> inline T ABS(T a) { return a < 0 ? -a : a; }
template <typename T> inline T MIN(T a, T b) { return a < b ? a : b; }
template <typename T> inline T MAX(T a, T b) { return a > b ? a : b; }
template <typename T> inline T CLAMP(T v, T lo, T hi) { return MAX(lo, MIN(v, hi)); }
template <typename T> inline int SGN(T a) { return a < 0 ? -1 : 1; }
template <typename T1, typename T2> inline T2 LERP(T1 t, T2 a, T2 b) { return (1.0f - t) * a + b * t; }
template <typename T> inline T LINEARSTEP(T lo, T hi, T t) { return CLAMP((t - lo) / (hi - lo), (T)0, (T)1); }

/* ---- vectors ------------------------------------------------------------------------------- */
struct AtVector {
    float x, y, z;
    float &operator[](int i) { return (&x)[i]; }
    const float &operator[](int i) const { return (&x)[i]; }
    AtVector operator+(const AtVector &b) const { return AtVector{x + b.x, y + b.y, z + b.z}; }
    AtVector operator-(const AtVector &b) const { return AtVector{x - b.x, y - b.y, z - b.z}; }
    AtVector operator*(const AtVector &b) const { return AtVector{x * b.x, y * b.y, z * b.z}; }
    AtVector operator/(const AtVector &b) const { return AtVector{x / b.x, y / b.y, z / b.z}; }
    AtVector operator*(float s) const { return AtVector{x * s, y * s, z * s}; }
    AtVector operator/(float s) const { return AtVector{x / s, y / s, z / s}; }
    AtVector operator-() const { return AtVector{-x, -y, -z}; }
    AtVector &operator+=(const AtVector &b) { x += b.x; y += b.y; z += b.z; return *this; }
    AtVector &operator-=(const AtVector &b) { x -= b.x; y -= b.y; z -= b.z; return *this; }
    AtVector &operator*=(const AtVector &b) { x *= b.x; y *= b.y; z *= b.z; return *this; }
    AtVector &operator*=(float s) { x *= s; y *= s; z *= s; return *this; }
    AtVector &operator/=(float s) { x /= s; y /= s; z /= s; return *this; }
    bool operator==(const AtVector &b) const { return x == b.x && y == b.y && z == b.z; }
    bool operator!=(const AtVector &b) const { return !(*this == b); }
};
inline AtVector operator*(float s, const AtVector &a) { return a * s; }
typedef AtVector AtPoint;

struct AtVector2 { float x, y; };
typedef AtVector2 AtPoint2;

struct AtRGB {
    float r, g, b;
    float &operator[](int i) { return (&r)[i]; }
    const float &operator[](int i) const { return (&r)[i]; }
    AtRGB operator+(const AtRGB &o) const { return AtRGB{r + o.r, g + o.g, b + o.b}; }
    AtRGB operator-(const AtRGB &o) const { return AtRGB{r - o.r, g - o.g, b - o.b}; }
    AtRGB operator*(const AtRGB &o) const { return AtRGB{r * o.r, g * o.g, b * o.b}; }
    AtRGB operator/(const AtRGB &o) const { return AtRGB{r / o.r, g / o.g, b / o.b}; }
    AtRGB operator+(float s) const { return AtRGB{r + s, g + s, b + s}; }
    AtRGB operator-(float s) const { return AtRGB{r - s, g - s, b - s}; }
    AtRGB operator*(float s) const { return AtRGB{r * s, g * s, b * s}; }
    AtRGB operator/(float s) const { return AtRGB{r / s, g / s, b / s}; }
    AtRGB operator-() const { return AtRGB{-r, -g, -b}; }
    AtRGB &operator+=(const AtRGB &o) { r += o.r; g += o.g; b += o.b; return *this; }
    AtRGB &operator*=(const AtRGB &o) { r *= o.r; g *= o.g; b *= o.b; return *this; }
    AtRGB &operator*=(float s) { r *= s; g *= s; b *= s; return *this; }
    AtRGB &operator/=(float s) { r /= s; g /= s; b /= s; return *this; }
    bool operator==(const AtRGB &o) const { return r == o.r && g == o.g && b == o.b; }
};
inline AtRGB operator*(float s, const AtRGB &c) { return c * s; }
inline AtRGB operator+(float s, const AtRGB &c) { return AtRGB{s + c.r, s + c.g, s + c.b}; }
inline AtRGB operator-(float s, const AtRGB &c) { return AtRGB{s - c.r, s - c.g, s - c.b}; }
typedef AtRGB AtColor;
struct AtRGBA { float r, g, b, a; };

typedef float AtMatrix[4][4];

#define AI_V3_ZERO    (AtVector{0.0f, 0.0f, 0.0f})
#define AI_RGB_BLACK  (AtRGB{0.0f, 0.0f, 0.0f})
#define AI_RGB_WHITE  (AtRGB{1.0f, 1.0f, 1.0f})
#define AI_RGB_RED    (AtRGB{1.0f, 0.0f, 0.0f})
#define AI_RGB_GREEN  (AtRGB{0.0f, 1.0f, 0.0f})

#define AiV3Create(v, a, b, c) ((v).x = (a), (v).y = (b), (v).z = (c))
inline float AiV3Dot(const AtVector &a, const AtVector &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline AtVector AiV3Cross(const AtVector &a, const AtVector &b)
{
    return AtVector{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
inline float AiV3Length(const AtVector &a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
inline float AiV3Dist(const AtVector &a, const AtVector &b) { return AiV3Length(a - b); }
inline AtVector AiV3Normalize(const AtVector &a)
{
    float tmp = AiV3Length(a);
    if (tmp != 0.0f) tmp = 1.0f / tmp;
    return AtVector{a.x * tmp, a.y * tmp, a.z * tmp};
}
#define AiV3RotateToFrame(a, u, v, w) \
    ((a) = AtVector{(a).x * (u).x + (a).y * (v).x + (a).z * (w).x, \
                    (a).x * (u).y + (a).y * (v).y + (a).z * (w).y, \
                    (a).x * (u).z + (a).y * (v).z + (a).z * (w).z})
inline bool AiV3IsZero(const AtVector &a) { return a.x == 0.0f && a.y == 0.0f && a.z == 0.0f; }
#define AiV3isZero AiV3IsZero
inline bool AiIsFinite(float f) { return isfinite(f); }
inline bool AiV3Exists(const AtVector &a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

inline bool AiColorIsSmall(const AtRGB &c, float eps = AI_EPSILON)
{
    return ABS(c.r) < eps && ABS(c.g) < eps && ABS(c.b) < eps;
}
inline bool AiColorIsZero(const AtRGB &c) { return c.r == 0.0f && c.g == 0.0f && c.b == 0.0f; }
inline AtRGB AiColorClamp(const AtRGB &c, float lo, float hi)
{
    return AtRGB{CLAMP(c.r, lo, hi), CLAMP(c.g, lo, hi), CLAMP(c.b, lo, hi)};
}

/* ---- renderer types -------------------------------------------------------------------------- */
struct AtNode;
struct AtNodeEntry;
struct AtList;
struct AtParamValue;
struct AtSampler;
struct AtSamplerIterator;
struct AtNodeMethods;
struct AtMetaDataStore;

#define AI_RAY_UNDEFINED  0x00
#define AI_RAY_CAMERA     0x01
#define AI_RAY_SHADOW     0x02
#define AI_RAY_REFLECTED  0x04
#define AI_RAY_REFRACTED  0x08
#define AI_RAY_SUBSURFACE 0x10
#define AI_RAY_DIFFUSE    0x20
#define AI_RAY_GLOSSY     0x40
#define AI_TYPE_RGB       0x05
#define AI_NODE_SHADER    0x0100

struct AtRay { AtUInt16 type; AtPoint origin; AtVector dir; double maxdist; };
struct AtScrSample { AtRGB color; float alpha; AtPoint point; AtVector normal; double z; };
struct AtShaderGlobalsOut { AtRGB RGB; };

struct AtShaderGlobals {
    AtPoint Ro, P, Po;
    AtVector Rd, N, Nf, Ng, Ngf, Ns;
    AtVector dPdu, dPdv, dPdx, dPdy, dNdx, dNdy;
    float Rl, area, bu, bv;
    AtUInt32 fi;
    AtUInt16 Rt;
    AtByte Rr, Rr_refr, Rr_diff, Rr_gloss;
    bool fhemi;
    AtNode *Op, *shader, *Lp;
    AtShaderGlobals *psg;
    AtShaderGlobalsOut out;
    AtRGB out_opacity;
};

/* ---- opaque services: declared only ---------------------------------------------------------- */
void AiBuildLocalFramePolar(AtVector *u, AtVector *v, const AtVector *N);
void AiBuildLocalFrameShirley(AtVector *u, AtVector *v, const AtVector *N);
void AiM4Frame(AtMatrix m, const AtPoint *o, const AtVector *u, const AtVector *v, const AtVector *w);
void AiM4VectorByMatrixMult(AtVector *out, const AtMatrix m, const AtVector *in);
void AiMakeRay(AtRay *ray, AtUInt32 type, const AtPoint *origin, const AtVector *dir, double maxdist,
               const AtShaderGlobals *sg);
bool AiRefractRay(AtRay *ray, const AtVector *n, float n1, float n2, const AtShaderGlobals *sg);
void AiReflectRay(AtRay *ray, const AtVector *n, const AtShaderGlobals *sg);
bool AiTrace(const AtRay *ray, AtScrSample *sample);
void AiTraceBackground(const AtRay *ray, AtScrSample *sample);
bool AiTraceProbe(const AtRay *ray, AtShaderGlobals *hit);

AtSampler *AiSampler(int nsamples, int ndim);
void AiSamplerDestroy(AtSampler *sampler);
AtSamplerIterator *AiSamplerIterator(const AtSampler *sampler, const AtShaderGlobals *sg);
bool AiSamplerGetSample(AtSamplerIterator *iter, float *sample);
int AiSamplerGetSampleCount(const AtSamplerIterator *iter);
float AiSamplerGetSampleInvCount(const AtSamplerIterator *iter);

typedef AtVector (*AtBRDFEvalSampleFunc)(const void *brdf, float rx, float ry);
typedef AtColor (*AtBRDFEvalBrdfFunc)(const void *brdf, const AtVector *indir);
typedef float (*AtBRDFEvalPdfFunc)(const void *brdf, const AtVector *indir);
AtColor AiEvaluateLightSample(AtShaderGlobals *sg, const void *brdf, AtBRDFEvalSampleFunc s,
                              AtBRDFEvalBrdfFunc b, AtBRDFEvalPdfFunc p);
AtColor AiBRDFIntegrate(AtShaderGlobals *sg, const void *brdf, AtBRDFEvalSampleFunc s, AtBRDFEvalBrdfFunc b,
                        AtBRDFEvalPdfFunc p, AtUInt16 ray_type);
void *AiOrenNayarMISCreateData(const AtShaderGlobals *sg, float r);
AtVector AiOrenNayarMISSample(const void *brdf, float rx, float ry);
AtColor AiOrenNayarMISBRDF(const void *brdf, const AtVector *indir);
float AiOrenNayarMISPDF(const void *brdf, const AtVector *indir);
void AiLightsPrepare(AtShaderGlobals *sg);
bool AiLightsGetSample(AtShaderGlobals *sg);
bool AiLightGetAffectDiffuse(const AtNode *light);
bool AiLightGetAffectSpecular(const AtNode *light);
float AiLightGetDiffuse(const AtNode *light);
float AiLightGetSpecular(const AtNode *light);

bool AiStateGetMsgInt(const char *name, int *val);
bool AiStateSetMsgInt(const char *name, int val);
bool AiStateGetMsgPtr(const char *name, void **val);
bool AiStateSetMsgPtr(const char *name, void *val);
bool AiStateGetMsgFlt(const char *name, float *val);
bool AiStateSetMsgFlt(const char *name, float val);
void *AiShaderGlobalsQuickAlloc(const AtShaderGlobals *sg, AtUInt32 size);
bool AiShaderGlobalsApplyOpacity(AtShaderGlobals *sg, const AtRGB &opacity);
void AiAOVSetRGB(AtShaderGlobals *sg, const char *name, const AtRGB &val);

AtNode *AiUniverseGetOptions();
AtNode *AiNodeLookUpByName(const char *name);
int AiNodeGetInt(const AtNode *node, const char *param);
float AiNodeGetFlt(const AtNode *node, const char *param);
bool AiNodeGetBool(const AtNode *node, const char *param);
const char *AiNodeGetStr(const AtNode *node, const char *param);
void *AiNodeGetLocalData(const AtNode *node);
void AiNodeSetLocalData(AtNode *node, void *data);
const AtNodeEntry *AiNodeGetNodeEntry(const AtNode *node);
const char *AiNodeEntryGetName(const AtNodeEntry *entry);

void AiMsgInfo(const char *fmt, ...);
void AiMsgWarning(const char *fmt, ...);
void AiMsgError(const char *fmt, ...);

void *AiNodeGetPtr(const AtNode *node, const char *param);
const char *AiNodeGetStrAtString(const AtNode *node, const char *param);
void AiShaderGlobalsSetTraceSet(AtShaderGlobals *sg, const char *set, bool inclusive);
void AiShaderGlobalsUnsetTraceSet(AtShaderGlobals *sg);
/* GaussianProfile's exponential (ref_services.cpp) */
float fast_exp(float x);

/* shader parameters: evaluated through the harness's table (ref_services.cpp) */
float AiShaderEvalParamFuncFlt(AtShaderGlobals *sg, const AtNode *node, int pid);
AtRGB AiShaderEvalParamFuncRGB(AtShaderGlobals *sg, const AtNode *node, int pid);
AtVector AiShaderEvalParamFuncVec(AtShaderGlobals *sg, const AtNode *node, int pid);
const char *AiShaderEvalParamFuncStr(AtShaderGlobals *sg, const AtNode *node, int pid);
bool AiShaderEvalParamFuncBool(AtShaderGlobals *sg, const AtNode *node, int pid);
int AiShaderEvalParamFuncInt(AtShaderGlobals *sg, const AtNode *node, int pid);
#define AiShaderEvalParamFlt(pid)  AiShaderEvalParamFuncFlt(sg, node, pid)
#define AiShaderEvalParamRGB(pid)  AiShaderEvalParamFuncRGB(sg, node, pid)
#define AiShaderEvalParamVec(pid)  AiShaderEvalParamFuncVec(sg, node, pid)
#define AiShaderEvalParamStr(pid)  AiShaderEvalParamFuncStr(sg, node, pid)
#define AiShaderEvalParamBool(pid) AiShaderEvalParamFuncBool(sg, node, pid)
#define AiShaderEvalParamInt(pid)  AiShaderEvalParamFuncInt(sg, node, pid)

/* node declaration */
void AiParameterFltFunc(AtList *params, const char *name, float v);
void AiParameterRGBFunc(AtList *params, const char *name, float r, float g, float b);
void AiParameterVecFunc(AtList *params, const char *name, float x, float y, float z);
void AiParameterStrFunc(AtList *params, const char *name, const char *v);
void AiParameterBoolFunc(AtList *params, const char *name, bool v);
void AiParameterIntFunc(AtList *params, const char *name, int v);
#define AiParameterFLT(n, v)          AiParameterFltFunc(params, n, v)
#define AiParameterFlt(n, v)          AiParameterFltFunc(params, n, v)
#define AiParameterRGB(n, r, g, b)    AiParameterRGBFunc(params, n, r, g, b)
#define AiParameterVec(n, x, y, z)    AiParameterVecFunc(params, n, x, y, z)
#define AiParameterVEC(n, x, y, z)    AiParameterVecFunc(params, n, x, y, z)
#define AiParameterSTR(n, v)          AiParameterStrFunc(params, n, v)
#define AiParameterBOOL(n, v)         AiParameterBoolFunc(params, n, v)
#define AiParameterBool(n, v)         AiParameterBoolFunc(params, n, v)
#define AiParameterINT(n, v)          AiParameterIntFunc(params, n, v)
void AiMetaDataSetInt(AtMetaDataStore *mds, const char *param, const char *name, int v);
void AiMetaDataSetStr(AtMetaDataStore *mds, const char *param, const char *name, const char *v);
void AiMetaDataSetFlt(AtMetaDataStore *mds, const char *param, const char *name, float v);
void AiMetaDataSetBool(AtMetaDataStore *mds, const char *param, const char *name, bool v);

#define AI_SHADER_NODE_EXPORT_METHODS(name) \
    static void Parameters(AtList *params, AtMetaDataStore *mds); \
    static void Initialize(AtNode *node, AtParamValue *params); \
    static void Update(AtNode *node, AtParamValue *params); \
    static void Finish(AtNode *node); \
    static void Evaluate(AtNode *node, AtShaderGlobals *sg); \
    AtNodeMethods *name = nullptr
#define node_parameters  static void Parameters(AtList *params, AtMetaDataStore *mds)
#define node_initialize  static void Initialize(AtNode *node, AtParamValue *params)
#define node_update      static void Update(AtNode *node, AtParamValue *params)
#define node_finish      static void Finish(AtNode *node)
#define shader_evaluate  static void Evaluate(AtNode *node, AtShaderGlobals *sg)

struct AtNodeLib { int node_type; int output_type; const char *name; AtNodeMethods *methods; char version[32]; };
#define AI_VERSION "4.2.11.0"
#define node_loader extern "C" bool NodeLoader(int i, AtNodeLib *node)

#endif
