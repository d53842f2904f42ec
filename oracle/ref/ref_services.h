/*
 * ref_services.h -- what the harness units under oracle/ref/ share: the per-thread inputs the stand-in
 * services read, and a static-chunk thread pool.  Stand-in semantics are listed in ref_services.cpp.
 */
#ifndef RLS_REF_SERVICES_H
#define RLS_REF_SERVICES_H

#include <stdint.h>

#include <ai.h>

namespace refh
{
/* AiBuildLocalFramePolar returns this tangent as u (v = N x u) */
extern thread_local AtVector tangent;
/* AiShaderEvalParamFunc{Flt,RGB,Vec}: per-thread table indexed by the node's parameter id */
extern thread_local float param_flt[32];
extern thread_local AtRGB param_rgb[32];
extern thread_local AtVector param_vec[32];
/* AiSampler: yields (xi[0], xi[1]) once per iterator */
extern thread_local float sample_xi[2];
extern thread_local int sample_left;
/* AiTrace records the last traced ray */
extern thread_local AtRay traced_ray;
/* what the last AiRefractRay returned */
extern thread_local int refracted;

void parallel_for(int64_t n, int nthreads, void (*fn)(int64_t lo, int64_t hi, void *ctx), void *ctx);
}

#endif
