// The per-element Adam update (torch.optim.Adam defaults as constructed at TrainingNeural.py:337 and stepped at :386),
// shared by adam.hip (gmc_adam_f32, gmc_adam_devstep_*: one sweep over a flat buffer) and instance.hip
// (gmc_inst_adam_f32: the same sweep segmented by graph).  One definition, so a graph's parameters take the same bits
// from either sweep.
#pragma once
#include "gmc_common.h"
#include <math.h>

namespace gmc {

struct AdamArgs {
    float *p;
    const float *g;
    float *m;
    float *v;
    long n;
    float one_minus_b1, b2, one_minus_b2, step_size, bc2_sqrt, eps;
};

// What the host derives for step number `step` (>= 1), in double as torch does in Python floats, before rounding to fp32.
static inline AdamArgs adam_args(float *p, const float *g, float *m, float *v, long n, double lr, double beta1,
                                 double beta2, double eps, int step) {
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    return AdamArgs{p, g, m, v, n, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                    (float)(lr / bc1), (float)sqrt(bc2), (float)eps};
}

__device__ __forceinline__ void adam1(float &p, float g, float &m, float &v, const AdamArgs &a) {
    m = m + (g - m) * a.one_minus_b1;                 // exp_avg.lerp_(grad, 1-beta1)
    v = fmaf(a.one_minus_b2 * g, g, v * a.b2);        // exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p - a.step_size * (m / denom);                // param.addcdiv_(m, denom, -step_size)
}

__device__ __forceinline__ void adam4(float4 &p, const float4 &g, float4 &m, float4 &v, const AdamArgs &a) {
    adam1(p.x, g.x, m.x, v.x, a); adam1(p.y, g.y, m.y, v.y, a);
    adam1(p.z, g.z, m.z, v.z, a); adam1(p.w, g.w, m.w, v.w, a);
}

}  // namespace gmc
