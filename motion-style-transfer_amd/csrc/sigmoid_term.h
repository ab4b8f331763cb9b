// The per-pixel fp32 arithmetic of the goal-map distribution sigmoid(x / T), shared by the per-plane analytics kernels through
// map_plane.h (likelihood.hip, temperature.hip, compliance.hip, credible.hip, occupancy.hip): one copy, so that every kernel forms the
// same z and the same w from the same logit.  (modes.hip includes it through map_plane.h too, and keeps its own weight: see there.)
#pragma once
#include <hip/hip_runtime.h>

namespace {

// z = x / T as sigmoid_temp_kernel (glue.hip) forms it for the sampler, in fp32: the product with 1 / T, corrected by its exact residual --
// the correctly rounded quotient (almost always) in three operations instead of the ten of an IEEE division.
template <bool DIVIDE>
__device__ __forceinline__ float tempered(float x, float inv_t, float t) {
    if (!DIVIDE) return x;
    const float z = x * inv_t;
    const float zc = __builtin_fmaf(__builtin_fmaf(-z, t, x), inv_t, z);
    return (zc == zc) ? zc : z;        // (infinite x: the residual is NaN, the product is the answer)
}

// One logit in fp32.  With a = |z|, e = exp(-a), u = 1 + e:   w = sigmoid(z) = 1 / u (z >= 0), e / u (z < 0).
// e comes from v_exp_f32 on the rounded product a * log2(e), corrected to first order by the product's exact residual.  a is clamped
// to 104 on the way: exp2 of -150 is 0 whatever the denormal mode, so a -inf logit has e = 0 and w = 0 exactly and adds 0 to every sum
// (between 87.4 and 104 the sigmoid is below fp32's normal range: a denormal or 0).  A NaN comes out as w = 0 here; the caller tracks
// NaNs itself.  e, u and ru = 1 / u are kept for log_sigmoid (likelihood.hip: logit_term).
struct SigmoidTerm {
    float e, u, ru;
};

__device__ __forceinline__ SigmoidTerm sigmoid_term(float z) {
    const float a = __builtin_fabsf(z);
    const float L2E = 1.44269502162933349609375f, L2El = 1.925963033500011e-8f;      // log2(e) = L2E + L2El
    const float ac = __builtin_fminf(a, 104.f);
    const float p = -ac * L2E;
    const float r = __builtin_fmaf(-ac, L2E, -p) - ac * L2El;
    float e = __builtin_amdgcn_exp2f(p);
    e = __builtin_fmaf(e, r * 0.693147182464599609375f, e);
    const float u = 1.f + e;
    const float ru = __builtin_amdgcn_rcpf(u);
    SigmoidTerm o;
    o.e = e;
    o.u = u;
    o.ru = ru;
    return o;
}

// w from the parts above (apart from them, so that a caller that also wants log_sigmoid forms its terms in the order it always did)
__device__ __forceinline__ float sigmoid_weight(float z, const SigmoidTerm s) { return (z >= 0.f) ? s.ru : s.e * s.ru; }

// w = sigmoid(x / T) alone, for the kernels that take no logarithm
template <bool DIVIDE>
__device__ __forceinline__ float weight(float x, float inv_t, float t) {
    const float z = tempered<DIVIDE>(x, inv_t, t);
    return sigmoid_weight(z, sigmoid_term(z));
}

}  // namespace
