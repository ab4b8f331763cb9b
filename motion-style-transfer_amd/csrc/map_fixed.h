// The fixed-point masses of the goal-map analytics that sum with integer atomics (credible.hip, radial.hip): a plane's fp32 weights
// as 64-bit integers scaled by a power of two that puts the plane's largest weight into [2^FRAC, 2^(FRAC + 1)).  Formed from w's own
// mantissa and exponent with shifts, so exact whatever the denormal mode; integer adds are order-free, so LDS atomics give the same bits
// run after run.  One copy, so that both kernels truncate the same weight to the same integer.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef unsigned long long u64;

// w = mant * 2^(ex - 150), 0 <= mant < 2^24 (ex = 1 for a denormal)
__device__ __forceinline__ void split(float w, unsigned& mant, int& ex) {
    const unsigned b = __float_as_uint(w) & 0x7fffffffu;
    const unsigned e = b >> 23;
    mant = (b & 0x7fffffu) | (e ? 0x800000u : 0u);
    ex = e ? (int)e : 1;
}

// trunc(w * 2^(k0 + 150)), by shifts.  k0 puts the plane's largest w into [2^40, 2^41); a w an ulp above it (the fp32 sigmoid is
// monotone up to its last bits only) still stays far below 2^42.
__device__ __forceinline__ u64 fixed(float w, int k0) {
    unsigned mant;
    int ex;
    split(w, mant, ex);
    const int s = ex + k0;
    return s >= 0 ? ((u64)mant << (s > 39 ? 39 : s)) : (s > -32 ? (u64)(mant >> -s) : 0ull);
}

// the k0 of `fixed` for a plane whose largest weight is wmax > 0: mant << (ex + k0) lies in [2^frac, 2^(frac + 1))
__device__ __forceinline__ int fixed_scale(float wmax, int frac) {
    unsigned mant;
    int ex;
    split(wmax, mant, ex);
    return frac - (31 - __builtin_clz(mant)) - ex;
}

}  // namespace
