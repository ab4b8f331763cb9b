// The shared base of the per-plane goal-map analytics (likelihood.hip, temperature.hip, compliance.hip, credible.hip, occupancy.hip,
// modes.hip, radial.hip): one workgroup per plane (agent b, step c) of x [B, C, H, W], fp32 per-pixel terms (sigmoid_term.h), fp64 sums combined
// in a fixed order.  A new per-plane entry starts from here; its streaming loop stays its own.
#pragma once
#include "ynet_common.h"
#include "sigmoid_term.h"
#include <math.h>

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// plane = b * C + c of a tensor whose planes are dense (n floats) and whose images lie bs floats apart: a channel view is read in place.
// (likelihood.hip, modes.hip and radial.hip call it.  The sweep, class-mass, credible and occupancy-normalise kernels spell the same expression out:
// through the function hipcc forms their scalar prologue arithmetic differently and renumbers scalar registers inside their loops.)
__device__ __forceinline__ const float* plane_ptr(const float* x, long long bs, int C, int n, long long plane) {
    return x + (plane / C) * bs + (plane % C) * (long long)n;
}

// The ground-truth pixel of a plane (gt: [planes][2] (x, y)), rounded half-even like the patch windows.  Its logit is read only when it
// lies inside the map; otherwise the plane's thread 0 raises the status flag.
struct GtPixel {
    bool in_map;
    float xg;
};

__device__ __forceinline__ GtPixel gt_pixel(const float* gt, long long plane, const float* p, int H, int W, int* status, int tid) {
    const float gx = rintf(gt[2 * plane]), gy = rintf(gt[2 * plane + 1]);
    GtPixel g;
    g.in_map = gx >= 0.f && gx < (float)W && gy >= 0.f && gy < (float)H;      // (false for a NaN coordinate)
    g.xg = INFINITY;
    if (g.in_map) g.xg = p[(int)gy * W + (int)gx];
    else if (tid == 0) atomicExch(status, 1);
    return g;
}

// The cross-wave combine of a 256-thread workgroup: the four waves' fp64 sums (ws: wave 0's, `stride` doubles from wave to wave) in a
// fixed tree, and whether any wave met a NaN logit.
__device__ __forceinline__ double four_wave_sum(const double* ws, int stride) {
    return (ws[0] + ws[stride]) + (ws[2 * stride] + ws[3 * stride]);
}

__device__ __forceinline__ bool four_wave_poison(const int* wpoison) { return (wpoison[0] | wpoison[1] | wpoison[2] | wpoison[3]) != 0; }

// The argument checks the entries share word for word; `what` is the entry's name.  -> 1 with the error set (the caller returns 1), else 0
inline int map_check_temperature(const char* what, float temperature) {
    YNET_REQUIRE(temperature > 0.f && temperature <= 3.0e38f && 1.f / temperature <= 3.0e38f,
                 "%s: the temperature and its reciprocal must be positive and finite", what);
    return 0;
}

inline int map_check_shape(const char* what, long long B, int C, int H, int W) {
    YNET_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: bad shape B=%lld C=%d %dx%d", what, B, C, H, W);
    return 0;
}

inline int map_check_pixel_index(const char* what, int H, int W) {      // (i += 256 stays an int)
    YNET_REQUIRE((long long)H * W <= (1ll << 31) - 2048, "%s: a plane of %dx%d is beyond the 32-bit pixel index", what, H, W);
    return 0;
}

inline int map_check_batch_stride(const char* what, long long batch_stride, int C, int H, int W) {
    YNET_REQUIRE(batch_stride >= (long long)C * H * W, "%s: batch stride %lld below the %d planes of %dx%d of an image", what, batch_stride,
                 C, H, W);
    return 0;
}

}  // namespace
