// Gradients with respect to the NETWORK INPUT (saliency, models/trainer.py:354-516 forward_test / _forward_batch) and the
// range-scaled Gaussian noise of forward_test(noisy_std_frac) (models/trainer.py:380-381, 472-479).
//
//   input_grad_kernel<CS, CM>   data gradient of the first 3 x 3 convolution (padding 1) whose input is the channel concatenation
//                               [scene CS | motion CM]: dx = conv3x3(dy [where relu_of > 0], mode-1 packed filter).  One thread per pixel of a
//                               32 x 8 tile, one workgroup per (tile, chunk of IG_IMGS images); the filter [cout][9][CS + CM] sits in
//                               LDS (read as broadcasts), dy is read straight from global memory (its 3 x 3 neighbourhoods overlap
//                               within the tile: L1 / L2 hits).  Motion channels are written per image; the scene channels are
//                               summed over the chunk's images in image order and written as the chunk's partial (or straight to
//                               d_scene when there is one chunk).
//   input_grad_combine_kernel   d_scene = sum of the chunk partials in chunk order.  No atomics: the two launches give the same
//                               bits every run.
//   avgpool_pyramid_bwd_kernel  backward of [x, AvgPool2d(2)(x), ..., AvgPool2d(2^L)(x)] (models/trainer.py:497-500): dx = sum over the
//                               levels of g_l at (h >> l, w >> l) / 4^l, level order 0, 1, ... (g_0 may be NULL: zero)
//   range_minmax_kernel / range_noise_kernel
//                               out = x + N(0, 1) * frac * (max(x) - min(x)); min / max per workgroup, then every workgroup of the
//                               second launch reduces the (fixed number of) partials itself.  N(0, 1) by Box-Muller in fp64 from the
//                               project's Philox4x32-10 (csrc/sample.hip, oracle/ynet_oracle.py:_philox4x32_10): element i takes
//                               u1 from counter (i lo, i hi, 0, 2), u2 from (i lo, i hi, 1, 2), each u = ((x0 >> 5) 2^26 + (x1 >> 6)
//                               + 0.5) 2^-53 -- reproducible from the seed alone, NOT the stream torch's normal_ draws.
// All offsets are 64-bit (planes beyond 2 and 4 GiB).
#include "ynet_common.h"
#include <math.h>

#define IG_TW 32
#define IG_TH 8
#define IG_IMGS 4
#define IG_MAX_COUT 64
#define IG_CIN_PAD 16        // mode-1 packing (conv_mfma.hip: pack_weight_kernel): rows = cout padded to 16, + 16 slack rows
#define IG_COL_PAD 64        //                                                    cols = cin padded to 64

template <int CS, int CM>
__global__ __launch_bounds__(256) void input_grad_kernel(const float* __restrict__ dy, const float* __restrict__ relu_of, const float* __restrict__ wp,
                                                         float* __restrict__ d_scene, float* __restrict__ d_motion,
                                                         float* __restrict__ part, int B, int H, int W, int cout, int cols_pad) {
    constexpr int CIN = CS + CM;
    extern __shared__ float w_s[];      // [cout][9][CIN]
    for (int i = threadIdx.x; i < cout * 9 * CIN; i += 256) {
        const int ci = i % CIN, t = (i / CIN) % 9, co = i / (CIN * 9);
        w_s[i] = wp[((long long)co * 9 + t) * cols_pad + ci];
    }
    __syncthreads();
    const int tiles_x = W / IG_TW;
    const int w = (blockIdx.x % tiles_x) * IG_TW + (threadIdx.x % IG_TW);
    const int h = (blockIdx.x / tiles_x) * IG_TH + (threadIdx.x / IG_TW);
    const long long plane = (long long)H * W;
    const long long pix = (long long)h * W + w;
    const int b0 = blockIdx.y * IG_IMGS;
    const int b1 = min(B, b0 + IG_IMGS);
    float acc_s[CS > 0 ? CS : 1];
#pragma unroll
    for (int c = 0; c < CS; ++c) acc_s[c] = 0.f;
    for (int b = b0; b < b1; ++b) {
        float acc[CIN];
#pragma unroll
        for (int c = 0; c < CIN; ++c) acc[c] = 0.f;
        const long long img = (long long)b * cout * plane;
        for (int co = 0; co < cout; ++co) {
            const float* p = dy + img + (long long)co * plane;
            const float* m = relu_of ? relu_of + img + (long long)co * plane : nullptr;
            float v[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int hh = h + t / 3 - 1, ww = w + t % 3 - 1;
                const bool in = hh >= 0 && hh < H && ww >= 0 && ww < W;
                const long long q = (long long)hh * W + ww;
                v[t] = (in && (!m || m[q] > 0.f)) ? p[q] : 0.f;
            }
            const float* wc = w_s + co * 9 * CIN;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
#pragma unroll
                for (int c = 0; c < CIN; ++c) acc[c] = fmaf(v[t], wc[t * CIN + c], acc[c]);
            }
        }
        if (CM > 0 && d_motion) {
            float* o = d_motion + (long long)b * CM * plane + pix;
#pragma unroll
            for (int c = 0; c < CM; ++c) o[(long long)c * plane] = acc[CS + c];
        }
#pragma unroll
        for (int c = 0; c < CS; ++c) acc_s[c] += acc[c];
    }
    if (CS > 0 && d_scene) {
        float* o = (gridDim.y > 1 ? part + (long long)blockIdx.y * CS * plane : d_scene) + pix;
#pragma unroll
        for (int c = 0; c < CS; ++c) o[(long long)c * plane] = acc_s[c];
    }
}

__global__ __launch_bounds__(256) void input_grad_combine_kernel(const float* __restrict__ part, float* __restrict__ d_scene,
                                                                 int nchunk, long long n) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float a = part[i];
        for (int k = 1; k < nchunk; ++k) a += part[i + (long long)k * n];
        d_scene[i] = a;
    }
}

template <int CS, int CM>
static void launch_input_grad(const float* dy, const float* relu_of, const float* wp, float* d_scene, float* d_motion, float* part, int B, int H, int W,
                              int cout, int cols_pad, int nchunk, hipStream_t s) {
    const dim3 grid((unsigned)((W / IG_TW) * (H / IG_TH)), (unsigned)nchunk);
    const size_t lds = (size_t)cout * 9 * (CS + CM) * sizeof(float);
    hipLaunchKernelGGL((input_grad_kernel<CS, CM>), grid, dim3(256), lds, s, dy, relu_of, wp, d_scene, d_motion, part, B, H, W, cout, cols_pad);
}

struct PyrGrads {
    const float* g[6];
};

__global__ __launch_bounds__(256) void avgpool_pyramid_bwd_kernel(PyrGrads g, int nlev, float* __restrict__ dx, long long N, int H, int W) {
    const long long n = N * H * W;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int w = (int)(i % W), h = (int)((i / W) % H);
        const long long img = i / ((long long)H * W);
        float a = g.g[0] ? g.g[0][i] : 0.f;
        for (int l = 1; l < nlev; ++l) {
            const int hl = H >> l, wl = W >> l;
            a += g.g[l][(img * hl + (h >> l)) * wl + (w >> l)] * (1.0f / (float)(1 << (2 * l)));
        }
        dx[i] = a;
    }
}

// ---- range-scaled noise --------------------------------------------------------------------------------------------------
#define RN_PARTS 512

__device__ __forceinline__ void rn_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned& o0,
                                          unsigned& o1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
        const unsigned n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        const unsigned n3 = (unsigned)p0;
        c0 = n0;
        c1 = n1;
        c2 = n2;
        c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o0 = c0;
    o1 = c1;
}

__device__ __forceinline__ double rn_uniform(long long i, unsigned row, unsigned k0, unsigned k1) {
    unsigned x0, x1;
    rn_philox((unsigned)i, (unsigned)((unsigned long long)i >> 32), row, 2u, k0, k1, x0, x1);
    return ((double)(x0 >> 5) * 67108864.0 + (double)(x1 >> 6) + 0.5) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ void block_minmax(float& lo, float& hi, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = lo;
        red[4 + (threadIdx.x >> 6)] = hi;
    }
    __syncthreads();
    lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
}

__global__ __launch_bounds__(256) void range_minmax_kernel(const float* __restrict__ x, long long n, float* __restrict__ ws) {
    __shared__ float red[8];
    float lo = INFINITY, hi = -INFINITY;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = x[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    block_minmax(lo, hi, red);
    if (threadIdx.x == 0) {
        ws[2 * blockIdx.x] = lo;
        ws[2 * blockIdx.x + 1] = hi;
    }
}

__global__ __launch_bounds__(256) void range_noise_kernel(const float* __restrict__ x, float* __restrict__ out, long long n, int nparts,
                                                          float frac, unsigned k0, unsigned k1, const float* __restrict__ ws) {
    __shared__ float red[8];
    float lo = INFINITY, hi = -INFINITY;
    for (int p = threadIdx.x; p < nparts; p += 256) {
        lo = fminf(lo, ws[2 * p]);
        hi = fmaxf(hi, ws[2 * p + 1]);
    }
    block_minmax(lo, hi, red);
    const float std_ = frac * (hi - lo);
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double u1 = rn_uniform(i, 0u, k0, k1), u2 = rn_uniform(i, 1u, k0, k1);
        const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
        out[i] = x[i] + (float)z * std_;
    }
}

extern "C" {

int ynet_input_grad_supported(int B, int H, int W, int cout, int c_s, int c_m) {
    const bool cs_ok = c_s == 0 || c_s == 6 || c_s == 16;
    const bool cm_ok = c_m == 0 || c_m == 5 || c_m == 8;
    return (cs_ok && cm_ok && c_s + c_m > 0 && (cout == 8 || cout == 16 || cout == 32 || cout == 64) && B >= 1 && B <= 65535 * IG_IMGS && H >= 32 && W >= 32 &&
            H % 32 == 0 && W % 32 == 0 && (long long)(W / IG_TW) * (H / IG_TH) <= 0x7fffffffll) ? 1 : 0;
}

long long ynet_input_grad_workspace_floats(int B, int H, int W, int c_s) {
    const long long nchunk = (B + IG_IMGS - 1) / IG_IMGS;
    return nchunk > 1 ? nchunk * c_s * (long long)H * W : 0;
}

int ynet_input_grad(const float* dy, const float* relu_of, const float* wp, float* d_scene, float* d_motion, float* workspace, int B, int H, int W, int cout,
                    int c_s, int c_m, void* stream) {
    YNET_REQUIRE(ynet_input_grad_supported(B, H, W, cout, c_s, c_m),
                 "input_grad: shape not served (B %d, %dx%d, cout %d, scene %d, motion %d channels): scene 0 / 6 / 16, motion 0 / 5 / 8, "
                 "cout 8 / 16 / 32 / 64, H and W multiples of 32", B, H, W, cout, c_s, c_m);
    YNET_REQUIRE(dy && wp, "input_grad: null dy / filter");
    YNET_REQUIRE(d_scene || d_motion, "input_grad: no destination");
    YNET_REQUIRE(!d_scene || c_s > 0, "input_grad: d_scene given but the input has no scene channels");
    YNET_REQUIRE(!d_motion || c_m > 0, "input_grad: d_motion given but the input has no motion channels");
    const int nchunk = (B + IG_IMGS - 1) / IG_IMGS;
    YNET_REQUIRE(!d_scene || nchunk == 1 || workspace, "input_grad: the batch sum needs ynet_input_grad_workspace_floats() floats of workspace");
    const int cols_pad = ((c_s + c_m + IG_COL_PAD - 1) / IG_COL_PAD) * IG_COL_PAD;
    hipStream_t s = (hipStream_t)stream;
#define IG_CASE(S, M) \
    if (c_s == S && c_m == M) launch_input_grad<S, M>(dy, relu_of, wp, d_scene, d_motion, workspace, B, H, W, cout, cols_pad, nchunk, s)
    IG_CASE(6, 8); else IG_CASE(6, 5); else IG_CASE(16, 8); else IG_CASE(16, 5);
    else IG_CASE(6, 0); else IG_CASE(16, 0); else IG_CASE(0, 8); else IG_CASE(0, 5);
#undef IG_CASE
    int rc = ynet_check_launch("input_grad");
    if (rc || !d_scene || nchunk == 1) return rc;
    const long long n = (long long)c_s * H * W;
    long long blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(input_grad_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, s, workspace, d_scene, nchunk, n);
    return ynet_check_launch("input_grad (batch sum)");
}

int ynet_avgpool_pyramid_bwd(const float* const* grads /* host array of nlev device pointers */, int nlev, float* dx, long long N, int H, int W, void* stream) {
    YNET_REQUIRE(grads && dx && nlev >= 1 && nlev <= 6 && N > 0, "avgpool_pyramid_bwd: bad arguments (levels %d)", nlev);
    YNET_REQUIRE(H % (1 << (nlev - 1)) == 0 && W % (1 << (nlev - 1)) == 0, "avgpool_pyramid_bwd: %dx%d not divisible by 2^%d", H, W, nlev - 1);
    PyrGrads a{};
    for (int l = 0; l < nlev; ++l) {
        YNET_REQUIRE(l == 0 || grads[l] != nullptr, "avgpool_pyramid_bwd: gradient of level %d is null", l);
        a.g[l] = grads[l];
    }
    long long blocks = (N * H * W + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(avgpool_pyramid_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, nlev, dx, N, H, W);
    return ynet_check_launch("avgpool_pyramid_bwd");
}

long long ynet_range_noise_workspace_floats(void) { return 2 * RN_PARTS; }

int ynet_add_range_noise(const float* x, float* out, long long n, float frac, unsigned long long seed, float* workspace, void* stream) {
    YNET_REQUIRE(x && out && workspace && n > 0, "add_range_noise: bad arguments");
    YNET_REQUIRE(frac >= 0.f && isfinite(frac), "add_range_noise: frac must be finite and >= 0");
    long long blocks = (n + 255) / 256;
    const int parts = (int)(blocks > RN_PARTS ? RN_PARTS : blocks);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(range_minmax_kernel, dim3(parts), dim3(256), 0, s, x, n, workspace);
    int rc = ynet_check_launch("add_range_noise (min / max)");
    if (rc) return rc;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(range_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, out, n, parts, frac, (unsigned)(seed & 0xffffffffull),
                       (unsigned)(seed >> 32), workspace);
    return ynet_check_launch("add_range_noise");
}

}  // extern "C"
