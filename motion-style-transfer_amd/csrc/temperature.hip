// Goal-map NLL and hpd at many temperatures in one pass (temperature scaling: the distribution of utils/evaluate.py:128-131, drawn from by
// utils/image_utils.py:110-135, scored as likelihood.hip scores it at one temperature).  Per plane (agent b, step c) and temperature T_k,
// with z = x / T_k, w = sigmoid(z), Z_k = sum w and g the ground-truth pixel:
//   nll[k] = log Z_k - log_sigmoid(z_g)
//   hpd[k] = (sum over {x >= x_g} of w) / Z_k                                  (membership on the raw fp32 logits: the same set at every k)
// One workgroup per plane, ONE pass over HBM for all the temperatures: per loaded pixel only sigmoid(x / T_k) is formed, with no logarithm
// (the two logs per plane and temperature are taken in fp64 at the end).  The temperatures and their reciprocals travel in the argument
// block: wave-uniform values, read with compile-time indices, so they live in scalar registers.  Per-pixel terms are fp32 (sigmoid_term.h,
// shared with likelihood.hip); the running sums, the cross-wave combine and the final logs are fp64, combined in a fixed order: two runs
// give the same bits, and so do two equal temperatures of one call.  The public C ABI is include/ynet_hip.h.
#include "map_plane.h"
#include "../../include/ynet_hip.h"

namespace {

struct SweepArgs {
    const float* x;
    long long bs;
    const float* gt;        // [planes][2] (x, y)
    long long planes;
    int C, H, W, n_temps;
    float t[YNET_SWEEP_MAX_TEMPS], inv_t[YNET_SWEEP_MAX_TEMPS];      // (padded by repeating the last temperature; the padding's sums are dropped)
    float* nll;             // [n_temps][planes] or NULL
    float* hpd;
    int* status;
};

// NT: the number of temperatures carried (2 fp64 sums each): 4, or a multiple of 8 up to 32 -- a 4-point sweep does not pay for 8, a 16-point
// sweep does not carry 64 accumulators.  The vector loop reads U 16-byte vectors per thread and trip and fetches the next trip's before
// it folds this one's: per vector a wave spends NT * 4 sigmoids, far longer than a load takes, so one trip of look-ahead hides HBM and
// the unrolled body (U * 4 * NT sigmoids) stays inside the instruction cache.  A trip past the end of the plane re-reads the plane's
// last vector (never anything outside it) and folds -inf, which adds 0 to every sum: no tail loop, and no branch anywhere in the
// unrolled body (with one, hipcc sinks each load down to its use).  The second launch bound is the waves per SIMD the registers are
// held to at least: 4 up to 16 temperatures (128 VGPRs), 3 at 24, 2 at 32 (the build reaches 3 there).
template <int NT>
__global__ __launch_bounds__(256, NT <= 16 ? 4 : NT == 24 ? 3 : 2) void map_likelihood_sweep_kernel(const SweepArgs a) {
    constexpr int U = NT <= 8 ? 4 : NT == 32 ? 1 : 2;
    __shared__ double ws[4][NT][2];
    __shared__ int wpoison[4];
    const int tid = threadIdx.x;
    const long long plane = blockIdx.x;
    const int n = a.H * a.W;
    const float* __restrict__ p = a.x + (plane / a.C) * a.bs + (plane % a.C) * (long long)n;      // (plane_ptr, spelled out: see map_plane.h)
    const GtPixel g = gt_pixel(a.gt, plane, p, a.H, a.W, a.status, tid);
    const bool in_map = g.in_map;
    const float xg = g.xg;
    // per temperature: sum w, and the sum of w over the members of the hpd region
    double sw[NT], sh[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) sw[k] = sh[k] = 0.0;
    bool poison = false;    // a NaN logit makes the whole plane NaN  (bit-wise ors below: a short-circuit || is a branch)
    auto fold1 = [&](const float v) {
        poison = poison | (v != v);
        const bool m = v >= xg;
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const float w = weight<true>(v, a.inv_t[k], a.t[k]);
            sw[k] += (double)w;
            sh[k] += (double)(m ? w : 0.f);
        }
    };
    auto fold = [&](const float4 v) {
        poison = poison | __builtin_isunordered(v.x, v.y) | __builtin_isunordered(v.z, v.w);
        const bool m0 = v.x >= xg, m1 = v.y >= xg, m2 = v.z >= xg, m3 = v.w >= xg;      // once per pixel, not once per temperature
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const float t = a.t[k], it = a.inv_t[k];
            const float w0 = weight<true>(v.x, it, t), w1 = weight<true>(v.y, it, t), w2 = weight<true>(v.z, it, t), w3 = weight<true>(v.w, it, t);
            sw[k] += (double)((w0 + w1) + (w2 + w3));
            // (the same four values in the same tree as sw: where every pixel is a member the two sums are equal bit for bit, and hpd == 1)
            sh[k] += (double)(((m0 ? w0 : 0.f) + (m1 ? w1 : 0.f)) + ((m2 ? w2 : 0.f) + (m3 ? w3 : 0.f)));
            // (four sigmoids at a time, closed here: left free, hipcc packs the last adds of many temperatures together and parks their
            //  operands in scratch memory meanwhile)
            asm volatile("" : "+v"(sw[k]), "+v"(sh[k]));
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    if ((n & 3) == 0 && (((uintptr_t)p) & 15) == 0) {
        const int n4 = n >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(p);
        const float4 none = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        float4 cur[U], nxt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = p4[min(tid + u * 256, n4 - 1)];
        for (int i = tid; i < n4; i += U * 256) {       // (n4 < 2^29: the look-ahead index stays an int)
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = p4[min(i + (U + u) * 256, n4 - 1)];
            __builtin_amdgcn_sched_barrier(0);      // (the next trip's loads are issued before this trip's arithmetic)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool valid = i + u * 256 < n4;
                float4 v = cur[u];
                v.x = valid ? v.x : none.x;
                v.y = valid ? v.y : none.y;
                v.z = valid ? v.z : none.z;
                v.w = valid ? v.w : none.w;
                fold(v);
                cur[u] = nxt[u];
            }
        }
    } else {        // a plane that does not start on a 16-byte boundary, or does not end on one
        for (int i = tid; i < n; i += 256) fold1(p[i]);
    }
    const int any_poison = __any(poison);
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const double s = wave_sum(sw[k]), h = wave_sum(sh[k]);
        if ((tid & 63) == 0) {
            ws[tid >> 6][k][0] = s;
            ws[tid >> 6][k][1] = h;
        }
    }
    if ((tid & 63) == 0) wpoison[tid >> 6] = any_poison;
    __syncthreads();
    // thread k closes temperature k; its T_k is picked from the scalar registers by a chain of selects (a run-time index into the
    // argument block would put the block into scratch memory)
    float tk = a.t[0], itk = a.inv_t[0];
#pragma unroll
    for (int k = 1; k < NT; ++k) {
        tk = (tid == k) ? a.t[k] : tk;
        itk = (tid == k) ? a.inv_t[k] : itk;
    }
    if (tid < a.n_temps) {
        const double nan = (double)__builtin_nanf("");
        double Z = four_wave_sum(&ws[0][tid][0], 2 * NT);
        const double hs = four_wave_sum(&ws[0][tid][1], 2 * NT);
        if (four_wave_poison(wpoison) || Z == 0.0) Z = nan;
        const long long o = (long long)tid * a.planes + plane;
        if (a.nll != nullptr) {
            double v = nan;
            if (in_map) {
                const double zg = (double)tempered<true>(xg, itk, tk);      // the z of the pass above: a one-pixel plane gives 0
                v = log(Z) - (fmin(zg, 0.0) - log1p(exp(-fabs(zg))));
            }
            a.nll[o] = (float)v;
        }
        if (a.hpd != nullptr) a.hpd[o] = (float)(in_map ? hs / Z : nan);
    }
}

}  // namespace

extern "C" int ynet_map_likelihood_sweep(const float* x, long long batch_stride, const float* gt_xy, long long B, int C, int H, int W,
                                         const float* temperatures, int n_temps, float* nll, float* hpd, int* status, void* stream) {
    YNET_REQUIRE(x != nullptr, "map_likelihood_sweep: null map");
    YNET_REQUIRE(temperatures != nullptr, "map_likelihood_sweep: null temperatures");
    YNET_REQUIRE(n_temps >= 1 && n_temps <= YNET_SWEEP_MAX_TEMPS, "map_likelihood_sweep: %d temperatures, expected 1 .. %d", n_temps,
                 YNET_SWEEP_MAX_TEMPS);
    for (int k = 0; k < n_temps; ++k) {
        const float t = temperatures[k];
        YNET_REQUIRE(t > 0.f && t <= 3.0e38f && 1.f / t <= 3.0e38f,
                     "map_likelihood_sweep: temperature %d: it and its reciprocal must be positive and finite", k);
    }
    if (map_check_shape("map_likelihood_sweep", B, C, H, W) || map_check_pixel_index("map_likelihood_sweep", H, W) ||
        map_check_batch_stride("map_likelihood_sweep", batch_stride, C, H, W))
        return 1;
    YNET_REQUIRE(nll != nullptr || hpd != nullptr, "map_likelihood_sweep: no output asked for");
    YNET_REQUIRE(gt_xy != nullptr, "map_likelihood_sweep: nll and hpd need the ground truth (gt_xy is null)");
    YNET_REQUIRE(status != nullptr, "map_likelihood_sweep: the ground truth needs a status flag (status is null)");
    const long long planes = B * C;
    YNET_REQUIRE(planes < (1ll << 31), "map_likelihood_sweep: too many planes");
    SweepArgs a;
    a.x = x;
    a.bs = batch_stride;
    a.gt = gt_xy;
    a.planes = planes;
    a.C = C;
    a.H = H;
    a.W = W;
    a.n_temps = n_temps;
    for (int k = 0; k < YNET_SWEEP_MAX_TEMPS; ++k) {
        a.t[k] = temperatures[k < n_temps ? k : n_temps - 1];
        a.inv_t[k] = 1.f / a.t[k];
    }
    a.nll = nll;
    a.hpd = hpd;
    a.status = status;
    const dim3 grid((unsigned)planes), block(256);
    if (n_temps <= 4) hipLaunchKernelGGL(map_likelihood_sweep_kernel<4>, grid, block, 0, (hipStream_t)stream, a);
    else if (n_temps <= 8) hipLaunchKernelGGL(map_likelihood_sweep_kernel<8>, grid, block, 0, (hipStream_t)stream, a);
    else if (n_temps <= 16) hipLaunchKernelGGL(map_likelihood_sweep_kernel<16>, grid, block, 0, (hipStream_t)stream, a);
    else if (n_temps <= 24) hipLaunchKernelGGL(map_likelihood_sweep_kernel<24>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(map_likelihood_sweep_kernel<32>, grid, block, 0, (hipStream_t)stream, a);
    return ynet_check_launch("map_likelihood_sweep");
}
