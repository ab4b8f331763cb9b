// Marginals of the goal map: the x- and y-marginal of the distribution sigmoid(pred_goal_map / T) (utils/evaluate.py:128-131 builds it,
// utils/image_utils.py:110-135 draws from it) -- the column sums and the row sums of every normalised plane -- and, against the rounded
// ground truth g, the per-axis continuous ranked probability score and probability integral transform.  Per plane (agent b, step c), with
// z = x / T, w = sigmoid(z), f = the fixed-point mass of w (map_fixed.h) and N = sum f:
//   col[j] = (sum over rows of f) / N        row[i] = (sum over columns of f) / N
//   crps   = sum_{t < g} F(t)^2 + sum_{t >= g} (1 - F(t))^2 over the integer grid, F = the marginal's CDF (0 below the map, 1 from its last bin on)
//   pit    = (F(g - 1), F(g))
// One workgroup per plane, two passes, the second one served by the caches (radial.hip's structure):
//   pass 1   the largest logit and the NaN flag: the scale of the fixed point
//   pass 2   per pixel w and f, added to W column bins and H row bins of 64-bit integers in LDS
// then one workgroup prefix scan per axis turns the bins into the integer CDF, from which the shares, the CRPS terms (fp64 per thread,
// combined in the fixed tree of map_plane.h) and the PIT follow.  Integer adds are order-free: two runs give the same bits, whichever
// path a plane takes, and there is no floating-point atomic.
// Pass 2 reaches the bins with 64-bit integer LDS atomics: one per pixel on its column bin (adjacent lanes, adjacent bins) and radial.hip's
// one atomic per run of equal bins for the rows; a 16-byte vector may run over a row end (W % 4 != 0) and over several (W < 4), hence
// row_col and the carry chain.  (A register path for planes whose W divides 1024 -- a thread's four columns are then the same in every
// iteration, so four column sums in registers, and the row sum by a segmented 64-bit xor-shuffle reduction over the W / 4 lanes that
// share a row -- measured no faster: 202.3 against 200.6 us at 128 x 12 planes of 256 x 256, T = 1, within a spread of 11 us, the same
// bits; profiles/marginals_register_ab.json, DESIGN.md section 4.17.  The pass is bound by the sigmoid and the fixed-point conversion,
// not by the bins, so there is one path.)
// row_col is a copy of radial.hip's: moved into map_plane.h it would have to leave radial.hip's code unchanged, which was not checked.
// The streaming loop is likelihood.hip's: 16-byte loads, eight in flight per thread, and an element-by-element path for a plane off a
// 16-byte boundary.  The public C ABI is include/ynet_hip.h.
#include "map_plane.h"
#include "map_fixed.h"
#include "../../include/ynet_hip.h"

namespace {

constexpr int MAX_SIDE = YNET_MAP_MARGINALS_MAX_SIDE;
constexpr int FRAC = YNET_MAP_MARGINALS_FRAC_BITS;
constexpr int GT_MARGIN = YNET_MAP_MARGINALS_GT_MARGIN;
static_assert(YNET_MAP_MARGINALS_MAX_PIXELS <= (1ll << (63 - (FRAC + 1))), "pixels x 2^41 stays below 2^63");
static_assert(YNET_MAP_MARGINALS_MAX_PIXELS <= (1 << 22), "row_col's float quotient is within one of the true one below 2^22 pixels");
static_assert(2 * MAX_SIDE * 8 <= 32768, "the two bin arrays take at most 32 KB of LDS: five workgroups per CU");
static_assert(MAX_SIDE <= 8 * 256, "the scan gives a thread at most eight bins");

struct MarginalArgs {
    const float* x;
    long long bs;
    const float* gt;        // [planes][2] (x, y); null when neither crps nor pit is asked for
    int C, H, W;
    float t, inv_t, rw;     // rw = 1 / W
    float* col;
    float* row;
    float* crps;
    float* pit;
    int* status;
};

// pixel index -> (row, col): radial.hip's, see there
__device__ __forceinline__ void row_col(int idx, int W, float rw, int& row, int& col) {
    const int q = (int)((float)idx * rw);
    const int r = idx - q * W;
    const int lo = r < 0 ? 1 : 0, hi = r >= W ? 1 : 0;
    row = q - lo + hi;
    col = r + (lo - hi) * W;
}

// One axis after pass 2: bins[side] -> the shares (share != null), in place the inclusive integer CDF, and this thread's part of the
// in-map CRPS terms against g (scored).  -> N, the total.  Thread t owns the bins [t * per, (t + 1) * per).  Ends on a barrier.
__device__ __forceinline__ u64 axis_scan(u64* bins, const int side, const bool scored, const int g, float* share, double& acc, u64* wtot,
                                         const int tid, const int lane, const int wave) {
    const int per = (side + 255) >> 8;
    const int lo = min(tid * per, side), hi = min(lo + per, side);
    u64 mine = 0;
    for (int t = lo; t < hi; ++t) mine += bins[t];
    u64 inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 up = __shfl_up(inc, o, 64);
        inc += lane >= o ? up : 0ull;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    const u64 w0 = wtot[0], w1 = wtot[1], w2 = wtot[2], w3 = wtot[3];
    const u64 base = (wave > 0 ? w0 : 0ull) + (wave > 1 ? w1 : 0ull) + (wave > 2 ? w2 : 0ull);
    const u64 N = (w0 + w1) + (w2 + w3);      // >= 2^40: the largest weight alone
    const double total = (double)N;
    u64 run = base + inc - mine;
    acc = 0.0;
    for (int t = lo; t < hi; ++t) {
        const u64 v = bins[t];
        if (share != nullptr) share[t] = (float)((double)v / total);
        run += v;
        bins[t] = run;
        if (scored) {
            const double F = (double)run / total, G = (double)(N - run) / total;
            acc += t < g ? F * F : G * G;
        }
    }
    __syncthreads();
    return N;
}

template <bool DIVIDE>
__global__ __launch_bounds__(256) void map_marginals_kernel(const MarginalArgs a) {
    extern __shared__ u64 bins[];       // [W] column bins, then [H] row bins: 8 (W + H) bytes
    __shared__ double ws[4][2];
    __shared__ u64 wtot[4];
    __shared__ float wmaxs[4];
    __shared__ int wpoison[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long plane = blockIdx.x;
    const int H = a.H, W = a.W, n = H * W;
    u64* const colb = bins;
    u64* const rowb = bins + W;
    const float* __restrict__ p = plane_ptr(a.x, a.bs, a.C, n, plane);
    const bool vec = (n & 3) == 0 && (((uintptr_t)p) & 15) == 0;

    // the ground truth: any pixel position within GT_MARGIN of the map (a NaN coordinate fails every compare)
    const bool has_gt = a.gt != nullptr;
    const float gxf = has_gt ? rintf(a.gt[2 * plane]) : 0.f, gyf = has_gt ? rintf(a.gt[2 * plane + 1]) : 0.f;
    const bool gt_ok = gxf >= (float)-GT_MARGIN && gxf <= (float)(W - 1 + GT_MARGIN) && gyf >= (float)-GT_MARGIN && gyf <= (float)(H - 1 + GT_MARGIN);
    const int gx = gt_ok ? (int)gxf : 0, gy = gt_ok ? (int)gyf : 0;
    const bool scored = has_gt && gt_ok;

    // pass 1: the largest logit, the NaN flag
    float xmax = -INFINITY;
    bool poison = false;
    if (vec) {
        const int n4 = n >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(p);
        int i = tid;
        for (; i + 7 * 256 < n4; i += 8 * 256) {     // eight independent 16-byte loads in flight per thread
            const float4 v0 = p4[i], v1 = p4[i + 256], v2 = p4[i + 512], v3 = p4[i + 768];
            const float4 v4 = p4[i + 1024], v5 = p4[i + 1280], v6 = p4[i + 1536], v7 = p4[i + 1792];
            __builtin_amdgcn_sched_barrier(0);      // (all eight issued before the first is consumed)
            const float4 vs[8] = {v0, v1, v2, v3, v4, v5, v6, v7};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                poison = poison | __builtin_isunordered(vs[j].x, vs[j].y) | __builtin_isunordered(vs[j].z, vs[j].w);
                xmax = __builtin_fmaxf(__builtin_fmaxf(xmax, __builtin_fmaxf(vs[j].x, vs[j].y)), __builtin_fmaxf(vs[j].z, vs[j].w));
            }
        }
        for (; i < n4; i += 256) {
            const float4 v = p4[i];
            poison = poison | __builtin_isunordered(v.x, v.y) | __builtin_isunordered(v.z, v.w);
            xmax = __builtin_fmaxf(__builtin_fmaxf(xmax, __builtin_fmaxf(v.x, v.y)), __builtin_fmaxf(v.z, v.w));
        }
    } else {        // a plane that does not start on a 16-byte boundary, or does not end on one
        for (int i = tid; i < n; i += 256) {
            const float v = p[i];
            poison = poison | (v != v);
            xmax = __builtin_fmaxf(xmax, v);        // (a NaN operand is dropped: the flag carries it)
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) xmax = __builtin_fmaxf(xmax, __shfl_xor(xmax, o, 64));
    const int any_poison = __any(poison);
    if (lane == 0) {
        wmaxs[wave] = xmax;
        wpoison[wave] = any_poison;
    }
    for (int i = tid; i < W + H; i += 256) bins[i] = 0;
    __syncthreads();
    xmax = __builtin_fmaxf(__builtin_fmaxf(wmaxs[0], wmaxs[1]), __builtin_fmaxf(wmaxs[2], wmaxs[3]));
    const float wmax = weight<DIVIDE>(xmax, a.inv_t, a.t);
    const float nan = __builtin_nanf("");
    if (tid == 0 && has_gt && !gt_ok) atomicExch(a.status, 1);
    if (four_wave_poison(wpoison) || !(wmax > 0.f)) {      // a NaN logit or Z == 0   (uniform: every thread leaves)
        if (a.col != nullptr)
            for (int k = tid; k < W; k += 256) a.col[plane * W + k] = nan;
        if (a.row != nullptr)
            for (int k = tid; k < H; k += 256) a.row[plane * H + k] = nan;
        if (a.crps != nullptr && tid < 2) a.crps[plane * 2 + tid] = nan;
        if (a.pit != nullptr && tid < 4) a.pit[plane * 4 + tid] = nan;
        return;
    }
    const int k0 = fixed_scale(wmax, FRAC);

    // pass 2: the bins
    auto fold1 = [&](const float v, const int idx) {
        int row, col;
        row_col(idx, W, a.rw, row, col);
        const u64 f = fixed(weight<DIVIDE>(v, a.inv_t, a.t), k0);
        atomicAdd(&colb[col], f);
        atomicAdd(&rowb[row], f);
    };
    auto fold = [&](const float4 v, const int i4) {
        int row, col;
        row_col(4 * i4, W, a.rw, row, col);
        // the three pixels after it: a 16-byte vector may run over the end of a row (W % 4 != 0), and of several (W < 4)
        int r1 = row, c1 = col + 1;
        r1 += c1 >= W ? 1 : 0;
        c1 = c1 >= W ? 0 : c1;
        int r2 = r1, c2 = c1 + 1;
        r2 += c2 >= W ? 1 : 0;
        c2 = c2 >= W ? 0 : c2;
        int r3 = r2, c3 = c2 + 1;
        r3 += c3 >= W ? 1 : 0;
        c3 = c3 >= W ? 0 : c3;
        const u64 f0 = fixed(weight<DIVIDE>(v.x, a.inv_t, a.t), k0), f1 = fixed(weight<DIVIDE>(v.y, a.inv_t, a.t), k0);
        const u64 f2 = fixed(weight<DIVIDE>(v.z, a.inv_t, a.t), k0), f3 = fixed(weight<DIVIDE>(v.w, a.inv_t, a.t), k0);
        atomicAdd(&colb[col], f0);
        atomicAdd(&colb[c1], f1);
        atomicAdd(&colb[c2], f2);
        atomicAdd(&colb[c3], f3);
        // one atomic per run of equal rows among the four: the running sum restarts where the row changes
        const bool e1 = r1 != row, e2 = r2 != r1, e3 = r3 != r2;
        const u64 s1 = e1 ? f1 : f0 + f1;
        const u64 s2 = e2 ? f2 : s1 + f2;
        const u64 s3 = e3 ? f3 : s2 + f3;
        if (e1) atomicAdd(&rowb[row], f0);
        if (e2) atomicAdd(&rowb[r1], s1);
        if (e3) atomicAdd(&rowb[r2], s2);
        atomicAdd(&rowb[r3], s3);
    };
    if (vec) {
        const int n4 = n >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(p);
        int i = tid;
        for (; i + 7 * 256 < n4; i += 8 * 256) {     // eight independent 16-byte loads in flight per thread
            const float4 v0 = p4[i], v1 = p4[i + 256], v2 = p4[i + 512], v3 = p4[i + 768];
            const float4 v4 = p4[i + 1024], v5 = p4[i + 1280], v6 = p4[i + 1536], v7 = p4[i + 1792];
            __builtin_amdgcn_sched_barrier(0);      // (all eight issued before the first is consumed)
            fold(v0, i);
            fold(v1, i + 256);
            fold(v2, i + 512);
            fold(v3, i + 768);
            fold(v4, i + 1024);
            fold(v5, i + 1280);
            fold(v6, i + 1536);
            fold(v7, i + 1792);
        }
        for (; i < n4; i += 256) fold(p4[i], i);
    } else {
        for (int i = tid; i < n; i += 256) fold1(p[i], i);
    }
    __syncthreads();

    // the bins -> shares, the integer CDF in place, the in-map CRPS terms
    double ax, ay;
    const u64 N = axis_scan(colb, W, scored, gx, a.col != nullptr ? a.col + plane * W : nullptr, ax, wtot, tid, lane, wave);
    (void)axis_scan(rowb, H, scored, gy, a.row != nullptr ? a.row + plane * H : nullptr, ay, wtot, tid, lane, wave);
    if (!has_gt) return;
    if (!gt_ok) {
        if (a.crps != nullptr && tid < 2) a.crps[plane * 2 + tid] = nan;
        if (a.pit != nullptr && tid < 4) a.pit[plane * 4 + tid] = nan;
        return;
    }
    ax = wave_sum(ax);
    ay = wave_sum(ay);
    if (lane == 0) {
        ws[wave][0] = ax;
        ws[wave][1] = ay;
    }
    __syncthreads();
    if (tid < 2) {      // thread 0: x, thread 1: y
        const int side = tid == 0 ? W : H, g = tid == 0 ? gx : gy;
        const u64* cum = tid == 0 ? colb : rowb;
        if (a.crps != nullptr) {
            // outside the map F is 0 (below) or 1 (from the last bin on): a ground truth k pixels outside adds k terms of 1
            const int k = g < 0 ? -g : (g >= side ? g - (side - 1) - 1 : 0);
            a.crps[plane * 2 + tid] = (float)(four_wave_sum(&ws[0][tid], 2) + (double)k);
        }
        if (a.pit != nullptr) {
            const double total = (double)N;
            const int gl = g - 1;
            const double lower = gl < 0 ? 0.0 : (gl >= side - 1 ? 1.0 : (double)cum[gl] / total);
            const double upper = g < 0 ? 0.0 : (g >= side - 1 ? 1.0 : (double)cum[g] / total);
            a.pit[plane * 4 + 2 * tid] = (float)lower;
            a.pit[plane * 4 + 2 * tid + 1] = (float)upper;
        }
    }
}

}  // namespace

extern "C" int ynet_map_marginals(const float* x, long long batch_stride, const float* gt_xy, long long B, int C, int H, int W,
                                  float temperature, float* col, float* row, float* crps, float* pit, int* status, void* stream) {
    YNET_REQUIRE(x != nullptr, "map_marginals: null map");
    YNET_REQUIRE(col != nullptr || row != nullptr || crps != nullptr || pit != nullptr, "map_marginals: no output asked for");
    const bool scores = crps != nullptr || pit != nullptr;
    YNET_REQUIRE(!scores || gt_xy != nullptr, "map_marginals: crps and pit need the ground truth (gt_xy)");
    YNET_REQUIRE(!scores || status != nullptr, "map_marginals: null status flag");
    if (map_check_temperature("map_marginals", temperature) || map_check_shape("map_marginals", B, C, H, W)) return 1;
    YNET_REQUIRE(H <= YNET_MAP_MARGINALS_MAX_SIDE && W <= YNET_MAP_MARGINALS_MAX_SIDE, "map_marginals: a plane of %dx%d has a side above %d",
                 H, W, YNET_MAP_MARGINALS_MAX_SIDE);
    YNET_REQUIRE((long long)H * W <= YNET_MAP_MARGINALS_MAX_PIXELS,
                 "map_marginals: a plane of %dx%d has more than the %d pixels the integer sums hold", H, W, YNET_MAP_MARGINALS_MAX_PIXELS);
    if (map_check_batch_stride("map_marginals", batch_stride, C, H, W)) return 1;
    const long long planes = B * C;
    YNET_REQUIRE(B < (1ll << 31) && planes < (1ll << 31), "map_marginals: too many planes");
    MarginalArgs a;
    a.x = x;
    a.bs = batch_stride;
    a.gt = scores ? gt_xy : nullptr;      // (col and row do not need it: with or without, the same bits)
    a.C = C;
    a.H = H;
    a.W = W;
    a.t = temperature;
    a.inv_t = 1.f / temperature;
    a.rw = 1.f / (float)W;
    a.col = col;
    a.row = row;
    a.crps = crps;
    a.pit = pit;
    a.status = status;
    const size_t lds = sizeof(u64) * (size_t)(H + W);
    if (temperature == 1.f) hipLaunchKernelGGL(map_marginals_kernel<false>, dim3((unsigned)planes), dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(map_marginals_kernel<true>, dim3((unsigned)planes), dim3(256), lds, (hipStream_t)stream, a);
    return ynet_check_launch("map_marginals");
}
