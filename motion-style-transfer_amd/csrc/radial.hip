// Radial scores of the goal map: the mass profile of the distribution sigmoid(pred_goal_map / T) (utils/evaluate.py:128-131 builds it,
// utils/image_utils.py:110-135 draws from it) around the ground-truth pixel -- what the reference's best-of-K FDE (utils/evaluate.py:268-291)
// estimates from one seeded draw, here as a function of the map alone.  Per plane (agent b, step c), with z = x / T, w = sigmoid(z),
// Z = sum w, g = the rounded ground truth (NOT required to lie inside the map) and d2_i = (col - g.x)^2 + (row - g.y)^2:
//   ring[k] = (sum over {floor(sqrt(d2)) == k} of w) / Z, k < n_rings      tail = (sum over {floor(sqrt(d2)) >= n_rings} of w) / Z
//   mean    = (sum w sqrt(d2)) / Z                                          mean_sq = (sum w d2) / Z
// Ring membership is decided in integers: the float sqrt is a first guess, corrected so that k^2 <= d2 < (k + 1)^2.
//
// One workgroup per plane, two passes, the second one served by the caches:
//   pass 1   the largest logit and the NaN flag (no sigmoid: w is monotone in x, so the largest w is the one of the largest logit)
//   pass 2   per pixel w, its ring and its fixed-point mass (map_fixed.h: w * 2^(40 - e), e = floor(log2 of the plane's largest w),
//            truncated), added to the ring's 64-bit integer bin in LDS with an atomic; sum w, sum w sqrt(d2) and sum w d2 in fp64 registers
// then the bins are divided by their own integer total.  Integer adds are order-free, the fp64 sums are per thread and combined in the
// fixed tree of map_plane.h: two runs give the same bits, and there is no floating-point atomic.
// LDS conflicts: the pixels of a row mostly share a ring, so a thread adds the four adjacent pixels of its 16-byte load as one atomic
// per run of equal rings.  (Several histograms picked by lane, the form credible.hip uses for its early passes, measured no faster
// here -- 1, 2 and 4 copies within 1 % of each other, DESIGN.md section 4.16 -- so there is one.)
// The streaming loop is likelihood.hip's: 16-byte loads, eight in flight per thread, no data-dependent branch around the loads, and an
// element-by-element path for a plane off a 16-byte boundary.  The public C ABI is include/ynet_hip.h.
#include "map_plane.h"
#include "map_fixed.h"
#include "../../include/ynet_hip.h"

namespace {

constexpr int MAXR = YNET_MAP_RADIAL_MAX_RINGS;
constexpr int FRAC = YNET_MAP_RADIAL_FRAC_BITS;
constexpr int GT_MARGIN = YNET_MAP_RADIAL_GT_MARGIN;
static_assert(YNET_MAP_RADIAL_MAX_PIXELS <= (1ll << (63 - (FRAC + 1))), "pixels x 2^41 stays below 2^63");
static_assert(YNET_MAP_RADIAL_MAX_PIXELS <= (1 << 22), "row_col's float quotient is within one of the true one below 2^22 pixels");
static_assert(2ll * (GT_MARGIN + 16383) * (GT_MARGIN + 16383) < (1ll << 31), "d2 fits 32 bits");

struct RadialArgs {
    const float* x;
    long long bs;
    const float* gt;        // [planes][2] (x, y)
    int C, H, W, R;
    float t, inv_t, rw;     // rw = 1 / W
    float* ring;
    float* tail;
    float* mean;
    float* mean_sq;
    int* status;
};

// pixel index -> (row, col): the float quotient is off by at most one below 2^22 pixels ((float)idx is exact, the product carries two
// roundings of 2^-24 on a quotient below 2^22), one step either way settles it
__device__ __forceinline__ void row_col(int idx, int W, float rw, int& row, int& col) {
    const int q = (int)((float)idx * rw);
    const int r = idx - q * W;
    const int lo = r < 0 ? 1 : 0, hi = r >= W ? 1 : 0;
    row = q - lo + hi;
    col = r + (lo - hi) * W;
}

// floor(sqrt(d2)) in integers, d2 < 2^31: v_sqrt_f32 on the rounded d2 is within 0.01 of the root, so the guess is off by at most one
__device__ __forceinline__ unsigned ring_of(unsigned d2) {
    unsigned k = (unsigned)__builtin_amdgcn_sqrtf((float)d2);
    k -= (k * k > d2) ? 1u : 0u;
    k += ((k + 1u) * (k + 1u) <= d2) ? 1u : 0u;      // ((k + 1)^2 <= 46342^2 < 2^32)
    return k;
}

template <bool DIVIDE>
__global__ __launch_bounds__(256) void map_radial_kernel(const RadialArgs a) {
    __shared__ u64 hist[MAXR + 1];      // 8.2 KB; bin R is the tail
    __shared__ double ws[4][3];
    __shared__ u64 wtot[4];
    __shared__ float wmaxs[4];
    __shared__ int wpoison[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long plane = blockIdx.x;
    const int H = a.H, W = a.W, R = a.R, n = H * W;
    const float* __restrict__ p = plane_ptr(a.x, a.bs, a.C, n, plane);
    const bool vec = (n & 3) == 0 && (((uintptr_t)p) & 15) == 0;

    // the ground truth: any pixel position within GT_MARGIN of the map (a NaN coordinate fails every compare)
    const float gxf = rintf(a.gt[2 * plane]), gyf = rintf(a.gt[2 * plane + 1]);
    const bool gt_ok = gxf >= (float)-GT_MARGIN && gxf <= (float)(W - 1 + GT_MARGIN) && gyf >= (float)-GT_MARGIN && gyf <= (float)(H - 1 + GT_MARGIN);
    const int gx = gt_ok ? (int)gxf : 0, gy = gt_ok ? (int)gyf : 0;

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
    for (int i = tid; i <= R; i += 256) hist[i] = 0;
    __syncthreads();
    xmax = __builtin_fmaxf(__builtin_fmaxf(wmaxs[0], wmaxs[1]), __builtin_fmaxf(wmaxs[2], wmaxs[3]));
    const float wmax = weight<DIVIDE>(xmax, a.inv_t, a.t);
    if (four_wave_poison(wpoison) || !(wmax > 0.f) || !gt_ok) {      // a NaN logit, Z == 0 or no usable ground truth   (uniform: every thread leaves)
        const float nan = __builtin_nanf("");
        if (a.ring != nullptr)
            for (int k = tid; k < R; k += 256) a.ring[plane * R + k] = nan;
        if (tid == 0) {
            if (a.tail != nullptr) a.tail[plane] = nan;
            if (a.mean != nullptr) a.mean[plane] = nan;
            if (a.mean_sq != nullptr) a.mean_sq[plane] = nan;
            if (!gt_ok) atomicExch(a.status, 1);
        }
        return;
    }
    const int k0 = fixed_scale(wmax, FRAC);

    // pass 2: running sums in fp64 -- sum w, sum w * sqrt(d2), sum w * d2 (the products formed inside the fma: never rounded on their own)
    double sw = 0.0, sm = 0.0, sq = 0.0;
    struct Pixel {
        float w;
        unsigned k;     // its bin: min(ring, R)
        u64 f;
    };
    auto pixel = [&](const float v, const int row, const int col, double& m, double& q) {
        Pixel o;
        o.w = weight<DIVIDE>(v, a.inv_t, a.t);
        const int dx = col - gx, dy = row - gy;
        const unsigned d2 = (unsigned)(dx * dx) + (unsigned)(dy * dy);
        const unsigned k = ring_of(d2);
        o.k = k < (unsigned)R ? k : (unsigned)R;
        o.f = fixed(o.w, k0);
        m = __builtin_fma((double)o.w, (double)sqrtf((float)d2), m);
        q = __builtin_fma((double)o.w, (double)d2, q);
        return o;
    };
    auto fold1 = [&](const float v, const int idx) {
        int row, col;
        row_col(idx, W, a.rw, row, col);
        const Pixel t = pixel(v, row, col, sm, sq);
        sw += (double)t.w;
        atomicAdd(&hist[t.k], t.f);
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
        const Pixel t0 = pixel(v.x, row, col, sm, sq), t1 = pixel(v.y, r1, c1, sm, sq);
        const Pixel t2 = pixel(v.z, r2, c2, sm, sq), t3 = pixel(v.w, r3, c3, sm, sq);
        sw += (double)((t0.w + t1.w) + (t2.w + t3.w));
        // one atomic per run of equal bins among the four: the running sum restarts where the bin changes
        const bool e1 = t1.k != t0.k, e2 = t2.k != t1.k, e3 = t3.k != t2.k;
        const u64 s1 = e1 ? t1.f : t0.f + t1.f;
        const u64 s2 = e2 ? t2.f : s1 + t2.f;
        const u64 s3 = e3 ? t3.f : s2 + t3.f;
        if (e1) atomicAdd(&hist[t0.k], t0.f);
        if (e2) atomicAdd(&hist[t1.k], s1);
        if (e3) atomicAdd(&hist[t2.k], s2);
        atomicAdd(&hist[t3.k], s3);
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
    sw = wave_sum(sw);
    sm = wave_sum(sm);
    sq = wave_sum(sq);
    if (lane == 0) {
        ws[wave][0] = sw;
        ws[wave][1] = sm;
        ws[wave][2] = sq;
    }
    __syncthreads();

    // the bins: their total, then the shares
    u64 mine = 0;
    for (int k = tid; k <= R; k += 256) mine += hist[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0) wtot[wave] = mine;
    __syncthreads();
    const double total = (double)((wtot[0] + wtot[1]) + (wtot[2] + wtot[3]));      // >= 2^40: the largest weight alone
    for (int k = tid; k <= R; k += 256) {
        const float share = (float)((double)hist[k] / total);
        if (k < R) {
            if (a.ring != nullptr) a.ring[plane * R + k] = share;
        } else if (a.tail != nullptr) {
            a.tail[plane] = share;
        }
    }
    if (tid == 0) {
        const double Z = four_wave_sum(&ws[0][0], 3);
        if (a.mean != nullptr) a.mean[plane] = (float)(four_wave_sum(&ws[0][1], 3) / Z);
        if (a.mean_sq != nullptr) a.mean_sq[plane] = (float)(four_wave_sum(&ws[0][2], 3) / Z);
    }
}

}  // namespace

extern "C" int ynet_map_radial(const float* x, long long batch_stride, const float* gt_xy, long long B, int C, int H, int W,
                               float temperature, int n_rings, float* ring, float* tail, float* mean, float* mean_sq, int* status,
                               void* stream) {
    YNET_REQUIRE(x != nullptr, "map_radial: null map");
    YNET_REQUIRE(gt_xy != nullptr, "map_radial: null ground truth (gt_xy)");
    YNET_REQUIRE(ring != nullptr || tail != nullptr || mean != nullptr || mean_sq != nullptr, "map_radial: no output asked for");
    YNET_REQUIRE(status != nullptr, "map_radial: null status flag");
    YNET_REQUIRE(n_rings >= 1 && n_rings <= YNET_MAP_RADIAL_MAX_RINGS, "map_radial: n_rings = %d, expected 1 .. %d", n_rings,
                 YNET_MAP_RADIAL_MAX_RINGS);
    if (map_check_temperature("map_radial", temperature) || map_check_shape("map_radial", B, C, H, W)) return 1;
    YNET_REQUIRE(H <= YNET_MAP_RADIAL_MAX_SIDE && W <= YNET_MAP_RADIAL_MAX_SIDE, "map_radial: a plane of %dx%d has a side above %d", H, W,
                 YNET_MAP_RADIAL_MAX_SIDE);
    YNET_REQUIRE((long long)H * W <= YNET_MAP_RADIAL_MAX_PIXELS, "map_radial: a plane of %dx%d has more than the %d pixels the integer sums hold",
                 H, W, YNET_MAP_RADIAL_MAX_PIXELS);
    if (map_check_batch_stride("map_radial", batch_stride, C, H, W)) return 1;
    const long long planes = B * C;
    YNET_REQUIRE(B < (1ll << 31) && planes < (1ll << 31), "map_radial: too many planes");
    RadialArgs a;
    a.x = x;
    a.bs = batch_stride;
    a.gt = gt_xy;
    a.C = C;
    a.H = H;
    a.W = W;
    a.R = n_rings;
    a.t = temperature;
    a.inv_t = 1.f / temperature;
    a.rw = 1.f / (float)W;
    a.ring = ring;
    a.tail = tail;
    a.mean = mean;
    a.mean_sq = mean_sq;
    a.status = status;
    if (temperature == 1.f) hipLaunchKernelGGL(map_radial_kernel<false>, dim3((unsigned)planes), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(map_radial_kernel<true>, dim3((unsigned)planes), dim3(256), 0, (hipStream_t)stream, a);
    return ynet_check_launch("map_radial");
}
