// Deterministic goal modes of the goal map: greedy non-maximum suppression per plane (no counterpart in the reference, whose one
// deterministic goal is the soft-argmax -- the mean of a multi-modal map).  Mode m is the not-yet-suppressed pixel with the largest
// raw fp32 logit (ties: the smallest linear index); it suppresses the disk (drow^2 + dcol^2 <= radius^2) around it and claims the
// probability mass sigmoid(x / T) / Z of the pixels it newly suppressed.  The contract, rule by rule, is in include/ynet_hip.h.
//
// One workgroup of 16 wavefronts per plane, and the plane is read from HBM once:
//   pass 1   every wave takes segments of 256 consecutive pixels; per segment the best (key, index) goes into an LDS table, and on the
//            way Z (fp64) and the NaN flag are formed
//   round m  argmax over the segment table (<= 1024 entries, one per thread) -> the mode; the threads walk the disk's bounding box and
//            set the pixel's bit in an LDS bitmap of H * W bits with atomicOr as test-and-set: the old bit says whether the pixel is
//            newly suppressed, i.e. whether it adds to the mode's mass; then only the segments the disk touched are scanned again
//            (from L2) with the bitmap applied.
// A round costs O(segments + disk area + touched segments), not a pass over the plane.
// Order: a logit is compared through `key`, a monotone map of its bits to a signed integer with -0.0 folded onto +0.0 -- integer
// compares know nothing of denormal flushing -- and (key, index) travel as ONE 64-bit number whose maximum is the winner: the larger
// key, and among equal keys the smaller index, whichever thread, wave or segment saw it.
// Sums are fp64; every pixel belongs to a fixed thread, and the partial sums are combined in a fixed tree: two runs give the same bits.
#include "map_plane.h"
#include "../../include/ynet_hip.h"
#include <limits.h>

namespace {

constexpr int THREADS = 1024, WAVES = THREADS / 64;
constexpr int SEG = 256;                             // pixels per segment: four per lane
constexpr int MAX_PIXELS = YNET_MAP_MODES_MAX_PIXELS;  // 512 x 512
constexpr int MAX_SEGS = MAX_PIXELS / SEG;           // 1024 == THREADS: the round's argmax reads one entry per thread
constexpr int MAX_MODES = 64;
constexpr int MAX_PLANES = (1 << 22) - 1;             // grid x block stays below 2^32 threads
static_assert((MAX_PIXELS & (MAX_PIXELS - 1)) == 0 && MAX_SEGS == THREADS, "one table entry per thread");

constexpr long long NO_CANDIDATE = LLONG_MIN;        // below every (key, index) of a candidate

// The order of the logits as an order of signed integers: `key`, the bits of x mapped monotonically, -0.0 folded onto +0.0 (a tie).
// (key, index) travel as one 64-bit number, key in the upper half; the lower half holds MAX_PIXELS - 1 - index, so that among equal
// keys the smaller index is the larger number, and below it one bit that remembers a -0.0: indices are unique, so the bit never
// decides an order, and the logit can be handed back exactly as it was stored without reading it again.
// A NaN never gets here as a winner (its plane is not ranked).
static_assert(MAX_PIXELS <= (1 << 18), "the index and the sign bit share the lower half");
constexpr int KEY_NINF = INT_MIN + 0x7fffff;        // the key of -inf

__device__ __forceinline__ long long ranked(float x, int index) {
    const int b = __float_as_int(x);
    const int k = b >= 0 ? b : (b == INT_MIN ? 0 : (b ^ 0x7fffffff));      // (INT_MIN is -0.0)
    if (k <= KEY_NINF) return NO_CANDIDATE;          // x == -inf: not a candidate
    return ((long long)k << 32) | (long long)(unsigned)(((MAX_PIXELS - 1 - index) << 1) | (b == INT_MIN ? 1 : 0));
}

__device__ __forceinline__ int index_of(long long r) { return MAX_PIXELS - 1 - (int)(((unsigned)r >> 1) & (unsigned)(MAX_PIXELS - 1)); }

__device__ __forceinline__ float logit_of(long long r) {
    const int k = (int)(r >> 32);
    return __int_as_float(k > 0 ? k : (k == 0 ? ((r & 1) ? INT_MIN : 0) : (k ^ 0x7fffffff)));
}

__device__ __forceinline__ long long llmax(long long a, long long b) { return a > b ? a : b; }

// Wave-wide reductions on the DPP path: a rotation inside each row of 16 lanes (row_ror 8, 4, 2, 1) leaves the row's result in every
// lane of the row, v_readlane fetches the four rows' results, and three more operations combine them -- a fixed tree, the same result
// in every lane.  (__shfl_xor compiles to ds_bpermute: twelve dependent LDS round trips per 64-bit reduction, which was most of a
// round's time.)
template <int CTRL>
__device__ __forceinline__ long long dpp64(long long v) {
    const int lo = (int)(unsigned)(v & 0xffffffffll), hi = (int)(v >> 32);
    const int rlo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false), rhi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
    return ((long long)rhi << 32) | (long long)(unsigned)rlo;
}

__device__ __forceinline__ long long lane64(long long v, int l) {
    const int lo = __builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffll), l), hi = __builtin_amdgcn_readlane((int)(v >> 32), l);
    return ((long long)hi << 32) | (long long)(unsigned)lo;
}

constexpr int ROW_ROR = 0x120;      // dpp_ctrl of row_ror:n is 0x120 + n

__device__ __forceinline__ long long wave_max(long long v) {
    v = llmax(v, dpp64<ROW_ROR + 8>(v));
    v = llmax(v, dpp64<ROW_ROR + 4>(v));
    v = llmax(v, dpp64<ROW_ROR + 2>(v));
    v = llmax(v, dpp64<ROW_ROR + 1>(v));
    return llmax(llmax(lane64(v, 0), lane64(v, 16)), llmax(lane64(v, 32), lane64(v, 48)));
}

// (not map_plane.h's wave_sum: another tree, so other bits)
__device__ __forceinline__ double wave_sum_dpp(double v) {
    v += __longlong_as_double(dpp64<ROW_ROR + 8>(__double_as_longlong(v)));
    v += __longlong_as_double(dpp64<ROW_ROR + 4>(__double_as_longlong(v)));
    v += __longlong_as_double(dpp64<ROW_ROR + 2>(__double_as_longlong(v)));
    v += __longlong_as_double(dpp64<ROW_ROR + 1>(__double_as_longlong(v)));
    const long long b = __double_as_longlong(v);      // (lanes 0, 16, 32, 48: one fixed order per row, whatever the other lanes hold)
    return (__longlong_as_double(lane64(b, 0)) + __longlong_as_double(lane64(b, 16)))
         + (__longlong_as_double(lane64(b, 32)) + __longlong_as_double(lane64(b, 48)));
}

// sigmoid(x / T) in fp32, formed as map_likelihood_kernel (likelihood.hip) forms its weight: the quotient as the product with 1 / T
// corrected by its exact residual, e = exp(-|z|) from v_exp_f32 corrected to first order, w = 1 / (1 + e) or e / (1 + e).
// -inf gives exactly 0, +inf exactly 1; a NaN never adds to a mass (its plane is not ranked).
// (Not sigmoid_term.h's weight<DIVIDE>, which map_plane.h brings in beside it: this one switches on T at run time, the same bits through
// another instruction stream.  A call without a template argument is this overload.)
__device__ __forceinline__ float weight(float x, float inv_t, float t) {
    float z = x;
    if (t != 1.f) {
        z = x * inv_t;
        const float zc = __builtin_fmaf(__builtin_fmaf(-z, t, x), inv_t, z);
        z = (zc == zc) ? zc : z;
    }
    const float L2E = 1.44269502162933349609375f, L2El = 1.925963033500011e-8f;      // log2(e) = L2E + L2El
    const float ac = __builtin_fminf(__builtin_fabsf(z), 104.f);
    const float p = -ac * L2E;
    const float r = __builtin_fmaf(-ac, L2E, -p) - ac * L2El;
    float e = __builtin_amdgcn_exp2f(p);
    e = __builtin_fmaf(e, r * 0.693147182464599609375f, e);
    const float ru = __builtin_amdgcn_rcpf(1.f + e);
    return (z >= 0.f) ? ru : e * ru;
}

struct ModesArgs {
    const float* x;
    long long bs;
    int C, H, W, M, radius;
    float t, inv_t;
    float* xy;
    float* logit;
    float* mass;
    int* count;
    int* status;
};

template <bool MASS>
__global__ __launch_bounds__(THREADS) void map_modes_kernel(const ModesArgs a) {
    __shared__ unsigned bitmap[MAX_PIXELS / 32];      // 32 KB: bit i = pixel i is suppressed
    __shared__ long long seg_best[MAX_SEGS];          //  8 KB: the best (key, index) among the unsuppressed candidates of every segment
    __shared__ long long wbest[WAVES];
    __shared__ double wsum[WAVES];
    __shared__ int wnan[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long plane = blockIdx.x;
    const int H = a.H, W = a.W, M = a.M;
    const int n = H * W, nseg = (n + SEG - 1) / SEG;
    const float* __restrict__ p = plane_ptr(a.x, a.bs, a.C, n, plane);
    float* xy = a.xy + plane * M * 2;
    float* logit = a.logit + plane * M;
    float* mass = MASS ? a.mass + plane * M : nullptr;

    for (int i = tid; i < (n + 31) / 32; i += THREADS) bitmap[i] = 0u;

    // The four pixels of a lane in segment s, loaded without a branch (with one, hipcc sinks a load down to its use and the loads of
    // a group no longer fly together): the index is clamped into the plane, and what lies past the plane reads as -inf.
    const float ninf = -INFINITY;
    auto load_segment = [&](int s, float (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = s * SEG + j * 64 + lane;
            const float x = p[i < n ? i : n - 1];
            v[j] = i < n ? x : ninf;
        }
    };

    // ---- pass 1: the segment table, Z and the NaN flag.  Four segments (sixteen loads per lane) are in flight per wave.
    double sw = 0.0;
    bool poison = false;
    for (int s = wave; s < nseg; s += 4 * WAVES) {
        float v[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) load_segment(s + k * WAVES, v[k]);      // (a segment past the table lies past the plane)
        __builtin_amdgcn_sched_barrier(0);            // (all sixteen issued before the first is consumed)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int sk = s + k * WAVES;
            long long b = NO_CANDIDATE;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                poison = poison | (v[k][j] != v[k][j]);
                b = llmax(b, ranked(v[k][j], sk * SEG + j * 64 + lane));
                if (MASS) sw += (double)weight(v[k][j], a.inv_t, a.t);
            }
            b = wave_max(b);
            if (lane == 0 && sk < nseg) seg_best[sk] = b;
        }
    }
    if (MASS) sw = wave_sum_dpp(sw);
    const int any_poison = __any(poison);
    if (lane == 0) {
        wsum[wave] = sw;
        wnan[wave] = any_poison;
    }
    __syncthreads();
    int bad = 0;
    double Z = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        bad |= wnan[w];
        Z += wsum[w];
    }
    __syncthreads();                                  // (wsum is written again in the rounds)

    int count = 0;
    if (bad) {
        count = -1;                                   // a NaN anywhere: nothing is ranked in this plane
        if (tid == 0) atomicOr(a.status, 1);
    } else {
        // the disk never reaches further than the map: beyond H + W every pixel is inside, and the squares below stay exact
        const long long R = a.radius < H + W ? a.radius : H + W, R2 = R * R;
        for (int m = 0; m < M; ++m) {
            // ---- the mode: argmax over the segment table
            long long b = wave_max(tid < nseg ? seg_best[tid] : NO_CANDIDATE);
            if (lane == 0) wbest[wave] = b;
            __syncthreads();
            b = wbest[0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) b = llmax(b, wbest[w]);
            if (b == NO_CANDIDATE) break;             // (the same value in every thread)
            count = m + 1;
            const int idx = index_of(b), row = idx / W, col = idx - row * W;
            if (tid == 0) {
                xy[2 * m] = (float)col;
                xy[2 * m + 1] = (float)row;
                logit[m] = logit_of(b);
            }
            // ---- suppression: the bounding box of the disk, clipped to the map
            const int r0 = (int)(row - R > 0 ? row - R : 0), r1 = (int)(row + R < H - 1 ? row + R : H - 1);
            const int c0 = (int)(col - R > 0 ? col - R : 0), c1 = (int)(col + R < W - 1 ? col + R : W - 1);
            const int bw = c1 - c0 + 1, box = bw * (r1 - r0 + 1);
            // the segments the box touches are scanned again below: [s_lo, s_hi], less those between two row spans of the box
            const int s_lo = (r0 * W + c0) / SEG, s_hi = (r1 * W + c1) / SEG;
            auto touched = [&](int s) {      // pixels [lo, hi] of s meet a row span [rr * W + c0, rr * W + c1] for some rr in [r0, r1]?
                const int lo = s * SEG, hi = lo + SEG - 1;
                const int first = lo - c1 > 0 ? (lo - c1 + W - 1) / W : 0, last = hi - c0 >= 0 ? (hi - c0) / W : -1;
                return s <= s_hi && (first > r0 ? first : r0) <= (last < r1 ? last : r1);
            };
            // Every global load of the round is issued here, before anything waits: the wave's first two segments of the re-scan
            // (their values do not depend on the bitmap, only their use does), then the disk's pixels.  A round then pays one trip
            // to L2, not three.
            const int sa = s_lo + wave, sb = sa + WAVES;
            const bool scan_a = touched(sa), scan_b = touched(sb);      // (the same in every lane of the wave)
            float va[4], vb[4];
            load_segment(scan_a ? sa : s_lo, va);
            load_segment(scan_b ? sb : s_lo, vb);
            double acc = 0.0;
            for (int i = tid; i < box; i += THREADS) {
                const int rr = r0 + i / bw, cc = c0 + i % bw, pix = rr * W + cc;
                const long long dr = rr - row, dc = cc - col;
                const float x = MASS ? p[pix] : 0.f;
                if (dr * dr + dc * dc <= R2) {
                    const unsigned bit = 1u << (pix & 31);
                    const unsigned old = atomicOr(&bitmap[pix >> 5], bit);      // test-and-set: the old bit says whether the pixel is new
                    if (MASS && (old & bit) == 0u) acc += (double)weight(x, a.inv_t, a.t);
                }
            }
            if (MASS) {
                acc = wave_sum_dpp(acc);
                if (lane == 0) wsum[wave] = acc;
            }
            __syncthreads();                          // the bitmap is complete (and wbest read by everyone)
            if (MASS && tid == 0) {
                double s = 0.0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) s += wsum[w];
                mass[m] = (float)(s / Z);
            }
            // ---- the touched segments, scanned again with the bitmap applied
            auto rescan = [&](int s, const float (&v)[4]) {
                long long best = NO_CANDIDATE;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = s * SEG + j * 64 + lane;
                    if (i < n && ((bitmap[i >> 5] >> (i & 31)) & 1u) == 0u) best = llmax(best, ranked(v[j], i));
                }
                best = wave_max(best);
                if (lane == 0) seg_best[s] = best;
            };
            if (scan_a) rescan(sa, va);
            if (scan_b) rescan(sb, vb);
            for (int s = sb + WAVES; s <= s_hi; s += WAVES) {      // (a box of more than 32 segments: a large radius, or a wide map)
                if (!touched(s)) continue;
                load_segment(s, va);
                rescan(s, va);
            }
            __syncthreads();                          // the table is complete (and wsum read)
        }
    }
    // ---- what no mode filled
    if (tid == 0) a.count[plane] = count;
    for (int m = (count < 0 ? 0 : count) + tid; m < M; m += THREADS) {
        xy[2 * m] = -1.f;
        xy[2 * m + 1] = -1.f;
        logit[m] = ninf;
        if (MASS) mass[m] = 0.f;
    }
}

}  // namespace

extern "C" int ynet_map_modes(const float* x, long long batch_stride, long long B, int C, int H, int W, int n_modes, int radius,
                              float temperature, float* xy, float* logit, float* mass, int* count, int* status, void* stream) {
    YNET_REQUIRE(x != nullptr && xy != nullptr && logit != nullptr && count != nullptr && status != nullptr,
                 "map_modes: null map, xy, logit, count or status");
    YNET_REQUIRE(n_modes >= 1 && n_modes <= MAX_MODES, "map_modes: n_modes = %d, expected 1 .. %d", n_modes, MAX_MODES);
    YNET_REQUIRE(radius >= 0, "map_modes: radius = %d is negative", radius);
    if (map_check_shape("map_modes", B, C, H, W)) return 1;
    YNET_REQUIRE((long long)H * W <= MAX_PIXELS, "map_modes: a plane of %dx%d is beyond the cap of %d pixels (the LDS suppression bitmap)",
                 H, W, MAX_PIXELS);
    if (map_check_batch_stride("map_modes", batch_stride, C, H, W)) return 1;
    YNET_REQUIRE(mass == nullptr || (temperature > 0.f && temperature <= 3.0e38f && 1.f / temperature <= 3.0e38f),
                 "map_modes: with mass, the temperature and its reciprocal must be positive and finite");
    YNET_REQUIRE(B <= MAX_PLANES / C, "map_modes: more than %d planes", MAX_PLANES);
    const long long planes = B * C;
    ModesArgs a;
    a.x = x;
    a.bs = batch_stride;
    a.C = C;
    a.H = H;
    a.W = W;
    a.M = n_modes;
    a.radius = radius;
    a.t = mass != nullptr ? temperature : 1.f;
    a.inv_t = mass != nullptr ? 1.f / temperature : 1.f;
    a.xy = xy;
    a.logit = logit;
    a.mass = mass;
    a.count = count;
    a.status = status;
    if (mass != nullptr) hipLaunchKernelGGL(map_modes_kernel<true>, dim3((unsigned)planes), dim3(THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(map_modes_kernel<false>, dim3((unsigned)planes), dim3(THREADS), 0, (hipStream_t)stream, a);
    return ynet_check_launch("map_modes");
}
