// Credible regions of the goal map: how SHARP the distribution sigmoid(pred_goal_map / T) is, where ynet_map_likelihood's hpd says how
// well calibrated (no counterpart in the reference, which only draws the maps).  Per plane (agent b, step c) and level q, with
// z = x / T, w = sigmoid(z), Z = sum w:
//   threshold = the largest logit value t present in the plane with  sum over {x >= t} of w  >=  q * Z
//   area      = #{x >= threshold},   mass = (sum over {x >= threshold} of w) / Z
// Membership is decided on the raw fp32 logits, as hpd decides it; the contract, rule by rule, is in include/ynet_hip.h.
//
// One workgroup of 16 wavefronts per plane, a MASS-WEIGHTED RADIX SELECT over the 32-bit order keys of the logits:
//   pass 0      the largest key and the NaN flag (no sigmoid: w is monotone in x, so the largest w is the one of the largest logit);
//               this is the plane's one trip to HBM, the later passes find it in the caches
//   pass 1..4   eight bits of the key per pass, from the top.  Every level carries the key prefix it has settled so far; a pixel whose
//               key starts with the prefix of some level adds its mass (and 1) to the bin of its next eight bits.  Then one wave per
//               level walks the 256 bins from the top, finds the bin in which the cumulative mass reaches q * Z, and appends it to
//               the level's prefix.  After four passes the prefix is the threshold's key and the last bin its plateau.
// Levels are nested, so their prefixes are ordered and levels with the same prefix share one histogram (a "group"); there are eight
// histogram slots, and while fewer groups than slots exist every group gets several copies, picked by lane, to spread the atomics
// of the early passes, in which few bins take nearly all pixels.
// Masses are 64-bit integers: w * 2^(40 - e), e = floor(log2 of the plane's largest w), truncated -- formed from w's own mantissa
// and exponent with shifts, so exact whatever the denormal mode.  Integer adds are order-free: LDS atomics give the same bits run
// after run, the sub-bins of a bin add up to it exactly, and the walk of pass k + 1 is certain to find its crossing inside the bin
// pass k chose.  The comparison against q * Z is fp64 (q: the fp32 level taken to fp64).
#include "map_plane.h"
#include "map_fixed.h"
#include "../../include/ynet_hip.h"
#include <limits.h>

namespace {

constexpr int THREADS = 1024, WAVES = THREADS / 64;
constexpr int MAXL = YNET_MAP_CREDIBLE_MAX_LEVELS;
constexpr int FRAC = YNET_MAP_CREDIBLE_FRAC_BITS;
constexpr int BINS = 256, DIGIT = 8, PASSES = 32 / DIGIT;
constexpr int SLOTS = 8;                              // histograms per pass: groups x copies
constexpr long long MAX_PLANES = (1 << 22) - 1;       // grid x block stays below 2^32 threads
static_assert(MAXL <= SLOTS && MAXL <= WAVES, "one histogram slot and one walking wave per level");
static_assert(YNET_MAP_CREDIBLE_MAX_PIXELS <= (1ll << (63 - (FRAC + 1))), "pixels x 2^41 stays below 2^63");

// The order of the logits as an order of unsigned integers: the monotone key of modes.hip (-0.0 folded onto +0.0; integer compares
// know nothing of denormal flushing), moved to unsigned so that its digits can be cut out.  -inf has key 0x007fffff.
__device__ __forceinline__ unsigned key_of(float x) {
    const int b = __float_as_int(x);
    const int k = b >= 0 ? b : (b == INT_MIN ? 0 : (b ^ 0x7fffffff));      // (INT_MIN is -0.0)
    return (unsigned)k ^ 0x80000000u;
}

__device__ __forceinline__ float logit_of(unsigned u) {
    const int k = (int)(u ^ 0x80000000u);
    return __int_as_float(k >= 0 ? k : (k ^ 0x7fffffff));
}

template <class F>
__device__ __forceinline__ void for_each_logit(const float* __restrict__ p, int n, int tid, bool vec, F&& f) {
    if (vec) {
        const int n4 = n >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(p);
        int i = tid;
        for (; i + 3 * THREADS < n4; i += 4 * THREADS) {     // four independent 16-byte loads in flight per thread
            const float4 v0 = p4[i], v1 = p4[i + THREADS], v2 = p4[i + 2 * THREADS], v3 = p4[i + 3 * THREADS];
            __builtin_amdgcn_sched_barrier(0);      // (all four issued before the first is consumed)
            f(v0.x); f(v0.y); f(v0.z); f(v0.w);
            f(v1.x); f(v1.y); f(v1.z); f(v1.w);
            f(v2.x); f(v2.y); f(v2.z); f(v2.w);
            f(v3.x); f(v3.y); f(v3.z); f(v3.w);
        }
        for (; i < n4; i += THREADS) {
            const float4 v = p4[i];
            f(v.x); f(v.y); f(v.z); f(v.w);
        }
    } else {        // a plane that does not start on a 16-byte boundary, or does not end on one
        for (int i = tid; i < n; i += THREADS) f(p[i]);
    }
}

struct CredArgs {
    const float* x;
    long long bs;
    int C, n, L;
    float t, inv_t;
    float q[MAXL];
    int* area;
    float* thr;
    float* mass;
    int* status;
};

template <bool DIVIDE>
__global__ __launch_bounds__(THREADS) void map_credible_kernel(const CredArgs a) {
    __shared__ u64 hist[BINS * SLOTS];            // 16 KB: [bin][slot] -- the copies of one bin lie in neighbouring banks
    __shared__ unsigned cnt[BINS * SLOTS];        //  8 KB
    __shared__ unsigned wkey[WAVES];
    __shared__ int wnan[WAVES];
    __shared__ unsigned prefix[MAXL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long plane = blockIdx.x;
    const int n = a.n, L = a.L;
    const float* __restrict__ p = a.x + (plane / a.C) * a.bs + (plane % a.C) * (long long)n;      // (plane_ptr, spelled out: see map_plane.h)
    const bool vec = (n & 3) == 0 && (((uintptr_t)p) & 15) == 0;

    // pass 0: the largest key, the NaN flag
    unsigned kmax = 0;
    bool poison = false;
    for_each_logit(p, n, tid, vec, [&](const float v) {
        poison = poison | (v != v);
        const unsigned k = key_of(v);
        kmax = k > kmax ? k : kmax;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)kmax, o, 64);
        kmax = other > kmax ? other : kmax;
    }
    const int any_poison = __any(poison);
    if (lane == 0) {
        wkey[wave] = kmax;
        wnan[wave] = any_poison;
    }
    __syncthreads();
    int bad = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        kmax = wkey[w] > kmax ? wkey[w] : kmax;
        bad |= wnan[w];
    }
    const float wmax = weight<DIVIDE>(logit_of(kmax), a.inv_t, a.t);
    if (bad != 0 || !(wmax > 0.f)) {      // a NaN logit: not ranked, flagged;  Z == 0: no region, no flag   (uniform: every thread leaves)
        if (tid < L) {
            a.area[plane * L + tid] = bad != 0 ? -1 : 0;
            a.thr[plane * L + tid] = __builtin_nanf("");
            a.mass[plane * L + tid] = __builtin_nanf("");
        }
        if (bad != 0 && tid == 0) atomicOr(a.status, 1);
        return;
    }
    const int k0 = fixed_scale(wmax, FRAC);      // mant << (ex + k0) lies in [2^40, 2^41)

    // what the wave of level `wave` carries from pass to pass (uniform over the wave)
    unsigned my_prefix = 0, my_cabove = 0;
    u64 my_above = 0, zint = 0;
    const double q = (double)a.q[wave < L ? wave : 0];

    for (int pass = 0; pass < PASSES; ++pass) {
        // groups: runs of levels with one prefix.  Unused slots hold a prefix no key has (a settled prefix is below 2^24).
        unsigned gp[SLOTS];
        int ng = 1, my_group = 0;
#pragma unroll
        for (int g = 0; g < SLOTS; ++g) gp[g] = 0xffffffffu;
        gp[0] = 0;
        if (pass > 0) {
            gp[0] = prefix[0];
            for (int l = 1; l < L; ++l) {
                const unsigned pl = prefix[l];
                if (pl != prefix[l - 1]) {
#pragma unroll
                    for (int g = 1; g < SLOTS; ++g)
                        if (g == ng) gp[g] = pl;
                    ++ng;
                }
                if (l == wave) my_group = ng - 1;
            }
        }
        const int copies = ng == 1 ? 8 : (ng == 2 ? 4 : (ng <= 4 ? 2 : 1));
        for (int i = tid; i < BINS * SLOTS; i += THREADS) {
            hist[i] = 0;
            cnt[i] = 0;
        }
        __syncthreads();

        const int hi_shift = 32 - DIGIT * pass, lo_shift = 32 - DIGIT * (pass + 1);
        const int my_copy = lane & (copies - 1);
        for_each_logit(p, n, tid, vec, [&](const float v) {
            const unsigned k = key_of(v);
            const unsigned hi = pass == 0 ? 0u : (k >> hi_shift);
            int g = -1;
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) g = (hi == gp[j]) ? j : g;
            if (g >= 0) {
                const int at = (int)((k >> lo_shift) & (BINS - 1)) * SLOTS + g * copies + my_copy;
                atomicAdd(&hist[at], fixed(weight<DIVIDE>(v, a.inv_t, a.t), k0));
                atomicAdd(&cnt[at], 1u);
            }
        });
        __syncthreads();

        // the walk: wave l takes level l; lane j takes the bins 255 - 4 j .. 252 - 4 j, so the lanes run from the top bin down
        if (wave < L) {
            u64 m[4];
            unsigned c[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int at = (BINS - 1 - 4 * lane - i) * SLOTS + my_group * copies;
                m[i] = 0;
                c[i] = 0;
                for (int r = 0; r < copies; ++r) {
                    m[i] += hist[at + r];
                    c[i] += cnt[at + r];
                }
            }
            const u64 msum = (m[0] + m[1]) + (m[2] + m[3]);
            const unsigned csum = (c[0] + c[1]) + (c[2] + c[3]);
            u64 mincl = msum;
            unsigned cincl = csum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {      // inclusive scan over the lanes
                const u64 mo = __shfl_up(mincl, o, 64);
                const unsigned co = (unsigned)__shfl_up((int)cincl, o, 64);
                if (lane >= o) {
                    mincl += mo;
                    cincl += co;
                }
            }
            if (pass == 0) zint = __shfl(mincl, 63, 64);      // every pixel is in pass 0's histogram
            const double target = q * (double)zint;
            // the first bin from the top at which the cumulative mass reaches the target
            u64 mb = my_above + (mincl - msum);      // mass and count above this lane's bins
            unsigned cb = my_cabove + (cincl - csum);
            int found = -1;
            u64 fm = 0, fmb = 0;
            unsigned fc = 0, fcb = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool hit = found < 0 && (double)(mb + m[i]) >= target;
                if (hit) {
                    found = i;
                    fm = m[i];
                    fc = c[i];
                    fmb = mb;
                    fcb = cb;
                }
                mb += m[i];
                cb += c[i];
            }
            const u64 ballot = __ballot(found >= 0);
            const int fl = ballot != 0 ? __builtin_ctzll(ballot) : 63;      // (exact integer sums: a crossing always exists)
            found = __shfl(found, fl, 64);
            fm = __shfl(fm, fl, 64);
            fmb = __shfl(fmb, fl, 64);
            fc = (unsigned)__shfl((int)fc, fl, 64);
            fcb = (unsigned)__shfl((int)fcb, fl, 64);
            const unsigned digit = (unsigned)(BINS - 1 - 4 * fl - (found < 0 ? 3 : found));
            my_prefix = (my_prefix << DIGIT) | digit;
            my_above = fmb;
            my_cabove = fcb;
            if (pass == PASSES - 1) {
                if (lane == 0) {      // the prefix is the whole key, the bin its plateau
                    a.area[plane * L + wave] = (int)(fcb + fc);
                    a.thr[plane * L + wave] = logit_of(my_prefix);
                    a.mass[plane * L + wave] = (float)((double)(fmb + fm) / (double)zint);
                }
            } else if (lane == 0) {
                prefix[wave] = my_prefix;
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int ynet_map_credible(const float* x, long long batch_stride, long long B, int C, int H, int W, const float* levels,
                                 int n_levels, float temperature, int* area, float* threshold, float* mass, int* status, void* stream) {
    YNET_REQUIRE(x != nullptr, "map_credible: null map");
    YNET_REQUIRE(levels != nullptr, "map_credible: null levels");
    YNET_REQUIRE(area != nullptr && threshold != nullptr && mass != nullptr, "map_credible: null output (area, threshold or mass)");
    YNET_REQUIRE(status != nullptr, "map_credible: null status flag");
    YNET_REQUIRE(n_levels >= 1 && n_levels <= YNET_MAP_CREDIBLE_MAX_LEVELS, "map_credible: n_levels = %d, expected 1 .. %d", n_levels,
                 YNET_MAP_CREDIBLE_MAX_LEVELS);
    for (int l = 0; l < n_levels; ++l) {
        YNET_REQUIRE(levels[l] > 0.f && levels[l] < 1.f, "map_credible: level %d = %g lies outside the open interval (0, 1)", l, (double)levels[l]);
        YNET_REQUIRE(l == 0 || levels[l] > levels[l - 1], "map_credible: the levels must ascend strictly (level %d = %g after %g)", l,
                     (double)levels[l], (double)levels[l - 1]);
    }
    if (map_check_temperature("map_credible", temperature) || map_check_shape("map_credible", B, C, H, W)) return 1;
    YNET_REQUIRE((long long)H * W <= YNET_MAP_CREDIBLE_MAX_PIXELS, "map_credible: a plane of %dx%d has more than the %d pixels the integer sums hold",
                 H, W, YNET_MAP_CREDIBLE_MAX_PIXELS);
    if (map_check_batch_stride("map_credible", batch_stride, C, H, W)) return 1;
    YNET_REQUIRE(B <= MAX_PLANES && B * C <= MAX_PLANES, "map_credible: too many planes (%lld x %d, at most %lld)", B, C, MAX_PLANES);
    CredArgs a;
    a.x = x;
    a.bs = batch_stride;
    a.C = C;
    a.n = H * W;
    a.L = n_levels;
    a.t = temperature;
    a.inv_t = 1.f / temperature;
    for (int l = 0; l < MAXL; ++l) a.q[l] = l < n_levels ? levels[l] : 0.f;
    a.area = area;
    a.thr = threshold;
    a.mass = mass;
    a.status = status;
    const dim3 grid((unsigned)(B * C)), block(THREADS);
    if (temperature == 1.f) hipLaunchKernelGGL(map_credible_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(map_credible_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
    return ynet_check_launch("map_credible");
}
