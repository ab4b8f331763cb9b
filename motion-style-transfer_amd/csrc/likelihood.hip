// Likelihood scores of the goal map (utils/evaluate.py:128-131 builds the distribution, utils/image_utils.py:110-135 draws from it;
// the reference keeps the draws and drops the distribution).  Per plane (agent b, step c), with z = x / T, w = sigmoid(z), Z = sum w:
//   nll     = log Z - log_sigmoid(z at the ground-truth pixel)
//   entropy = log Z - (sum w * log_sigmoid(z)) / Z
//   hpd     = (sum over {x >= x at the ground-truth pixel} of w) / Z            (membership on the raw fp32 logits: exact)
// One workgroup per plane, ONE pass over HBM: the three sums are known once the ground-truth logit has been read.  16-byte loads, eight
// in flight per thread, as softargmax_plane (glue.hip) but without its row / column bookkeeping.  Per-pixel terms are fp32; the running
// sums, the cross-wave combine and the final logs are fp64.  The public C ABI is include/ynet_hip.h.
#include "map_plane.h"

namespace {

// One logit in fp32 (z and w: sigmoid_term.h, shared with the sibling kernels).  With a = |z|, e = exp(-a), u = 1 + e:
//   w = sigmoid(z) = 1 / u (z >= 0), e / u (z < 0);   log_sigmoid(z) = zmin - l1p,  zmin = min(z, 0),  l1p = log1p(e) = log(u) + (e - (u - 1)) / u
// (the last term restores what the rounding of 1 + e dropped).  The two parts of log_sigmoid stay apart: zmin is exact and may be large,
// l1p <= log 2 carries the rounding -- rounded into one fp32 number their sum would lose half an ulp of |z|, which a plane of a few
// pixels (entropy ~ 0 as the difference of two numbers of that size) does not forgive.  zmin is clamped to -FLT_MAX, so that 0 * -inf
// never forms.  A NaN comes out as w = 0 here; the caller tracks NaNs itself.
struct Term {
    float w, zmin, l1p;
};

template <bool DIVIDE>
__device__ __forceinline__ Term logit_term(float x, float inv_t, float t) {
    const float z = tempered<DIVIDE>(x, inv_t, t);
    const SigmoidTerm s = sigmoid_term(z);
    Term o;
    o.l1p = __builtin_fmaf(__builtin_amdgcn_logf(s.u), 0.693147182464599609375f, (s.e - (s.u - 1.f)) * s.ru);
    o.w = sigmoid_weight(z, s);
    o.zmin = __builtin_amdgcn_fmed3f(z, -3.402823466e38f, 0.f);
    return o;
}

struct LikeArgs {
    const float* x;
    long long bs;
    const float* gt;        // [planes][2] (x, y) or NULL
    int C, H, W;
    float t, inv_t;
    float* nll;
    float* ent;
    float* hpd;
    int* status;
};

// DIVIDE: T != 1.  (A compile-time switch, and no branch anywhere in the unrolled loop body: with one, hipcc sinks each of the eight
// loads down to its use and waits for them one by one.)
template <bool DIVIDE>
__global__ __launch_bounds__(256) void map_likelihood_kernel(const LikeArgs a) {
    __shared__ double ws[4][3];
    __shared__ int wpoison[4];
    const int tid = threadIdx.x;
    const long long plane = blockIdx.x;
    const int n = a.H * a.W;
    const float* __restrict__ p = plane_ptr(a.x, a.bs, a.C, n, plane);
    bool in_map = false;
    float xg = INFINITY;
    if (a.gt != nullptr) {
        const GtPixel g = gt_pixel(a.gt, plane, p, a.H, a.W, a.status, tid);
        in_map = g.in_map;
        xg = g.xg;
    }
    // running sums in fp64: sum w, sum w * zmin (every product exact in fp64), sum w * l1p, sum of w over the members of the hpd region
    double sw = 0.0, shi = 0.0, slo = 0.0, sh = 0.0;
    bool poison = false;    // a NaN logit makes the whole plane NaN  (bit-wise ors below: a short-circuit || is a branch)
    auto fold1 = [&](const float v) {
        poison = poison | (v != v);
        const Term t = logit_term<DIVIDE>(v, a.inv_t, a.t);
        sw += (double)t.w;
        shi = __builtin_fma((double)t.w, (double)t.zmin, shi);
        slo += (double)(t.w * t.l1p);
        sh += (double)(v >= xg ? t.w : 0.f);
    };
    auto fold = [&](const float4 v) {
        poison = poison | __builtin_isunordered(v.x, v.y) | __builtin_isunordered(v.z, v.w);
        const Term t0 = logit_term<DIVIDE>(v.x, a.inv_t, a.t), t1 = logit_term<DIVIDE>(v.y, a.inv_t, a.t);
        const Term t2 = logit_term<DIVIDE>(v.z, a.inv_t, a.t), t3 = logit_term<DIVIDE>(v.w, a.inv_t, a.t);
        sw += (double)((t0.w + t1.w) + (t2.w + t3.w));
        shi = __builtin_fma((double)t0.w, (double)t0.zmin, shi);
        shi = __builtin_fma((double)t1.w, (double)t1.zmin, shi);
        shi = __builtin_fma((double)t2.w, (double)t2.zmin, shi);
        shi = __builtin_fma((double)t3.w, (double)t3.zmin, shi);
        slo += (double)((t0.w * t0.l1p + t1.w * t1.l1p) + (t2.w * t2.l1p + t3.w * t3.l1p));
        // (the same four values in the same tree as sw: where every pixel is a member the two sums are equal bit for bit, and hpd == 1)
        sh += (double)(((v.x >= xg ? t0.w : 0.f) + (v.y >= xg ? t1.w : 0.f)) + ((v.z >= xg ? t2.w : 0.f) + (v.w >= xg ? t3.w : 0.f)));
    };
    if ((n & 3) == 0 && (((uintptr_t)p) & 15) == 0) {
        const int n4 = n >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(p);
        int i = tid;
        for (; i + 7 * 256 < n4; i += 8 * 256) {     // eight independent 16-byte loads in flight per thread
            const float4 v0 = p4[i], v1 = p4[i + 256], v2 = p4[i + 512], v3 = p4[i + 768];
            const float4 v4 = p4[i + 1024], v5 = p4[i + 1280], v6 = p4[i + 1536], v7 = p4[i + 1792];
            __builtin_amdgcn_sched_barrier(0);      // (all eight issued before the first is consumed)
            fold(v0);
            fold(v1);
            fold(v2);
            fold(v3);
            fold(v4);
            fold(v5);
            fold(v6);
            fold(v7);
        }
        for (; i < n4; i += 256) fold(p4[i]);
    } else {        // a plane that does not start on a 16-byte boundary, or does not end on one
        for (int i = tid; i < n; i += 256) fold1(p[i]);
    }
    sw = wave_sum(sw);
    const double swl = wave_sum(shi - slo);
    sh = wave_sum(sh);
    const int any_poison = __any(poison);
    if ((tid & 63) == 0) {
        ws[tid >> 6][0] = sw;
        ws[tid >> 6][1] = swl;
        ws[tid >> 6][2] = sh;
        wpoison[tid >> 6] = any_poison;
    }
    __syncthreads();
    if (tid == 0) {
        const double nan = (double)__builtin_nanf("");
        double Z = four_wave_sum(&ws[0][0], 3);
        const double wl = four_wave_sum(&ws[0][1], 3), hs = four_wave_sum(&ws[0][2], 3);
        if (four_wave_poison(wpoison) || Z == 0.0) Z = nan;
        const double logz = log(Z);
        if (a.ent != nullptr) a.ent[plane] = (float)(logz - wl / Z);
        if (a.nll != nullptr) {
            double v = nan;
            if (in_map) {
                const double zg = (double)tempered<DIVIDE>(xg, a.inv_t, a.t);      // the z of the pass above: a one-pixel plane gives 0
                v = logz - (fmin(zg, 0.0) - log1p(exp(-fabs(zg))));
            }
            a.nll[plane] = (float)v;
        }
        if (a.hpd != nullptr) a.hpd[plane] = (float)(in_map ? hs / Z : nan);
    }
}

}  // namespace

extern "C" int ynet_map_likelihood(const float* x, long long batch_stride, const float* gt_xy, long long B, int C, int H, int W,
                                   float temperature, float* nll, float* entropy, float* hpd, int* status, void* stream) {
    YNET_REQUIRE(x != nullptr, "map_likelihood: null map");
    if (map_check_temperature("map_likelihood", temperature) || map_check_shape("map_likelihood", B, C, H, W) ||
        map_check_pixel_index("map_likelihood", H, W) || map_check_batch_stride("map_likelihood", batch_stride, C, H, W))
        return 1;
    YNET_REQUIRE(nll != nullptr || entropy != nullptr || hpd != nullptr, "map_likelihood: no output asked for");
    YNET_REQUIRE(gt_xy != nullptr || (nll == nullptr && hpd == nullptr), "map_likelihood: nll and hpd need the ground truth (gt_xy is null)");
    YNET_REQUIRE(gt_xy == nullptr || status != nullptr, "map_likelihood: the ground truth needs a status flag (status is null)");
    const long long planes = B * C;
    YNET_REQUIRE(planes < (1ll << 31), "map_likelihood: too many planes");
    LikeArgs a;
    a.x = x;
    a.bs = batch_stride;
    a.gt = gt_xy;
    a.C = C;
    a.H = H;
    a.W = W;
    a.t = temperature;
    a.inv_t = 1.f / temperature;
    a.nll = nll;
    a.ent = entropy;
    a.hpd = hpd;
    a.status = status;
    if (temperature == 1.f) hipLaunchKernelGGL(map_likelihood_kernel<false>, dim3((unsigned)planes), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(map_likelihood_kernel<true>, dim3((unsigned)planes), dim3(256), 0, (hipStream_t)stream, a);
    return ynet_check_launch("map_likelihood");
}
