// Scene compliance of the goal map: how much of the distribution `sampling` draws from (utils/evaluate.py:128-131,
// utils/image_utils.py:110-135) lies on each semantic class of the scene.  Per plane (agent b, step c), with z = x / T, w = sigmoid(z),
// Z = sum w over the whole plane and one class label per pixel:
//   mass[b, c, k] = (sum over {i : labels[i] == k} of w_i) / Z
// One workgroup per plane, ONE pass over HBM, structured as map_likelihood_kernel (likelihood.hip): 16-byte logit loads, eight in
// flight per thread, and beside each one 4-byte load of the four labels.  Per-pixel terms are fp32 (sigmoid_term.h: the same z and the
// same w as the likelihood kernels form); the running sums, the cross-wave combine and the division are fp64.  The public C ABI is
// include/ynet_hip.h.
#include "map_plane.h"
#include "../../include/ynet_hip.h"

namespace {

struct MassArgs {
    const float* x;
    long long bs;
    const unsigned char* labels;
    long long lbs;          // bytes between the label planes of two rows; 0: one plane for the whole call
    int lstep;              // 1: the distance between two labels, as a run-time value (see the element-wise path)
    int C, H, W;
    float t, inv_t;
    float* mass;
};

// DIVIDE: T != 1; K: the number of classes.  (Both compile-time, and no branch anywhere in the unrolled loop body -- see the DIVIDE
// comment of likelihood.hip; with K fixed the class sums are K register pairs and a launch pays for its own classes only.)
template <bool DIVIDE, int K>
__global__ __launch_bounds__(256) void map_class_mass_kernel(const MassArgs a) {
    __shared__ double ws[4][K + 1];
    __shared__ int wpoison[4];
    const int tid = threadIdx.x;
    const long long plane = blockIdx.x;
    const long long row = plane / a.C;
    const int n = a.H * a.W;
    const float* __restrict__ p = a.x + row * a.bs + (plane % a.C) * (long long)n;      // (plane_ptr, spelled out: see map_plane.h)
    const unsigned char* __restrict__ lab = a.labels + row * a.lbs;
    // running sums in fp64: sum w, and per class the sum of w over its pixels
    double sw = 0.0;
    double sc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) sc[k] = 0.0;
    bool poison = false;    // a NaN logit makes the whole plane NaN  (bit-wise ors below: a short-circuit || is a branch)
    auto fold1 = [&](const float v, const unsigned l) {
        poison = poison | (v != v);
        const float w = weight<DIVIDE>(v, a.inv_t, a.t);
        sw += (double)w;
#pragma unroll
        for (int k = 0; k < K; ++k) sc[k] += (double)(l == (unsigned)k ? w : 0.f);
    };
    auto fold = [&](const float4 v, const unsigned l4) {
        poison = poison | __builtin_isunordered(v.x, v.y) | __builtin_isunordered(v.z, v.w);
        const float w0 = weight<DIVIDE>(v.x, a.inv_t, a.t), w1 = weight<DIVIDE>(v.y, a.inv_t, a.t);
        const float w2 = weight<DIVIDE>(v.z, a.inv_t, a.t), w3 = weight<DIVIDE>(v.w, a.inv_t, a.t);
        const unsigned l0 = l4 & 255u, l1 = (l4 >> 8) & 255u, l2 = (l4 >> 16) & 255u, l3 = l4 >> 24;
        sw += (double)((w0 + w1) + (w2 + w3));
        // (the same four values in the same tree as sw: where every pixel has class k the two sums are equal bit for bit and mass == 1,
        // and a class with no pixel sums zeros alone)
#pragma unroll
        for (int k = 0; k < K; ++k)
            sc[k] += (double)(((l0 == (unsigned)k ? w0 : 0.f) + (l1 == (unsigned)k ? w1 : 0.f)) + ((l2 == (unsigned)k ? w2 : 0.f) + (l3 == (unsigned)k ? w3 : 0.f)));
    };
    // wide loads need the plane to end and to start on a 16-byte boundary, and its labels to start on a 4-byte one
    if ((n & 3) == 0 && (((uintptr_t)p) & 15) == 0 && (((uintptr_t)lab) & 3) == 0) {
        const int n4 = n >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(p);
        const unsigned* q4 = reinterpret_cast<const unsigned*>(lab);
        int i = tid;
        for (; i + 7 * 256 < n4; i += 8 * 256) {     // eight independent 16-byte loads in flight per thread, and their eight label words
            const float4 v0 = p4[i], v1 = p4[i + 256], v2 = p4[i + 512], v3 = p4[i + 768];
            const float4 v4 = p4[i + 1024], v5 = p4[i + 1280], v6 = p4[i + 1536], v7 = p4[i + 1792];
            const unsigned l0 = q4[i], l1 = q4[i + 256], l2 = q4[i + 512], l3 = q4[i + 768];
            const unsigned l4 = q4[i + 1024], l5 = q4[i + 1280], l6 = q4[i + 1536], l7 = q4[i + 1792];
            __builtin_amdgcn_sched_barrier(0);      // (all sixteen issued before the first is consumed)
            // (a fence after each fold: left alone the scheduler runs the eight folds side by side and holds all their per-class
            // partial sums at once -- K = 6 then takes 148 registers instead of 67)
            fold(v0, l0);
            __builtin_amdgcn_sched_barrier(0);
            fold(v1, l1);
            __builtin_amdgcn_sched_barrier(0);
            fold(v2, l2);
            __builtin_amdgcn_sched_barrier(0);
            fold(v3, l3);
            __builtin_amdgcn_sched_barrier(0);
            fold(v4, l4);
            __builtin_amdgcn_sched_barrier(0);
            fold(v5, l5);
            __builtin_amdgcn_sched_barrier(0);
            fold(v6, l6);
            __builtin_amdgcn_sched_barrier(0);
            fold(v7, l7);
        }
        for (; i < n4; i += 256) fold(p4[i], q4[i]);
    } else {
        // A plane or a label plane off its boundary, or a plane that does not end on one: element-wise loads, nothing assumed about
        // alignment.  The pixels are still taken four at a time, by the same threads in the same order and through the same fold as
        // above, so a plane gives the same bits whichever path its addresses send it down; the n % 4 pixels left go one by one.
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += 256) {
            const float* q = p + 4 * (long long)i;
            const unsigned char* lq = lab + 4 * (long long)i;
            // (the label stride is the run-time 1 of the argument block: with a literal 1 hipcc fuses the four byte loads into one
            // 4-byte load at whatever address the labels start, which is the misaligned wide load this path exists to avoid)
            const int s1 = a.lstep;
            fold(make_float4(q[0], q[1], q[2], q[3]),
                 (unsigned)lq[0] | ((unsigned)lq[s1] << 8) | ((unsigned)lq[2 * s1] << 16) | ((unsigned)lq[3 * s1] << 24));
        }
        for (int i = (n4 << 2) + tid; i < n; i += 256) fold1(p[i], lab[i]);
    }
    sw = wave_sum(sw);
#pragma unroll
    for (int k = 0; k < K; ++k) sc[k] = wave_sum(sc[k]);
    const int any_poison = __any(poison);
    if ((tid & 63) == 0) {
        ws[tid >> 6][0] = sw;
#pragma unroll
        for (int k = 0; k < K; ++k) ws[tid >> 6][1 + k] = sc[k];
        wpoison[tid >> 6] = any_poison;
    }
    __syncthreads();
    if (tid < K) {      // thread k: class k, the four waves' sums in the order Z takes them
        const double Z = four_wave_sum(&ws[0][0], K + 1), s = four_wave_sum(&ws[0][1 + tid], K + 1);
        const bool bad = four_wave_poison(wpoison) || Z == 0.0;
        a.mass[plane * K + tid] = bad ? __builtin_nanf("") : (float)(s / Z);
    }
}

template <bool DIVIDE>
void launch(int K, long long planes, const MassArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)planes), block(256);
    switch (K) {
    case 1: hipLaunchKernelGGL((map_class_mass_kernel<DIVIDE, 1>), grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((map_class_mass_kernel<DIVIDE, 2>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((map_class_mass_kernel<DIVIDE, 3>), grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((map_class_mass_kernel<DIVIDE, 4>), grid, block, 0, stream, a); break;
    case 5: hipLaunchKernelGGL((map_class_mass_kernel<DIVIDE, 5>), grid, block, 0, stream, a); break;
    case 6: hipLaunchKernelGGL((map_class_mass_kernel<DIVIDE, 6>), grid, block, 0, stream, a); break;
    case 7: hipLaunchKernelGGL((map_class_mass_kernel<DIVIDE, 7>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((map_class_mass_kernel<DIVIDE, 8>), grid, block, 0, stream, a); break;
    }
}

}  // namespace

static_assert(YNET_MAP_MAX_CLASSES == 8, "the class switch above covers 1 .. 8");

extern "C" int ynet_map_class_mass(const float* x, long long batch_stride, const unsigned char* labels, long long label_batch_stride,
                                   long long B, int C, int H, int W, int n_classes, float temperature, float* mass, void* stream) {
    YNET_REQUIRE(x != nullptr, "map_class_mass: null map");
    YNET_REQUIRE(labels != nullptr, "map_class_mass: null labels");
    YNET_REQUIRE(mass != nullptr, "map_class_mass: null output (mass)");
    YNET_REQUIRE(n_classes >= 1 && n_classes <= YNET_MAP_MAX_CLASSES, "map_class_mass: n_classes = %d, expected 1 .. %d", n_classes,
                 YNET_MAP_MAX_CLASSES);
    if (map_check_temperature("map_class_mass", temperature) || map_check_shape("map_class_mass", B, C, H, W) ||
        map_check_pixel_index("map_class_mass", H, W) || map_check_batch_stride("map_class_mass", batch_stride, C, H, W))
        return 1;
    YNET_REQUIRE(label_batch_stride == 0 || label_batch_stride >= (long long)H * W,
                 "map_class_mass: label batch stride %lld is neither 0 (one label plane for all rows) nor at least the %dx%d bytes of a plane",
                 label_batch_stride, H, W);
    const long long planes = B * C;
    YNET_REQUIRE(planes < (1ll << 31), "map_class_mass: too many planes");
    MassArgs a;
    a.x = x;
    a.bs = batch_stride;
    a.labels = labels;
    a.lbs = label_batch_stride;
    a.lstep = 1;
    a.C = C;
    a.H = H;
    a.W = W;
    a.t = temperature;
    a.inv_t = 1.f / temperature;
    a.mass = mass;
    if (temperature == 1.f) launch<false>(n_classes, planes, a, (hipStream_t)stream);
    else launch<true>(n_classes, planes, a, (hipStream_t)stream);
    return ynet_check_launch("map_class_mass");
}
