// Goal / waypoint sampling of evaluate() on the device:
//
//   multinomial_topk_kernel   torch.multinomial(prob, K, replacement=False) of utils/image_utils.py:110-135 with a
//                             DOCUMENTED counter-based generator, so that a CPU restatement (oracle/ynet_oracle.py
//                             device_multinomial) reproduces every draw from the seed alone
//   multinomial_cdf_kernel    the replacement=True form (TTST's 10000 thresholded goal samples, utils/evaluate.py:137-139)
//   cws_prior_kernel          torch_multivariate_gaussian_heatmap x sigmoid map, normalised, and its expectation
//                             (conditioned waypoint sampling, utils/evaluate.py:9-34, 172-224)
//   score_rank_kernel         the K sampled futures of an agent scored against the goal map and ranked (predict())
//   score_rank_rows_kernel    the same body (score_rank_body), every agent's results written to a row of the caller's choosing
//                             (predict_styles())
//   gather_rows_kernel        dst[i, :] = src[idx[i], :]: a style-sorted batch built from the caller's rows (predict_styles())
//
// Random numbers: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11; the constants of Random123 / cuRAND / torch's
// device generator), key = (seed & 0xffffffff, seed >> 32), counter = (element, 0, row, stream) with stream 0 for the
// race without replacement and 1 for the inverse-CDF draws.  A 53-bit uniform in (0, 1) is built from the first two
// output words: u = ((x0 >> 5) * 2^26 + (x1 >> 6) + 0.5) * 2^-53.
//
// Without replacement (exponential race, the algorithm ATen's multinomial uses too): element i of row r gets the
// key  p_i / E_i,  E_i = -log(u_i)  (fp64);  the K samples are the indices of the K largest keys in DESCENDING key
// order (ties: smaller index first); p_i = 0 never wins.  With `rel_threshold` entries below threshold * max(row) are
// zeroed first (utils/image_utils.py:113-118).
// With replacement: the row is cut into 256 contiguous segments; cdf = (sequential fp64 sum of the segments before) +
// (sequential fp64 sum inside the segment); sample j takes the first element whose cdf >= u_j * total.
#include "ynet_common.h"
#include <math.h>

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned& o0, unsigned& o1) {
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

__device__ __forceinline__ double philox_uniform(unsigned elem, unsigned row, unsigned stream, unsigned k0, unsigned k1) {
    unsigned x0, x1;
    philox4x32_10(elem, 0u, row, stream, k0, k1, x0, x1);
    return ((double)(x0 >> 5) * 67108864.0 + (double)(x1 >> 6) + 0.5) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// max of a row (block-wide), every thread gets it
__device__ float block_row_max(const float* __restrict__ p, int n, float* red) {
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, p[i]);
    m = wave_max_f(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return m;
}

// ------------------------------------------------------------------------------------------------
// K samples without replacement per row; one workgroup per row.  Every thread keeps the K best keys of its
// (strided) elements in a sorted list in LDS, then K rounds of a block-wide arg-max over the list heads merge them.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void multinomial_topk_kernel(const float* __restrict__ prob, long long row_stride, int n,
                                                               int K, float rel_threshold, unsigned k0, unsigned k1,
                                                               long long* __restrict__ out, int* __restrict__ status,
                                                               const unsigned long long* __restrict__ seed_ptr) {
    if (seed_ptr != nullptr) {      // the seed as a device input (a captured evaluation sweep: ynet_multinomial_devseed)
        const unsigned long long sd = *seed_ptr;
        k0 = (unsigned)(sd & 0xffffffffull);
        k1 = (unsigned)(sd >> 32);
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double* lkey = reinterpret_cast<double*>(lds_raw);                 // [K][256]
    int* lidx = reinterpret_cast<int*>(lkey + (size_t)K * 256);        // [K][256]
    __shared__ float red[4];
    __shared__ double wkey[4];
    __shared__ int widx[4], wthr[4];
    const int tid = threadIdx.x, row = blockIdx.x;
    const float* p = prob + (long long)row * row_stride;
    float cut = 0.f;
    if (rel_threshold > 0.f) cut = block_row_max(p, n, red) * rel_threshold;
    for (int k = 0; k < K; ++k) {
        lkey[k * 256 + tid] = -1.0;
        lidx[k * 256 + tid] = 0x7fffffff;
    }
    double kmin = -1.0;         // this thread's K-th best so far
    for (int i = tid; i < n; i += 256) {
        float pv = p[i];
        if (rel_threshold > 0.f && pv < cut) pv = 0.f;
        if (!(pv > 0.f)) continue;
        const double u = philox_uniform((unsigned)i, (unsigned)row, 0u, k0, k1);
        const double key = (double)pv / -log(u);
        if (key > kmin) {       // insert (descending; elements arrive in increasing index order, so ties keep the smaller index first)
            int pos = K - 1;
            while (pos > 0 && lkey[(pos - 1) * 256 + tid] < key) {
                lkey[pos * 256 + tid] = lkey[(pos - 1) * 256 + tid];
                lidx[pos * 256 + tid] = lidx[(pos - 1) * 256 + tid];
                --pos;
            }
            lkey[pos * 256 + tid] = key;
            lidx[pos * 256 + tid] = i;
            kmin = lkey[(K - 1) * 256 + tid];
        }
    }
    int head = 0;
    for (int k = 0; k < K; ++k) {
        double bk = head < K ? lkey[head * 256 + tid] : -1.0;
        int bi = head < K ? lidx[head * 256 + tid] : 0x7fffffff;
        int bt = tid;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ok = __shfl_xor(bk, o, 64);
            const int oi = __shfl_xor(bi, o, 64), ot = __shfl_xor(bt, o, 64);
            if (ok > bk || (ok == bk && oi < bi)) {
                bk = ok;
                bi = oi;
                bt = ot;
            }
        }
        if ((tid & 63) == 0) {
            wkey[tid >> 6] = bk;
            widx[tid >> 6] = bi;
            wthr[tid >> 6] = bt;
        }
        __syncthreads();
        bk = wkey[0];
        bi = widx[0];
        bt = wthr[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (wkey[w] > bk || (wkey[w] == bk && widx[w] < bi)) {
                bk = wkey[w];
                bi = widx[w];
                bt = wthr[w];
            }
        __syncthreads();
        if (tid == bt) ++head;
        if (tid == 0) {
            if (!(bk > 0.0)) {          // fewer than K entries with positive probability (torch raises here)
                atomicExch(status, 1);
                bi = 0;
            }
            out[(long long)row * K + k] = bi;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K samples WITH replacement per row (inverse CDF in fp64, fixed summation order); one workgroup per row.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void multinomial_cdf_kernel(const float* __restrict__ prob, long long row_stride, int n, int K,
                                                              float rel_threshold, unsigned k0, unsigned k1,
                                                              long long* __restrict__ out, int* __restrict__ status,
                                                              const unsigned long long* __restrict__ seed_ptr) {
    if (seed_ptr != nullptr) {
        const unsigned long long sd = *seed_ptr;
        k0 = (unsigned)(sd & 0xffffffffull);
        k1 = (unsigned)(sd >> 32);
    }
    __shared__ float red[4];
    __shared__ double seg_off[257];      // exclusive sums of the segment totals, [256] = total
    const int tid = threadIdx.x, row = blockIdx.x;
    const float* p = prob + (long long)row * row_stride;
    float cut = 0.f;
    if (rel_threshold > 0.f) cut = block_row_max(p, n, red) * rel_threshold;
    const int seg = (n + 255) / 256;
    const int lo = min(n, tid * seg), hi = min(n, lo + seg);
    double s = 0.0;
    for (int i = lo; i < hi; ++i) {
        float pv = p[i];
        if (rel_threshold > 0.f && pv < cut) pv = 0.f;
        if (pv > 0.f) s += (double)pv;
    }
    seg_off[tid + 1] = s;
    __syncthreads();
    if (tid == 0) {
        double run = 0.0;
        seg_off[0] = 0.0;
        for (int t = 1; t <= 256; ++t) {
            run += seg_off[t];
            seg_off[t] = run;
        }
        if (!(run > 0.0)) atomicExch(status, 1);
    }
    __syncthreads();
    const double total = seg_off[256];
    for (int j = tid; j < K; j += 256) {
        const double target = philox_uniform((unsigned)j, (unsigned)row, 1u, k0, k1) * total;
        int a = 0, b = 256;             // first segment whose inclusive sum reaches the target
        while (a < b) {
            const int m = (a + b) >> 1;
            if (seg_off[m + 1] >= target) b = m;
            else a = m + 1;
        }
        const int t = min(a, 255);
        double run = seg_off[t];
        const int l2 = min(n, t * seg), h2 = min(n, l2 + seg);
        int pick = -1, last_pos = -1;
        for (int i = l2; i < h2; ++i) {
            float pv = p[i];
            if (rel_threshold > 0.f && pv < cut) pv = 0.f;
            if (pv > 0.f) {
                run += (double)pv;
                last_pos = i;
                if (run >= target) {
                    pick = i;
                    break;
                }
            }
        }
        if (pick < 0) pick = last_pos >= 0 ? last_pos : 0;
        out[(long long)row * K + j] = pick;
    }
}

// ------------------------------------------------------------------------------------------------
// Conditioned waypoint sampling prior.  For row n (person n % B of goal sample n / B):
//   k(x, y)  = exp(-0.5 * m^T T^-1 m),  m = (lin_W(x) - mean_x, lin_H(y) - mean_y),  lin_N(i) = i * N / (N - 1)
//   T        = R diag((d/sf/ratio)^2, (d/sf)^2) R^T,  d = |dist| + 5,  R = rotation by atan2(dist_x, dist_y) [, then 90 deg]
//   map      = sig * k / sum(sig * k)                                  (out_map, optional)
//   xy       = (sum x * map, sum y * map) over pixel indices x, y     (out_xy, optional)
// Everything per pixel in fp64 (the reference's fp32 chain is within 3e-6 pixels of the exact value; T^-1 is taken
// analytically as R diag(1/a, 1/b) R^T).  One workgroup per row.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cws_prior_kernel(const float* __restrict__ sig, long long sig_bs, int nb,
                                                        const float* __restrict__ mean_xy, const float* __restrict__ dist_xy,
                                                        int H, int W, float sigma_factor, float ratio, int rot,
                                                        float* __restrict__ out_map, float* __restrict__ out_xy) {
    __shared__ double wsum[4][3];
    const int tid = threadIdx.x, row = blockIdx.x;
    const float* s = sig + (long long)(row % nb) * sig_bs;
    const double mx = (double)mean_xy[2 * row], my = (double)mean_xy[2 * row + 1];
    const double dx = (double)dist_xy[2 * row], dy = (double)dist_xy[2 * row + 1];
    const double rad = atan2(dx, dy);
    double c = cos(rad), sn = sin(rad);
    // R = [[c, sn], [-sn, c]];  rot: R <- [[0, -1], [1, 0]] R = [[sn, -c], [c, sn]]
    double r00 = c, r01 = sn, r10 = -sn, r11 = c;
    if (rot) {
        r00 = sn;
        r01 = -c;
        r10 = c;
        r11 = sn;
    }
    const double d = sqrt(dx * dx + dy * dy) + 5.0;
    const double sa = d / (double)sigma_factor / (double)ratio, sb = d / (double)sigma_factor;
    const double ia = 1.0 / (sa * sa), ib = 1.0 / (sb * sb);
    // T^-1 = R diag(ia, ib) R^T
    const double t00 = r00 * r00 * ia + r01 * r01 * ib;
    const double t01 = r00 * r10 * ia + r01 * r11 * ib;
    const double t11 = r10 * r10 * ia + r11 * r11 * ib;
    const double stepx = W > 1 ? (double)W / (double)(W - 1) : 0.0, stepy = H > 1 ? (double)H / (double)(H - 1) : 0.0;
    const int n = H * W;
    double S = 0.0, Sx = 0.0, Sy = 0.0;
    for (int i = tid; i < n; i += 256) {
        const int y = i / W, x = i - y * W;
        const double X = (double)x * stepx - mx, Y = (double)y * stepy - my;
        const double q = X * (t00 * X + t01 * Y) + Y * (t01 * X + t11 * Y);
        const double v = (double)s[i] * exp(-0.5 * q);
        S += v;
        Sx += v * (double)x;
        Sy += v * (double)y;
    }
    S = wave_sum_d(S);
    Sx = wave_sum_d(Sx);
    Sy = wave_sum_d(Sy);
    if ((tid & 63) == 0) {
        wsum[tid >> 6][0] = S;
        wsum[tid >> 6][1] = Sx;
        wsum[tid >> 6][2] = Sy;
    }
    __syncthreads();
    S = (wsum[0][0] + wsum[1][0]) + (wsum[2][0] + wsum[3][0]);
    Sx = (wsum[0][1] + wsum[1][1]) + (wsum[2][1] + wsum[3][1]);
    Sy = (wsum[0][2] + wsum[1][2]) + (wsum[2][2] + wsum[3][2]);
    if (out_xy != nullptr && tid == 0) {
        out_xy[2 * row] = (float)(Sx / S);
        out_xy[2 * row + 1] = (float)(Sy / S);
    }
    if (out_map != nullptr) {
        float* o = out_map + (long long)row * n;
        const double inv = 1.0 / S;
        for (int i = tid; i < n; i += 256) {
            const int y = i / W, x = i - y * W;
            const double X = (double)x * stepx - mx, Y = (double)y * stepy - my;
            const double q = X * (t00 * X + t01 * Y) + Y * (t01 * X + t11 * Y);
            o[i] = (float)((double)s[i] * exp(-0.5 * q) * inv);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Scoring and ranking of the K sampled futures of an agent (predict(): utils/evaluate.py:229-266 without the ground
// truth).  One wavefront per agent, sample k on lane k:
//   score_k = sum over way-points w (in order, fp32) of logf(prob[b][w][y][x] + 1e-12f),  (x, y) = rint of the sample
//   rank_k  = #{j : score_j > score_k  or  (score_j == score_k and j < k)}               (descending, ties to the lower index)
// The ranks are counted in the wave with one broadcast per sample (no LDS storage, no atomics); ds_permute sends k to lane
// rank_k, so lane r knows the sample that takes output row r.  Rows are copied as (x, y) pairs, lanes along the output.
// A sample that rounds to a pixel outside the map is not read: *status becomes 1 (every lane that sees one writes the same value).
//
// Agent b reads its own maps and samples at b.  score_rank_kernel writes score / order / ranked / ranked_goals at row b;
// score_rank_rows_kernel (ROWS) writes them at row out_row[b], for a batch that was reordered before the sweep (predict_styles() sorts
// the agents by style), so the results land in the caller's order from this launch (no pass over [N, K, pred_len, 2] afterwards).
// out_row must be a permutation of 0 .. B - 1 (two agents with one row would race); an entry outside 0 .. B - 1 is never used as an
// address: the agent's wave writes nothing and *status becomes 2.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int score_order_key(float s) {
    // a total order on the bits (a NaN score still gets a rank of its own): larger key = better sample
    const int b = __float_as_int(s + 0.f);      // (-0 -> +0)
    return b >= 0 ? b : (b ^ 0x7fffffff);
}

template <bool ROWS>
__device__ __forceinline__ void score_rank_body(const float* __restrict__ prob, const float* __restrict__ wps, const float* __restrict__ trajs,
                                                const int* __restrict__ out_row, int B, int K, int n_wp, int pred_len, int H, int W,
                                                float inv_resize, float* __restrict__ score, int* __restrict__ order,
                                                float* __restrict__ ranked, float* __restrict__ ranked_goals, int* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;      // (whole waves leave; nothing below synchronises the workgroup)
    const long long row = ROWS ? out_row[b] : b;
    if (ROWS && (row < 0 || row >= B)) {      // (the same for all 64 lanes: the wave leaves as one)
        *status = 2;
        return;
    }
    const long long plane = (long long)H * W;
    float s = 0.f;
    if (lane < K) {
        const float2* wp = reinterpret_cast<const float2*>(wps) + ((long long)lane * B + b) * n_wp;
        const float* pb = prob + b * n_wp * plane;
        bool bad = false;
        for (int w = 0; w < n_wp; ++w) {
            const float2 c = wp[w];
            const float fx = rintf(c.x), fy = rintf(c.y);
            if (fx >= 0.f && fx < (float)W && fy >= 0.f && fy < (float)H) {
                s += logf(pb[w * plane + (long long)fy * W + (long long)fx] + 1e-12f);
            } else {
                bad = true;
            }
        }
        if (bad) *status = 1;
    }
    // every cross-lane step below runs with all 64 lanes active: a shuffle reads nothing from a lane that has left
    const int key = score_order_key(s);
    int rank = 0;
    for (int j = 0; j < K; ++j) {
        const int kj = __shfl(key, j, 64);
        rank += (kj > key || (kj == key && j < lane)) ? 1 : 0;
    }
    if (lane >= K) rank = lane;      // lanes past K keep their own number: the permutation stays one-to-one
    const int src = __builtin_amdgcn_ds_permute(rank << 2, lane);      // lane r <- the sample whose rank is r
    const float s_src = __shfl(s, src, 64);
    if (lane < K) {
        order[row * K + lane] = src;
        score[row * K + lane] = s_src;
    }
    {
        const float2* in = reinterpret_cast<const float2*>(trajs);
        float2* out = reinterpret_cast<float2*>(ranked) + row * K * pred_len;
        const int total = K * pred_len;
        for (int i0 = 0; i0 < total; i0 += 64) {
            const int i = i0 + lane, r = min(i, total - 1) / pred_len, t = i - r * pred_len;
            const int k = __shfl(src, r, 64);
            if (i < total) {
                float2 v = in[((long long)k * B + b) * pred_len + t];
                v.x *= inv_resize;
                v.y *= inv_resize;
                out[i] = v;
            }
        }
    }
    {
        const float2* in = reinterpret_cast<const float2*>(wps);
        float2* out = reinterpret_cast<float2*>(ranked_goals) + row * K * n_wp;
        const int total = K * n_wp;
        for (int i0 = 0; i0 < total; i0 += 64) {
            const int i = i0 + lane, r = min(i, total - 1) / n_wp, w = i - r * n_wp;
            const int k = __shfl(src, r, 64);
            if (i < total) out[i] = in[((long long)k * B + b) * n_wp + w];
        }
    }
}

// (two __global__ functions under plain names and not one templated kernel: profiles/ and DESIGN.md name them as a profiler prints them)
__global__ __launch_bounds__(256) void score_rank_kernel(const float* __restrict__ prob, const float* __restrict__ wps,
                                                         const float* __restrict__ trajs, int B, int K, int n_wp, int pred_len, int H,
                                                         int W, float inv_resize, float* __restrict__ score, int* __restrict__ order,
                                                         float* __restrict__ ranked, float* __restrict__ ranked_goals,
                                                         int* __restrict__ status) {
    score_rank_body<false>(prob, wps, trajs, nullptr, B, K, n_wp, pred_len, H, W, inv_resize, score, order, ranked, ranked_goals, status);
}

__global__ __launch_bounds__(256) void score_rank_rows_kernel(const float* __restrict__ prob, const float* __restrict__ wps,
                                                              const float* __restrict__ trajs, const int* __restrict__ out_row, int B, int K,
                                                              int n_wp, int pred_len, int H, int W, float inv_resize,
                                                              float* __restrict__ score, int* __restrict__ order, float* __restrict__ ranked,
                                                              float* __restrict__ ranked_goals, int* __restrict__ status) {
    score_rank_body<true>(prob, wps, trajs, out_row, B, K, n_wp, pred_len, H, W, inv_resize, score, order, ranked, ranked_goals, status);
}

// ------------------------------------------------------------------------------------------------
// dst[i][:] = src[idx[i]][:] for n rows of `units` elements T (a float, or a float2 for rows of an even number of floats behind 8-byte
// aligned pointers).  Grid-stride over the n * units elements, 64-bit offsets throughout.  An index outside 0 .. src_rows - 1 is never
// used as an address: that row of dst is left as it was and *status becomes 1.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_kernel(const T* __restrict__ src, long long src_rows, const int* __restrict__ idx,
                                                          T* __restrict__ dst, long long n, int units, int* __restrict__ status) {
    const long long total = n * units, step = (long long)gridDim.x * 256;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
        const long long i = e / units;
        const long long r = idx[i];
        if (r < 0 || r >= src_rows) {
            *status = 1;
            continue;
        }
        dst[e] = src[r * units + (e - i * units)];
    }
}

static int multinomial_impl(const float* prob, long long rows, long long row_stride, int n, int K, int replacement,
                            float rel_threshold, unsigned long long seed, const unsigned long long* seed_ptr, long long* out, int* status,
                            void* stream) {
    YNET_REQUIRE(prob && out && status, "multinomial: null pointer");
    YNET_REQUIRE(rows > 0 && rows < (1ll << 31) && n > 0 && K > 0, "multinomial: bad shape rows=%lld n=%d K=%d", rows, n, K);
    YNET_REQUIRE(rel_threshold >= 0.f && rel_threshold <= 1.f, "multinomial: rel_threshold must lie in [0, 1]");
    const unsigned k0 = (unsigned)(seed & 0xffffffffull), k1 = (unsigned)(seed >> 32);
    if (replacement) {
        hipLaunchKernelGGL(multinomial_cdf_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, prob, row_stride, n, K,
                           rel_threshold, k0, k1, out, status, seed_ptr);
        return ynet_check_launch("multinomial(replacement)");
    }
    YNET_REQUIRE(K <= 48 && K <= n, "multinomial: without replacement K <= min(48, n) is supported (got K=%d, n=%d)", K, n);
    const int lds = K * 256 * 12;
    static bool attr_dev[YNET_MAX_DEV] = {false};
    bool& attr_set = attr_dev[ynet_device_slot()];
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(multinomial_topk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  48 * 256 * 12);
        attr_set = true;
    }
    hipLaunchKernelGGL(multinomial_topk_kernel, dim3((unsigned)rows), dim3(256), lds, (hipStream_t)stream, prob, row_stride, n, K,
                       rel_threshold, k0, k1, out, status, seed_ptr);
    return ynet_check_launch("multinomial");
}

extern "C" {

int ynet_multinomial(const float* prob, long long rows, long long row_stride, int n, int K, int replacement,
                     float rel_threshold, unsigned long long seed, long long* out, int* status, void* stream) {
    return multinomial_impl(prob, rows, row_stride, n, K, replacement, rel_threshold, seed, nullptr, out, status, stream);
}

// ynet_multinomial with the seed read from device memory by the kernel (8 bytes, 8-byte aligned): the launch has no per-call
// argument and can be recorded into a hipGraph (utils/evaluate.py: the captured sweep copies the seeds it draws into a static buffer)
int ynet_multinomial_devseed(const float* prob, long long rows, long long row_stride, int n, int K, int replacement,
                             float rel_threshold, const unsigned long long* seed_dev, long long* out, int* status, void* stream) {
    YNET_REQUIRE(seed_dev != nullptr && (reinterpret_cast<uintptr_t>(seed_dev) & 7) == 0, "multinomial_devseed: null / unaligned seed pointer");
    return multinomial_impl(prob, rows, row_stride, n, K, replacement, rel_threshold, 0ull, seed_dev, out, status, stream);
}

int ynet_cws_prior(const float* sig, long long sig_batch_stride, int n_persons, const float* mean_xy, const float* dist_xy,
                   int rows, int H, int W, float sigma_factor, float ratio, int rot, float* out_map, float* out_xy,
                   void* stream) {
    YNET_REQUIRE(sig && mean_xy && dist_xy && (out_map || out_xy), "cws_prior: null pointer");
    YNET_REQUIRE(rows > 0 && n_persons > 0 && H > 0 && W > 0, "cws_prior: bad shape rows=%d persons=%d %dx%d", rows, n_persons, H, W);
    YNET_REQUIRE(sigma_factor != 0.f && ratio != 0.f, "cws_prior: sigma_factor and ratio must be non-zero");
    hipLaunchKernelGGL(cws_prior_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, sig, sig_batch_stride, n_persons,
                       mean_xy, dist_xy, H, W, sigma_factor, ratio, rot, out_map, out_xy);
    return ynet_check_launch("cws_prior");
}

// The K sampled futures of each agent, scored against the goal map and handed back best first (utils/evaluate.py:229-266 draws
// and decodes them; utils/image_utils.py:110-135: a sample is (x, y) = (column, row) of the map).  Contiguous arrays; see the header.
// ynet_score_rank_samples_rows is the same call for a batch the caller reordered before the sweep: agent b writes its results at row
// out_row[b] (B device ints, a permutation of 0 .. B - 1).  `what` is the entry's name in the messages, `rows` whether it takes out_row.
static int score_rank_launch(const char* what, bool rows, const float* prob, const float* waypoint_samples, const float* trajs,
                             const int* out_row, int B, int K, int n_wp, int pred_len, int H, int W, float inv_resize_factor, float* score,
                             int* order, float* ranked, float* ranked_goals, int* status, void* stream) {
    YNET_REQUIRE(K >= 1 && K <= 64, "%s: K = %d samples per agent; one wavefront ranks 1 .. 64", what, K);
    YNET_REQUIRE(prob && waypoint_samples && trajs && (out_row || !rows) && score && order && ranked && ranked_goals && status,
                 "%s: null pointer", what);
    YNET_REQUIRE(B > 0 && n_wp > 0 && pred_len > 0 && H > 0 && W > 0 && n_wp <= (1 << 16) && pred_len <= (1 << 16),
                 "%s: bad shape B=%d n_wp=%d pred_len=%d map %dx%d", what, B, n_wp, pred_len, H, W);
    YNET_REQUIRE(inv_resize_factor > 0.f && inv_resize_factor < INFINITY, "%s: 1 / resize_factor must be positive and finite", what);
    YNET_REQUIRE(((reinterpret_cast<uintptr_t>(waypoint_samples) | reinterpret_cast<uintptr_t>(trajs) | reinterpret_cast<uintptr_t>(ranked) |
                   reinterpret_cast<uintptr_t>(ranked_goals)) & 7) == 0,
                 "%s: the (x, y) arrays must be 8-byte aligned", what);
    YNET_REQUIRE((reinterpret_cast<uintptr_t>(out_row) & 3) == 0, "%s: out_row must be 4-byte aligned", what);
    const dim3 grid((unsigned)ceil_div(B, 4));
    if (rows) {
        hipLaunchKernelGGL(score_rank_rows_kernel, grid, dim3(256), 0, (hipStream_t)stream, prob, waypoint_samples, trajs, out_row, B, K, n_wp,
                           pred_len, H, W, inv_resize_factor, score, order, ranked, ranked_goals, status);
    } else {
        hipLaunchKernelGGL(score_rank_kernel, grid, dim3(256), 0, (hipStream_t)stream, prob, waypoint_samples, trajs, B, K, n_wp, pred_len, H,
                           W, inv_resize_factor, score, order, ranked, ranked_goals, status);
    }
    return ynet_check_launch(what);
}

int ynet_score_rank_samples(const float* prob, const float* waypoint_samples, const float* trajs, int B, int K, int n_wp, int pred_len,
                            int H, int W, float inv_resize_factor, float* score, int* order, float* ranked, float* ranked_goals,
                            int* status, void* stream) {
    return score_rank_launch("score_rank_samples", false, prob, waypoint_samples, trajs, nullptr, B, K, n_wp, pred_len, H, W,
                             inv_resize_factor, score, order, ranked, ranked_goals, status, stream);
}

int ynet_score_rank_samples_rows(const float* prob, const float* waypoint_samples, const float* trajs, const int* out_row, int B, int K,
                                 int n_wp, int pred_len, int H, int W, float inv_resize_factor, float* score, int* order, float* ranked,
                                 float* ranked_goals, int* status, void* stream) {
    return score_rank_launch("score_rank_samples_rows", true, prob, waypoint_samples, trajs, out_row, B, K, n_wp, pred_len, H, W,
                             inv_resize_factor, score, order, ranked, ranked_goals, status, stream);
}

// dst[i][0 .. L) = src[idx[i]][0 .. L): the row gather predict_styles() builds its style-sorted batch with (see the header).
int ynet_gather_rows(const float* src, long long src_rows, const int* idx, float* dst, long long n, int L, int* status, void* stream) {
    YNET_REQUIRE(src && idx && dst && status, "gather_rows: null pointer");
    YNET_REQUIRE(src_rows > 0 && src_rows < (1ll << 31) && n > 0 && n < (1ll << 31) && L > 0,
                 "gather_rows: bad shape src_rows=%lld n=%lld L=%d", src_rows, n, L);
    YNET_REQUIRE(((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(idx)) & 3) == 0,
                 "gather_rows: pointers must be 4-byte aligned");
    const bool pairs = L % 2 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 7) == 0;
    const int units = pairs ? L / 2 : L;
    const long long blocks = (n * units + 255) / 256;
    const dim3 grid((unsigned)(blocks < (1ll << 16) ? blocks : (1ll << 16)));
    if (pairs) {
        hipLaunchKernelGGL(gather_rows_kernel<float2>, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float2*>(src), src_rows,
                           idx, reinterpret_cast<float2*>(dst), n, units, status);
    } else {
        hipLaunchKernelGGL(gather_rows_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, src, src_rows, idx, dst, n, units, status);
    }
    return ynet_check_launch("gather_rows");
}

}  // extern "C"
