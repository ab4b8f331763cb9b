// Scene occupancy of the goal map: the distributions `sampling` draws from (utils/evaluate.py:128-131, utils/image_utils.py:110-135)
// of ALL the agents of a scene, summed per step.  Per group g (a run of rows of x: the agents of one scene), step c and cell of
// cell x cell pixels, with z = x / T, w = sigmoid(z), Z_a = sum w over agent a's plane and m_a = (sum of w over the cell) / Z_a:
//   occupancy = D = sum_a m_a      any = 1 - prod_a (1 - m_a)      conflict = 1/2 sum_cells (D^2 - sum_a m_a^2)
//   risk_a = sum_cells m_a (D - m_a)
// Three kernels behind one entry point, no floating-point atomic anywhere (two runs give the same bits):
//   1. occupancy_normalise_kernel   1 / Z_a in fp64 per plane (NaN for a plane with a NaN logit or Z == 0): map_class_mass_kernel
//                                   (compliance.hip) with no classes -- same loads, same fp64 combine order
//   2. occupancy_accumulate_kernel  one workgroup per (g, c, tile of 64 patches); a thread owns a patch of max(4, cell) x cell pixels,
//                                   that is 4 / 2 / 1 / 1 whole cells at cell 1 / 2 / 4 / 8, so no cell is shared between lanes, and
//                                   walks agents in row order with D, sum m^2 and prod (1 - m) in fp64 registers.  The larger the
//                                   patch, the fewer the tiles: the workgroup has 1 / 2 / 4 / 8 waves that take consecutive runs of
//                                   the group's agents and add their sums through LDS in wave order, so a coarse cell still puts
//                                   enough waves on the chip.  A second walk over the same agents (only when risk is
//                                   wanted) forms each agent's sum m (D - m).
//   3. occupancy_combine_kernel     the tile partials of every (g, c) and (a, c), summed in a fixed order in fp64
// Per-pixel terms are fp32 (sigmoid_term.h: the same z and the same w as the likelihood kernels form).  The public C ABI is
// include/ynet_hip.h.
#include "map_plane.h"
#include "../../include/ynet_hip.h"

namespace {

// ---- 1. the normalisers -----------------------------------------------------------------------------------------------------------------
struct NormArgs {
    const float* x;
    long long bs;
    int C, H, W;
    float t, inv_t;
    double* rz;             // [B * C]: 1 / Z, NaN for a plane that holds a NaN logit or whose weights are all 0
};

// One workgroup per plane, as map_class_mass_kernel: eight 16-byte loads in flight per thread, fp32 terms, fp64 sums.
template <bool DIVIDE>
__global__ __launch_bounds__(256) void occupancy_normalise_kernel(const NormArgs a) {
    __shared__ double ws[4];
    __shared__ int wpoison[4];
    const int tid = threadIdx.x;
    const long long plane = blockIdx.x;
    const long long row = plane / a.C;
    const int n = a.H * a.W;
    const float* __restrict__ p = a.x + row * a.bs + (plane % a.C) * (long long)n;      // (plane_ptr, spelled out: see map_plane.h)
    double sw = 0.0;
    bool poison = false;    // (bit-wise ors below: a short-circuit || is a branch)
    auto fold1 = [&](const float v) {
        poison = poison | (v != v);
        sw += (double)weight<DIVIDE>(v, a.inv_t, a.t);
    };
    auto fold = [&](const float4 v) {
        poison = poison | __builtin_isunordered(v.x, v.y) | __builtin_isunordered(v.z, v.w);
        const float w0 = weight<DIVIDE>(v.x, a.inv_t, a.t), w1 = weight<DIVIDE>(v.y, a.inv_t, a.t);
        const float w2 = weight<DIVIDE>(v.z, a.inv_t, a.t), w3 = weight<DIVIDE>(v.w, a.inv_t, a.t);
        sw += (double)((w0 + w1) + (w2 + w3));
    };
    if ((n & 3) == 0 && (((uintptr_t)p) & 15) == 0) {
        const int n4 = n >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(p);
        int i = tid;
        for (; i + 7 * 256 < n4; i += 8 * 256) {     // eight independent 16-byte loads in flight per thread
            const float4 v0 = p4[i], v1 = p4[i + 256], v2 = p4[i + 512], v3 = p4[i + 768];
            const float4 v4 = p4[i + 1024], v5 = p4[i + 1280], v6 = p4[i + 1536], v7 = p4[i + 1792];
            __builtin_amdgcn_sched_barrier(0);      // (all eight issued before the first is consumed)
            fold(v0);      // (a fence after each fold, as in compliance.hip: left alone the scheduler runs the eight side by side)
            __builtin_amdgcn_sched_barrier(0);
            fold(v1);
            __builtin_amdgcn_sched_barrier(0);
            fold(v2);
            __builtin_amdgcn_sched_barrier(0);
            fold(v3);
            __builtin_amdgcn_sched_barrier(0);
            fold(v4);
            __builtin_amdgcn_sched_barrier(0);
            fold(v5);
            __builtin_amdgcn_sched_barrier(0);
            fold(v6);
            __builtin_amdgcn_sched_barrier(0);
            fold(v7);
        }
        for (; i < n4; i += 256) fold(p4[i]);
    } else {
        // A plane off its boundary, or one that does not end on one: element-wise loads, the pixels still four at a time, by the same
        // threads in the same order and through the same fold, so a plane gives the same bits whichever path its address sends it down.
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += 256) {
            const float* q = p + 4 * (long long)i;
            fold(make_float4(q[0], q[1], q[2], q[3]));
        }
        for (int i = (n4 << 2) + tid; i < n; i += 256) fold1(p[i]);
    }
    sw = wave_sum(sw);
    const int any_poison = __any(poison);
    if ((tid & 63) == 0) {
        ws[tid >> 6] = sw;
        wpoison[tid >> 6] = any_poison;
    }
    __syncthreads();
    if (tid == 0) {
        const double Z = four_wave_sum(ws, 1);
        const bool bad = four_wave_poison(wpoison) || Z == 0.0;
        a.rz[plane] = bad ? __builtin_nan("") : 1.0 / Z;      // (the NaN travels: every m, D, product and partial it enters is NaN)
    }
}

// ---- 2. the walk over a group's agents --------------------------------------------------------------------------------------------------
struct AccArgs {
    const float* x;
    long long bs;
    const int* offsets;     // device, [G + 1]
    long long B;
    int C, H, W, Hc, Wc;
    int pwn;                // patches along a row of the map
    int P;                  // patches per plane
    int T;                  // tiles of 64 patches per plane
    int wvec;               // W % 4 == 0: a plane on a 16-byte boundary is read in 16-byte vectors
    float t, inv_t;
    const double* rz;       // [B * C]
    double* cpart;          // [G * C * T]: 1/2 (D^2 - sum m^2) over the tile's cells
    double* rpart;          // [B * C * T]: sum m (D - m) over the tile's cells, per agent; null: risk is not wanted
    float* occ;
    float* any;             // or null
    int* status;
};

// CELL: the cell edge; DIVIDE: T != 1.  A patch is PW = max(4, CELL) pixels wide and CELL rows high: NV 16-byte vectors per row,
// NL = CELL * NV loads per agent, NC = PW / CELL cells.  DEPTH agents' loads are issued before the first is consumed: 8 vectors in
// flight per thread as in the sibling kernels (one agent's 16 at CELL 8).  SPLIT waves share a tile's agents: one per four pixels of the
// patch (at most 8: at CELL 8 the kernel needs more than the 128 registers a workgroup of 16 waves leaves a thread), so that a plane is
// spread over as many waves at CELL 1, 2 and 4 (a 256 x 256 plane: 256) and half as many at CELL 8.
template <int CELL>
struct Patch {
    static constexpr int PW = CELL < 4 ? 4 : CELL;
    static constexpr int NV = PW / 4;
    static constexpr int NL = CELL * NV;
    static constexpr int NC = PW / CELL;
    static constexpr int DEPTH = NL >= 8 ? 1 : 8 / NL;
    static constexpr int SPLIT = NL > 8 ? 8 : NL;
};

template <int CELL, bool DIVIDE>
__global__ __launch_bounds__(64 * Patch<CELL>::SPLIT) void occupancy_accumulate_kernel(const AccArgs a) {
    using G = Patch<CELL>;
    constexpr int PW = G::PW, NV = G::NV, NL = G::NL, NC = G::NC, DEPTH = G::DEPTH, SPLIT = G::SPLIT;
    __shared__ double shared[SPLIT > 1 ? SPLIT : 1][3 * NC][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long blk = blockIdx.x;
    const int tile = (int)(blk % a.T);
    const long long gc = blk / a.T;
    const int c = (int)(gc % a.C);
    const long long g = gc / a.C;
    const int n = a.H * a.W;
    // this thread's patch, and its cells
    const int p = tile * 64 + lane;
    const bool live = p < a.P;
    const int prow = live ? p / a.pwn : 0, pcol = live ? p % a.pwn : 0;
    const int y0 = prow * CELL, x0 = pcol * PW;
    const long long obase = (gc * a.Hc + prow) * (long long)a.Wc + (long long)pcol * NC;
    bool cell_in[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) cell_in[k] = live && pcol * NC + k < a.Wc;
    const long long lo = a.offsets[g], hi = a.offsets[g + 1];
    if (!(0 <= lo && lo <= hi && hi <= a.B)) {      // bounds that do not name rows of x: nothing is addressed through them
        const float nan = __builtin_nanf("");
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if (cell_in[k] && wv == 0) {
                a.occ[obase + k] = nan;
                if (a.any) a.any[obase + k] = nan;
            }
        }
        if (threadIdx.x == 0) {
            a.cpart[blk] = __builtin_nan("");
            if (tile == 0 && c == 0) atomicOr(a.status, 2);
        }
        return;
    }
    const float ninf = -__builtin_inff();      // a pixel outside the map: w = 0 exactly, it adds 0 wherever it enters
    // one agent's patch.  Both paths deliver the same NL vectors, so the sums below do not depend on where a plane starts.
    auto load = [&](const long long row, float4 (&v)[NL]) {
        const float* __restrict__ pl = a.x + row * a.bs + (long long)c * n;
        const bool vec = a.wvec != 0 && (((uintptr_t)pl) & 15) == 0;
#pragma unroll
        for (int r = 0; r < CELL; ++r) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int y = y0 + r, xx = x0 + 4 * j;
                float4 q = make_float4(ninf, ninf, ninf, ninf);
                if (live && y < a.H && xx < a.W) {
                    const float* s = pl + ((long long)y * a.W + xx);
                    if (vec) {      // (W % 4 == 0 and xx % 4 == 0: the whole vector is inside the row)
                        q = *reinterpret_cast<const float4*>(s);
                    } else {
                        q.x = s[0];
                        if (xx + 1 < a.W) q.y = s[1];
                        if (xx + 2 < a.W) q.z = s[2];
                        if (xx + 3 < a.W) q.w = s[3];
                    }
                }
                v[r * NV + j] = q;
            }
        }
    };
    // the fp32 sum of w over each cell of the patch, in a fixed order: per row the cell's pixels in a balanced tree, the rows one after
    // the other -> m = (float)((double)s / Z)
    auto shares = [&](const float4 (&v)[NL], const double rz, float (&m)[NC]) {
        float s[NC];
#pragma unroll
        for (int r = 0; r < CELL; ++r) {
            float q[NC];
            if constexpr (CELL == 1) {
                const float4 u = v[r];
                q[0] = weight<DIVIDE>(u.x, a.inv_t, a.t);
                q[1] = weight<DIVIDE>(u.y, a.inv_t, a.t);
                q[2] = weight<DIVIDE>(u.z, a.inv_t, a.t);
                q[3] = weight<DIVIDE>(u.w, a.inv_t, a.t);
            } else if constexpr (CELL == 2) {
                const float4 u = v[r];
                q[0] = weight<DIVIDE>(u.x, a.inv_t, a.t) + weight<DIVIDE>(u.y, a.inv_t, a.t);
                q[1] = weight<DIVIDE>(u.z, a.inv_t, a.t) + weight<DIVIDE>(u.w, a.inv_t, a.t);
            } else {
                float h[NV];
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const float4 u = v[r * NV + j];
                    h[j] = (weight<DIVIDE>(u.x, a.inv_t, a.t) + weight<DIVIDE>(u.y, a.inv_t, a.t))
                           + (weight<DIVIDE>(u.z, a.inv_t, a.t) + weight<DIVIDE>(u.w, a.inv_t, a.t));
                }
                if constexpr (NV == 1) q[0] = h[0];
                else q[0] = h[0] + h[1];
            }
#pragma unroll
            for (int k = 0; k < NC; ++k) s[k] = r == 0 ? q[k] : s[k] + q[k];
        }
#pragma unroll
        for (int k = 0; k < NC; ++k) m[k] = (float)((double)s[k] * rz);
    };
    // this wave's run of the group's agents (the split depends on the group's size alone)
    const long long per = (hi - lo + SPLIT - 1) / SPLIT;
    const long long wlo = lo + wv * per < hi ? lo + wv * per : hi, whi = wlo + per < hi ? wlo + per : hi;
    // DEPTH agents' loads issued before the first is consumed, then the agents left one by one: the same adds in the same order
    auto walk = [&](auto&& consume) {
        long long r = wlo;
        for (; r + DEPTH <= whi; r += DEPTH) {
            float4 v[DEPTH][NL];
            double rz[DEPTH];
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {
                load(r + d, v[d]);
                rz[d] = a.rz[(r + d) * a.C + c];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {
                float m[NC];
                shares(v[d], rz[d], m);
                consume(r + d, m);
            }
        }
        for (; r < whi; ++r) {
            float4 v[NL];
            load(r, v);
            float m[NC];
            shares(v, a.rz[r * a.C + c], m);
            consume(r, m);
        }
    };
    // D, sum m^2 and prod (1 - m) per cell, owned by this thread alone.  m is an fp32 value: m * m is exact in fp64.
    double D[NC], S2[NC], Q[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        D[k] = 0.0;
        S2[k] = 0.0;
        Q[k] = 1.0;
    }
    walk([&](const long long, const float (&m)[NC]) {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const double md = (double)m[k];
            D[k] += md;
            S2[k] += md * md;
            Q[k] *= 1.0 - md;
        }
    });
    if constexpr (SPLIT > 1) {      // the waves' runs joined in wave order, by every wave for itself: each needs D for its second walk
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            shared[wv][3 * k][lane] = D[k];
            shared[wv][3 * k + 1][lane] = S2[k];
            shared[wv][3 * k + 2][lane] = Q[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            D[k] = shared[0][3 * k][lane];
            S2[k] = shared[0][3 * k + 1][lane];
            Q[k] = shared[0][3 * k + 2][lane];
            for (int w = 1; w < SPLIT; ++w) {      // (a wave with no agent adds 0 and multiplies by 1: exact)
                D[k] += shared[w][3 * k][lane];
                S2[k] += shared[w][3 * k + 1][lane];
                Q[k] *= shared[w][3 * k + 2][lane];
            }
        }
    }
    if (wv == 0) {
        double part = 0.0;      // (a cell outside the map holds zeros alone: it adds 0)
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            if (cell_in[k]) {
                a.occ[obase + k] = (float)D[k];
                if (a.any) a.any[obase + k] = (float)(1.0 - Q[k]);
            }
            part += 0.5 * (D[k] * D[k] - S2[k]);
        }
        part = wave_sum(part);
        if (lane == 0) {
            a.cpart[blk] = part;
            if (tile == 0 && D[0] != D[0]) atomicOr(a.status, 1);      // (patch 0 of the plane: a poisoned (g, c) is NaN in every cell)
        }
    }
    if (a.rpart == nullptr) return;
    // the second walk: every agent's share of the tile's pairs, the planes read again (through the caches where they still are)
    walk([&](const long long row, const float (&m)[NC]) {
        double rp = 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const double md = (double)m[k];
            rp += md * (D[k] - md);
        }
        rp = wave_sum(rp);
        if (lane == 0) a.rpart[(row * a.C + c) * a.T + tile] = rp;
    });
}

// ---- 3. the tile partials, summed ------------------------------------------------------------------------------------------------------
struct CombArgs {
    const int* offsets;
    long long B, G;
    int C, T;
    long long nconf;        // G * C when conflict is wanted, else 0: the first nconf workgroups sum conflicts, the others risks
    const double* cpart;
    const double* rpart;
    float* conflict;
    float* risk;
};

// One wave per result: lane l adds tiles l, l + 64, ... in that order, then the lanes' sums are added in wave_sum's tree.
__global__ __launch_bounds__(64) void occupancy_combine_kernel(const CombArgs a) {
    const int lane = threadIdx.x;
    const long long blk = blockIdx.x;
    const double* src;
    float* dst;
    if (blk < a.nconf) {
        src = a.cpart + blk * a.T;
        dst = a.conflict + blk;
    } else {
        const long long rc = blk - a.nconf, row = rc / a.C;
        // the group of this row: the last one whose first row is not beyond it (the bounds of legal groups ascend)
        long long g0 = 0, g1 = a.G;
        while (g1 - g0 > 1) {
            const long long mid = (g0 + g1) >> 1;
            if ((long long)a.offsets[mid] <= row) g0 = mid;
            else g1 = mid;
        }
        const long long lo = a.offsets[g0], hi = a.offsets[g0 + 1];
        dst = a.risk + rc;
        if (!(0 <= lo && lo <= hi && hi <= a.B)) {      // a group with bad bounds: NaN from its first row on, no partial was written
            if (lane == 0 && lo <= row) *dst = __builtin_nanf("");
            return;
        }
        if (row < lo || row >= hi) return;               // a row of no group: not written
        src = a.rpart + rc * a.T;
    }
    double s = 0.0;
    for (int i = lane; i < a.T; i += 64) s += src[i];
    s = wave_sum(s);
    if (lane == 0) *dst = (float)s;
}

bool cell_ok(int cell) { return cell == 1 || cell == 2 || cell == 4 || cell == 8; }

// patches per plane and tiles of 64 patches
void plan(int H, int W, int cell, int* pwn, long long* P, long long* T) {
    const int pw = cell < 4 ? 4 : cell;
    *pwn = (W + pw - 1) / pw;
    *P = (long long)*pwn * ((H + cell - 1) / cell);
    *T = (*P + 63) / 64;
}

template <bool DIVIDE>
void launch_accumulate(int cell, long long blocks, const AccArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)blocks), block(64 * (cell == 1 ? 1 : cell == 2 ? 2 : cell == 4 ? 4 : 8));      // Patch<cell>::SPLIT waves
    switch (cell) {
    case 1: hipLaunchKernelGGL((occupancy_accumulate_kernel<1, DIVIDE>), grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((occupancy_accumulate_kernel<2, DIVIDE>), grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((occupancy_accumulate_kernel<4, DIVIDE>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((occupancy_accumulate_kernel<8, DIVIDE>), grid, block, 0, stream, a); break;
    }
}

}  // namespace

static_assert(YNET_MAP_OCCUPANCY_MAX_CELL == 8, "the cell switch above covers 1, 2, 4, 8");

extern "C" long long ynet_map_occupancy_workspace_bytes(long long B, int C, int H, int W, long long G, int cell) {
    if (!(B >= 1 && C >= 1 && H >= 1 && W >= 1 && G >= 1 && cell_ok(cell)) || (long long)H * W > (1ll << 31) - 2048) {
        ynet_set_error("map_occupancy_workspace_bytes: bad shape B=%lld C=%d %dx%d G=%lld cell=%d", B, C, H, W, G, cell);
        return -1;
    }
    int pwn;
    long long P, T;
    plan(H, W, cell, &pwn, &P, &T);
    if (B * C >= (1ll << 31) || G * C >= (1ll << 31) / T) {
        ynet_set_error("map_occupancy_workspace_bytes: too many planes or tiles (B=%lld G=%lld C=%d, %lld tiles per plane)", B, G, C, T);
        return -1;
    }
    return 8 * (B * C + G * C * T + B * C * T);
}

extern "C" int ynet_map_occupancy(const float* x, long long batch_stride, const int* offsets, long long B, long long G, int C, int H, int W,
                                  int cell, float temperature, float* occupancy, float* any, float* conflict, float* risk,
                                  void* workspace, int* status, void* stream) {
    YNET_REQUIRE(x != nullptr, "map_occupancy: null map");
    YNET_REQUIRE(offsets != nullptr, "map_occupancy: null offsets");
    YNET_REQUIRE(occupancy != nullptr, "map_occupancy: null output (occupancy)");
    YNET_REQUIRE(workspace != nullptr, "map_occupancy: null workspace");
    YNET_REQUIRE((((uintptr_t)workspace) & 7) == 0, "map_occupancy: the workspace must start on an 8-byte boundary");
    YNET_REQUIRE(status != nullptr, "map_occupancy: null status flag");
    YNET_REQUIRE(cell_ok(cell), "map_occupancy: cell = %d, expected 1, 2, 4 or %d", cell, YNET_MAP_OCCUPANCY_MAX_CELL);
    if (map_check_temperature("map_occupancy", temperature)) return 1;
    YNET_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1 && G >= 1, "map_occupancy: bad shape B=%lld C=%d %dx%d G=%lld", B, C, H, W, G);
    if (map_check_pixel_index("map_occupancy", H, W) || map_check_batch_stride("map_occupancy", batch_stride, C, H, W)) return 1;
    int pwn;
    long long P, T;
    plan(H, W, cell, &pwn, &P, &T);
    YNET_REQUIRE(B * C < (1ll << 31), "map_occupancy: too many planes");
    YNET_REQUIRE(G * C < (1ll << 31) / T, "map_occupancy: too many tiles (%lld groups x %d steps x %lld tiles per plane)", G, C, T);
    const hipStream_t s = (hipStream_t)stream;
    double* ws = static_cast<double*>(workspace);
    NormArgs na;
    na.x = x;
    na.bs = batch_stride;
    na.C = C;
    na.H = H;
    na.W = W;
    na.t = temperature;
    na.inv_t = 1.f / temperature;
    na.rz = ws;
    if (temperature == 1.f) hipLaunchKernelGGL((occupancy_normalise_kernel<false>), dim3((unsigned)(B * C)), dim3(256), 0, s, na);
    else hipLaunchKernelGGL((occupancy_normalise_kernel<true>), dim3((unsigned)(B * C)), dim3(256), 0, s, na);
    AccArgs a;
    a.x = x;
    a.bs = batch_stride;
    a.offsets = offsets;
    a.B = B;
    a.C = C;
    a.H = H;
    a.W = W;
    a.Hc = (H + cell - 1) / cell;
    a.Wc = (W + cell - 1) / cell;
    a.pwn = pwn;
    a.P = (int)P;
    a.T = (int)T;
    a.wvec = (W & 3) == 0;
    a.t = temperature;
    a.inv_t = 1.f / temperature;
    a.rz = ws;
    a.cpart = ws + B * C;
    a.rpart = risk != nullptr ? ws + B * C + G * C * T : nullptr;
    a.occ = occupancy;
    a.any = any;
    a.status = status;
    if (temperature == 1.f) launch_accumulate<false>(cell, G * C * T, a, s);
    else launch_accumulate<true>(cell, G * C * T, a, s);
    if (conflict != nullptr || risk != nullptr) {
        CombArgs ca;
        ca.offsets = offsets;
        ca.B = B;
        ca.G = G;
        ca.C = C;
        ca.T = (int)T;
        ca.nconf = conflict != nullptr ? G * C : 0;
        ca.cpart = a.cpart;
        ca.rpart = a.rpart;
        ca.conflict = conflict;
        ca.risk = risk;
        const long long blocks = ca.nconf + (risk != nullptr ? B * C : 0);
        YNET_REQUIRE(blocks < (1ll << 31), "map_occupancy: too many results to combine");
        hipLaunchKernelGGL(occupancy_combine_kernel, dim3((unsigned)blocks), dim3(64), 0, s, ca);
    }
    return ynet_check_launch("map_occupancy");
}
